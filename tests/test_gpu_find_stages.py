"""Every exit of the three `find` runs on the device (find_homo_run, find_del_run, find_het_run on the FindStage of csrc/mtg_gpu_misc.hip), for
both entries of each (mtg_index_find_*_sequences / _packed_device), on the inputs of tests/find_stage_cases.py: k = 13, at most four sequences
of at most 200 nt, one index.  Calls and statistics against the plain models; tests/test_find_stages_cpu.py shows that every input is the stage
it is named after."""
import numpy as np
import pytest

from tests import find_cases as fc
from tests import find_stage_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5


@pytest.fixture(scope="module")
def idx():
    import torch
    torch.cuda.init()  # torch bundles its own HIP runtime: initialise it before libmtgfill.so touches the device
    import mindthegap_amd
    mindthegap_amd.load_library()
    assert mindthegap_amd.device_count() >= 1, "these tests need a HIP device"
    kms = np.array(sorted(sc.SOLID), dtype=np.uint64)
    index = mindthegap_amd.Index.from_kmers(kms, np.full(len(kms), 9, dtype=np.uint32), sc.K)
    yield index
    index.close()


@pytest.fixture(scope="module")
def expected():
    """the models' (calls, statistics) of every input, computed once"""
    want = {(layer, stage): sc.model(layer, sc.SOLID, seqs) for layer in sc.LAYERS for stage, seqs in sc.STAGES[layer].items()}
    want.update({(layer, "all"): sc.model(layer, sc.SOLID, sc.ALL_LAYERS) for layer in sc.LAYERS})
    return want


def tuples(calls):
    return [tuple(int(x) for x in c) for c in calls]


def pack(seqs):
    """(packed words, word offsets, lengths) in the layout of mtg_index_profile_packed_device"""
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    word_off = np.zeros(len(seqs), dtype=np.uint64)
    nw = 0
    for i, n in enumerate(lens):
        word_off[i] = nw
        nw += (int(n) + 31) // 32 + 1
    packed = np.zeros(nw + 1, dtype=np.uint64)
    for i, s in enumerate(seqs):
        codes = (np.frombuffer(s.encode(), dtype=np.uint8).astype(np.uint64) >> np.uint64(1)) & np.uint64(3)
        for j0 in range(0, len(s), 32):
            c = codes[j0:j0 + 32]
            packed[int(word_off[i]) + (j0 >> 5)] = np.bitwise_or.reduce(c << (np.arange(len(c), dtype=np.uint64) * np.uint64(2)))
    return packed, word_off, lens


def by_strings(idx, layer, seqs, cap=None):
    """(calls, total, statistics) of the host-string entry"""
    if layer == "homo":
        calls, st = idx.find_homo_sequences(seqs, sc.MAX_REPEAT, cap=cap)
    elif layer == "del":
        calls, st = idx.find_del_sequences(seqs, sc.MAX_REPEAT, cap=cap)
    else:
        calls, st = idx.find_het_sequences(seqs, None, sc.MAX_REPEAT, sc.BRANCHING, cap=cap)
    assert calls.dtype == fc.CALL_DTYPE
    return tuples(calls), st["n_calls"], st


def by_device(idx, layer, seqs, cap=None):
    """(calls, total, statistics) of the packed device entry; the output array holds a guard pattern, which must be intact behind the
    min(total, cap) records.  cap None: room for 64 calls"""
    import torch
    room = 64 if cap is None else cap
    packed, word_off, lens = pack(seqs)
    dev = torch.device("cuda", 0)
    d_w = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_wo = torch.from_numpy(word_off.view(np.int64)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_calls = torch.from_numpy(np.full((room + 2) * 7, GUARD, dtype=np.uint32).view(np.int32)).to(dev)
    ptrs = (d_w.data_ptr(), d_wo.data_ptr() or None, d_ln.data_ptr() or None, len(seqs))
    out = (d_calls.data_ptr() if room else None, room)
    if layer == "homo":
        total, st = idx.find_homo_packed_device(*ptrs, sc.MAX_REPEAT, *out)
    elif layer == "del":
        total, st = idx.find_del_packed_device(*ptrs, sc.MAX_REPEAT, *out)
    else:
        total, st = idx.find_het_packed_device(*ptrs, None, sc.MAX_REPEAT, sc.BRANCHING, *out)
    torch.cuda.synchronize()
    raw = d_calls.cpu().numpy().view(np.uint32)
    n = min(total, room)
    assert (raw[7 * n:] == GUARD).all(), "the output array was written behind its %d records" % n
    return tuples(raw[:7 * n].view(fc.CALL_DTYPE)), total, st


ENTRIES = {"sequences": by_strings, "packed_device": by_device}


def same(layer, got, want, seqs):
    """calls, total and statistics of a run are the model's"""
    calls, total, st = got
    wcalls, wst = want
    assert calls == wcalls and total == len(wcalls)
    assert {x: st[x] for x in sc.stat_keys(layer)} == {x: wst[x] for x in sc.stat_keys(layer)}
    assert st["n_positions"] == sum(max(len(s) - sc.K + 1, 0) for s in seqs)


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("layer", sc.LAYERS)
def test_every_exit_of_a_layer(idx, expected, layer, entry):
    """inputs 1-6: no sequence, none of k nt, all in the graph, nothing a candidate, no candidate called, calls with every capacity"""
    run = ENTRIES[entry]
    for stage in sc.STAGE_NAMES:
        seqs = sc.STAGES[layer][stage]
        same(layer, run(idx, layer, seqs), expected[layer, stage], seqs)
    seqs, (wcalls, wst) = sc.STAGES[layer]["calls"], expected[layer, "calls"]
    n = len(wcalls)
    assert n >= 3
    for cap in (0, 1, n, n + 2):
        calls, total, st = run(idx, layer, seqs, cap)
        assert total == n and calls == wcalls[:cap], cap
        assert {x: st[x] for x in sc.stat_keys(layer)} == {x: wst[x] for x in sc.stat_keys(layer)}, cap


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_the_layers_one_after_another_and_in_reverse(idx, expected, entry):
    """input 7: the three runs on one index and one input, then in reverse order: nothing of a run reaches the next"""
    run = ENTRIES[entry]
    first = {layer: run(idx, layer, sc.ALL_LAYERS) for layer in sc.LAYERS}
    second = {layer: run(idx, layer, sc.ALL_LAYERS) for layer in reversed(sc.LAYERS)}
    for layer in sc.LAYERS:
        assert expected[layer, "all"][0], layer
        same(layer, first[layer], expected[layer, "all"], sc.ALL_LAYERS)
        same(layer, second[layer], expected[layer, "all"], sc.ALL_LAYERS)
        assert first[layer][:2] == second[layer][:2]
        assert {x: first[layer][2][x] for x in sc.stat_keys(layer)} == {x: second[layer][2][x] for x in sc.stat_keys(layer)}
