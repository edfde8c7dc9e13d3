"""Every exit of the five `find` runs on the device (find_run of csrc/mtg_gpu_misc.hip: find_gap_run with its four observers, find_het_run), for
both entries of each (mtg_index_find_*_sequences / _packed_device), on the inputs of tests/find_stage_cases.py: k = 13, at most four sequences
of at most 200 nt (one of 310 nt for the multi-SNP layer), one index.  Calls and statistics against the plain models; tests/test_find_stages_cpu.py shows that every input is the stage
it is named after."""
import functools

import numpy as np
import pytest

from tests import find_cases as fc
from tests import find_msnp_cases as fm
from tests import find_stage_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5
GAP_DTYPE = np.dtype([(name, np.uint32) for name in ("seq", "start", "length", "consumed", "n_snps")])
GAP_ROOM = 16


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
    want = {(layer, stage): sc.model(layer, sc.SOLID, seqs) for layer in sc.LAYERS for stage, seqs in sc.inputs(layer).items()}
    want.update({(layer, "all"): sc.model(layer, sc.SOLID, sc.ALL_LAYERS) for layer in sc.LAYERS})
    return want


def tuples(calls):
    return [tuple(int(x) for x in c) for c in calls]


@functools.lru_cache(maxsize=None)
def _gap_records(seqs):
    return tuples(sc.msnp_gap_records(sc.SOLID, list(seqs)))


def gap_records(seqs):
    """the multi-SNP model's gap records of an input, computed once"""
    return _gap_records(tuple(seqs))


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
    """(calls, total, statistics) of the host-string entry; of the multi-SNP layer the gap records too"""
    if layer == "msnp":
        calls, recs, st = idx.find_msnp_sequences(seqs, sc.MAX_REPEAT, sc.SNP_MIN_VAL, cap=cap)
        assert calls.dtype == fc.CALL_DTYPE and recs.dtype == GAP_DTYPE
        return tuples(calls), st["n_calls"], st, tuples(recs)
    if layer == "homo":
        calls, st = idx.find_homo_sequences(seqs, sc.MAX_REPEAT, cap=cap)
    elif layer == "del":
        calls, st = idx.find_del_sequences(seqs, sc.MAX_REPEAT, cap=cap)
    elif layer == "snp":
        calls, st = idx.find_snp_sequences(seqs, sc.MAX_REPEAT, cap=cap)
    else:
        calls, st = idx.find_het_sequences(seqs, None, sc.MAX_REPEAT, sc.BRANCHING, cap=cap)
    assert calls.dtype == fc.CALL_DTYPE
    return tuples(calls), st["n_calls"], st


def by_device(idx, layer, seqs, cap=None, gap_cap=GAP_ROOM):
    """(calls, total, statistics) of the packed device entry; the output array holds a guard pattern, which must be intact behind the
    min(total, cap) records.  cap None: room for 64 calls.  Of the multi-SNP layer the gap records too, their array of gap_cap records
    (None: a NULL array) guarded alike, with the gap total in the statistics as n_gap_records"""
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
    elif layer == "snp":
        total, st = idx.find_snp_packed_device(*ptrs, sc.MAX_REPEAT, *out)
    elif layer == "msnp":
        groom = gap_cap or 0
        d_recs = torch.from_numpy(np.full((groom + 2) * 5, GUARD, dtype=np.uint32).view(np.int32)).to(dev)
        total, gtotal, st = idx.find_msnp_packed_device(*ptrs, sc.MAX_REPEAT, sc.SNP_MIN_VAL, *out, None if gap_cap is None else d_recs.data_ptr(), groom)
        st = dict(st, n_gap_records=gtotal)
    else:
        total, st = idx.find_het_packed_device(*ptrs, None, sc.MAX_REPEAT, sc.BRANCHING, *out)
    torch.cuda.synchronize()
    raw = d_calls.cpu().numpy().view(np.uint32)
    n = min(total, room)
    assert (raw[7 * n:] == GUARD).all(), "the output array was written behind its %d records" % n
    if layer != "msnp":
        return tuples(raw[:7 * n].view(fc.CALL_DTYPE)), total, st
    graw = d_recs.cpu().numpy().view(np.uint32)
    g = min(gtotal, groom)
    assert (graw[5 * g:] == GUARD).all(), "the gap array was written behind its %d records" % g
    return tuples(raw[:7 * n].view(fc.CALL_DTYPE)), total, st, tuples(graw[:5 * g].view(GAP_DTYPE))


ENTRIES = {"sequences": by_strings, "packed_device": by_device}


def same(layer, got, want, seqs):
    """calls, total and statistics of a run are the model's; of the multi-SNP layer the gap records too"""
    calls, total, st = got[:3]
    wcalls, wst = want
    if layer == "msnp":
        assert got[3] == gap_records(seqs) and len(got[3]) == wst["n_candidates"] == st.get("n_gap_records", len(got[3]))
    assert calls == wcalls and total == len(wcalls)
    assert {x: st[x] for x in sc.stat_keys(layer)} == {x: wst[x] for x in sc.stat_keys(layer)}
    assert st["n_positions"] == sum(max(len(s) - sc.K + 1, 0) for s in seqs)


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("layer", sc.LAYERS)
def test_every_exit_of_a_layer(idx, expected, layer, entry):
    """inputs 1-6: no sequence, none of k nt, all in the graph, nothing a candidate, no candidate called, calls with every capacity"""
    run = ENTRIES[entry]
    for stage, seqs in sc.inputs(layer).items():
        same(layer, run(idx, layer, seqs), expected[layer, stage], seqs)
    seqs, (wcalls, wst) = sc.STAGES[layer]["calls"], expected[layer, "calls"]
    n = len(wcalls)
    assert n >= 3
    for cap in (0, 1, n, n + 2):
        calls, total, st = run(idx, layer, seqs, cap)[:3]
        assert total == n and calls == wcalls[:cap], cap
        assert {x: st[x] for x in sc.stat_keys(layer)} == {x: wst[x] for x in sc.stat_keys(layer)}, cap


@pytest.mark.parametrize("stage", ["calls", "unjudged"])
def test_the_gap_records_with_every_capacity(idx, expected, stage):
    """the multi-SNP layer's second output, with and without a slab behind it: gap capacities 0, 1, n and n + 2 and a NULL array, each with
    call capacities 0 and n + 2; the first min(total, cap) records of each output, the guard intact behind them, both totals in every case"""
    seqs, (wcalls, wst) = sc.inputs("msnp")[stage], expected["msnp", stage]
    wrecs = gap_records(seqs)
    n = len(wrecs)
    assert n == wst["n_candidates"] >= 1
    for gap_cap in (0, 1, n, n + 2, None):
        for cap in (0, len(wcalls) + 2):
            calls, total, st, recs = by_device(idx, "msnp", seqs, cap, gap_cap)
            assert total == len(wcalls) and calls == wcalls[:cap] and st["n_gap_records"] == n and recs == wrecs[:gap_cap or 0], (gap_cap, cap)
            assert {x: st[x] for x in fm.STAT_KEYS} == {x: wst[x] for x in fm.STAT_KEYS}, (gap_cap, cap)
    # the host-string entry: with the records, which its array grows to hold, and without (a NULL array and a NULL total)
    calls, recs, st = idx.find_msnp_sequences(seqs, sc.MAX_REPEAT, sc.SNP_MIN_VAL)
    assert tuples(calls) == wcalls and tuples(recs) == wrecs
    calls, recs, st = idx.find_msnp_sequences(seqs, sc.MAX_REPEAT, sc.SNP_MIN_VAL, cap=1, gaps=False)
    assert tuples(calls) == wcalls[:1] and recs is None and st["n_calls"] == len(wcalls) and st["n_candidates"] == n


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_the_layers_one_after_another_and_in_reverse(idx, expected, entry):
    """input 7: the five runs on one index and one input, then in reverse order: nothing of a run reaches the next"""
    run = ENTRIES[entry]
    first = {layer: run(idx, layer, sc.ALL_LAYERS) for layer in sc.LAYERS}
    second = {layer: run(idx, layer, sc.ALL_LAYERS) for layer in reversed(sc.LAYERS)}
    for layer in sc.LAYERS:
        assert expected[layer, "all"][0], layer
        same(layer, first[layer], expected[layer, "all"], sc.ALL_LAYERS)
        same(layer, second[layer], expected[layer, "all"], sc.ALL_LAYERS)
        assert first[layer][:2] == second[layer][:2] and first[layer][3:] == second[layer][3:]
        assert {x: first[layer][2][x] for x in sc.stat_keys(layer)} == {x: second[layer][2][x] for x in sc.stat_keys(layer)}
