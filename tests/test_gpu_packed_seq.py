"""The packed link path of a batch's sequence arena (PACKED_SEQ_SHARE of the tuning table): the tail of a whole-batch launch's arena crosses as
2-bit codes and the host expands it.  Records and sequence bytes must be those of the all-ASCII path (share 0) for every share, and the cases
that keep the ASCII path (several launches, an arena that grows) must still give them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHARES = ("0", "0.5", "1")


@pytest.fixture(scope="module")
def mtg():
    import torch
    torch.cuda.init()  # torch bundles its own HIP runtime: initialise it before libmtgfill.so touches the device
    import mindthegap_amd
    mindthegap_amd.load_library()
    assert mindthegap_amd.device_count() >= 1, "these tests need a HIP device"
    return mindthegap_amd


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _index(mtg, S):
    import torch
    pw, po, pl, pn = S.packed()
    w = torch.from_numpy(pw.view(np.int64)).cuda()
    wo = torch.from_numpy(po.view(np.int64)).cuda()
    ln = torch.from_numpy(pl.view(np.int32)).cuda()
    idx = mtg.Index.from_packed_device(w.data_ptr(), wo.data_ptr(), ln.data_ptr(), pn, S.total_kmers_upper_bound, 31, 3, 0)
    torch.cuda.synchronize()
    return idx


def _gaps(mtg, S, reverse_every=0):
    gaps = []
    for i in range(S.n_sites):
        l, r, _ = S.site(i)
        if reverse_every and i % reverse_every == 1:  # the reverse attempt: from the right anchor's complement, fills come back complemented
            gaps.append(mtg.Gap(_rc(r), _rc(l), [(_rc(l), S.site_name(i), False)], reverse=True))
        else:
            gaps.append(mtg.Gap(l, r, [(r, S.site_name(i), False)]))
    return gaps


def _prepared_bytes(idx, prep):
    h, nf, seqs = idx.fill_prepared(prep)
    idx.free_results(h)
    return nf.tobytes(), seqs.tobytes()


def _runs(mtg, idx, gaps, monkeypatch, capfd):
    """per share: two fill_batch calls (the second on a recycled, large enough arena) and one prepared batch; what the debug timers said"""
    prep = idx.prepare_batch(gaps)
    out = {}
    monkeypatch.setenv("MTG_DEBUG_TIMERS", "1")
    for s in SHARES:
        monkeypatch.setenv("MTG_PACKED_SEQ_SHARE", s)
        capfd.readouterr()
        got = (idx.fill_batch(gaps), idx.fill_batch(gaps), _prepared_bytes(idx, prep))
        out[s] = (got, "packed tail" in capfd.readouterr().err)
    monkeypatch.delenv("MTG_DEBUG_TIMERS")
    prep.close()
    return out


def _check_same(out, want_packed=True):
    ref, used = out["0"]
    assert not used, "share 0 took the packed path"
    assert sum(len(r["filled"]) for r in ref[0]) > 0
    for s in SHARES[1:]:
        got, used = out[s]
        assert used == want_packed, (s, used)
        for a, b in zip(got, ref):
            assert a == b, s


@pytest.mark.parametrize("kind", ["haploid", "het", "indel", "tips"])
def test_packed_share_gives_the_ascii_results(mtg, monkeypatch, capfd, kind):
    """every share: the same records (every field) and sequence bytes; haploid with forward and reverse attempts, the divergence-heavy sets with
    their multi-contig gaps (the host writes those fills after the expansion)"""
    from mindthegap_amd.synth import SynthSet
    het = 4 if kind in ("het", "indel") else 0
    S = SynthSet(nseq=3000 * (2 if het else 1), n_sites=3000, seed=17, het_snps=het, het_indels=2 if kind == "indel" else 0,
                 tips=1.0 / 3.0 if kind == "tips" else 0.0)
    idx = _index(mtg, S)
    gaps = _gaps(mtg, S, reverse_every=5 if kind == "haploid" else 0)
    out = _runs(mtg, idx, gaps, monkeypatch, capfd)
    _check_same(out)
    if kind == "haploid":
        res = out["1"][0][1]
        for i in range(S.n_sites):
            if i % 5 != 1:
                assert [f["seq"] for f in res[i]["filled"]] == [S.site(i)[2]], i
        assert any(res[i]["filled"] for i in range(1, S.n_sites, 5))
    idx.close()


def test_packed_share_with_multi_contig_gaps(mtg, monkeypatch, capfd):
    """single-allele sites (the device writes their fills into the arena, packed in its tail) between two-allele sites whose several solutions
    the host writes after the expansion"""
    import random
    from tests import oracle_lib
    rng = random.Random(31)
    rs = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    seqs, sites = [], []
    for i in range(600):
        L, R, a = rs(300), rs(300), rs(rng.randrange(50, 900))
        seqs.append(L + a + R)
        if i % 3 == 0:  # a second allele the bubble code cannot merge
            seqs.append(L + rs(rng.randrange(150, 900)) + R)
        sites.append((L[-31:], R[:31]))
    o = oracle_lib.Index.from_sequences(seqs, 31, 3, 40)
    km, ct = o.export()
    o.close()
    idx = mtg.Index.from_kmers(km, ct, 31)
    gaps = [mtg.Gap(l, r, [(r, "s%d" % i, False)]) for i, (l, r) in enumerate(sites)]
    out = _runs(mtg, idx, gaps, monkeypatch, capfd)
    _check_same(out)
    res = out["1"][0][1]
    assert sum(len(r["filled"]) > 1 for r in res) > 20 and sum(len(r["filled"]) == 1 for r in res) > 300
    idx.close()


def test_packed_share_falls_back_for_several_launches(mtg, monkeypatch, capfd):
    """MAX_CHUNK: a batch of several launches keeps the ASCII path, whatever the share"""
    from mindthegap_amd.synth import SynthSet
    S = SynthSet(nseq=1500, n_sites=1500, seed=19)
    idx = _index(mtg, S)
    monkeypatch.setenv("MTG_MAX_CHUNK", "397")
    out = _runs(mtg, idx, _gaps(mtg, S, reverse_every=4), monkeypatch, capfd)
    _check_same(out, want_packed=False)
    idx.close()


def test_packed_share_on_a_first_batch_whose_arena_grows(mtg, monkeypatch, capfd):
    """a result object fresh from the allocator has room for 64 characters a gap: the first launch finds its arena too small, grows it and emits
    again in ASCII; the next batch on the grown object takes the packed path.  Both give the share-0 results."""
    from mindthegap_amd.synth import SynthSet
    S = SynthSet(nseq=2000, n_sites=2000, seed=23, ins_min=300, ins_max=1000)
    idx = _index(mtg, S)
    gaps = _gaps(mtg, S)
    small = mtg.Index.prepare_gaps(gaps[:10])
    monkeypatch.setenv("MTG_DEBUG_TIMERS", "1")
    out = {}
    for s in SHARES:
        monkeypatch.setenv("MTG_PACKED_SEQ_SHARE", s)
        held = [idx.fill_prepared(small, want_seqs=False)[0] for _ in range(16)]  # every recycled result object (at most 12) taken: the next one is new
        capfd.readouterr()
        first = idx.fill_batch(gaps)
        first_packed = "packed tail" in capfd.readouterr().err
        second = idx.fill_batch(gaps)  # on the object the first call grew (the held ones are still out)
        second_packed = "packed tail" in capfd.readouterr().err
        for h in held:
            idx.free_results(h)
        out[s] = (first, second, first_packed, second_packed)
    for s in SHARES:
        assert out[s][0] == out["0"][0] and out[s][1] == out["0"][0], s
        assert not out[s][2], "the grown arena's launch must stay ASCII"
    assert out["1"][3] and out["0.5"][3] and not out["0"][3]
    idx.close()
