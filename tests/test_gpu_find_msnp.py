"""`find` for close homozygous SNPs on the device (k_gap_mark<MultiObserver>, k_msnp_bound, k_msnp_judge, k_msnp_emit, k_msnp_gaps in
csrc/mtg_gpu_misc.hip behind mtg_index_find_msnp_sequences / _packed_device and `MindTheGap find -multi-snps | -solo-snps -multi-snps`)
against the plain model of tests/find_msnp_cases.py: the literal FindMultiSNP::update with the literal snp_at_end and correct_history on a
ring of 256 slots inside the literal loop of the scan; gaps of 255 positions and more are not judged (the documented deviation).  Every
comparison is exact -- calls, per-gap records and statistics -- through both entries.

An index takes 11 <= k <= 31, so the small sizes here are k = 11 and 13 (the CPU tests go down to k = 5, where alternatives compete by
chance; here they compete by construction: several donors that differ at the same places).  A case is a sequence and the k-mers of one or
more donors, each donor the sequence with some nucleotides substituted."""
import os
import subprocess

import numpy as np
import pytest

from tests import find_cases as fc
from tests import find_del_cases as fd
from tests import find_het_cases as fh
from tests import find_msnp_cases as fm
from tests import find_snp_cases as fs
from tests import profile_cases as pc
from tests.test_gpu_find_snp import index_of, pack, run_tool, tuples

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FASTQ_PAIR = [os.path.join(GOLDEN, "data", "reads_r1.fastq"), os.path.join(GOLDEN, "data", "reads_r2.fastq")]
REFERENCE = os.path.join(GOLDEN, "full_test", "reference.fasta")
K, CUTOFF, MAX_REPEAT, BRANCHING, M = 31, 7, 5, 15, 5
GOLDEN_CALLS = [("Seq1", 206, "G", "C"), ("Seq1", 219, "T", "A"), ("Seq2", 320, "T", "C"), ("Seq2", 344, "C", "A"), ("Seq3", 766, "G", "A")]


@pytest.fixture(scope="module")
def mtg():
    import torch
    torch.cuda.init()  # torch bundles its own HIP runtime: initialise it before libmtgfill.so touches the device
    import mindthegap_amd
    mindthegap_amd.load_library()
    assert mindthegap_amd.device_count() >= 1, "these tests need a HIP device"
    return mindthegap_amd


def packed_device(idx, seqs, m, cap, gap_cap):
    """(total calls, calls, total gaps, gap records, stats, the input words after the run) of the packed device entry"""
    import torch
    packed, word_off, lens = pack(seqs)
    dev = torch.device("cuda", 0)
    d_w = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_wo = torch.from_numpy(word_off.view(np.int64)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_calls = torch.full((max(cap, 1) * 7 + 7,), -1, dtype=torch.int32, device=dev)
    d_gaps = torch.full((max(gap_cap, 1) * 5 + 5,), -1, dtype=torch.int32, device=dev)
    total, gtotal, st = idx.find_msnp_packed_device(d_w.data_ptr(), d_wo.data_ptr(), d_ln.data_ptr(), len(seqs), MAX_REPEAT, m, d_calls.data_ptr() if cap else None, cap,
                                                    d_gaps.data_ptr() if gap_cap else None, gap_cap)
    torch.cuda.synchronize()
    raw, graw = d_calls.cpu().numpy().view(np.uint32), d_gaps.cpu().numpy().view(np.uint32)
    n, gn = min(total, cap), min(gtotal, gap_cap)
    assert (raw[7 * n:] == 0xFFFFFFFF).all() and (graw[5 * gn:] == 0xFFFFFFFF).all()  # nothing behind the records that were asked for
    assert (d_w.cpu().numpy().view(np.uint64) == packed).all()                           # the input is read-only: a call corrects a private copy
    return total, tuples(raw[:7 * n].view(fc.CALL_DTYPE)), gtotal, tuples(graw[:5 * gn].view(fm_dtype())), st


def fm_dtype():
    from mindthegap_amd import lib as L
    return L.MSNP_GAP_DTYPE


def check(idx, solid, k, seqs, m=M, packed=True):
    """the device against the model: calls, per-gap records and statistics, by the string entry, with a NULL gap output, and (for sequences
    without N) by the packed device entry; returns (calls, gap records, the model's scan)"""
    sc = fm.scan(solid, k, seqs, m, MAX_REPEAT)
    want, wrecs, wst = sc.calls, sc.gap_records, fm.stats_of(sc)
    calls, recs, st = idx.find_msnp_sequences(seqs, MAX_REPEAT, m)
    got, grecs = tuples(calls), tuples(recs)
    assert calls.dtype == fc.CALL_DTYPE
    diff = [i for i in range(min(len(got), len(want))) if got[i] != want[i]]
    assert not diff and len(got) == len(want), "%d calls, expected %d; first difference: %r, expected %r" % (
        len(got), len(want), got[diff[0]] if diff else got[len(want):][:1], want[diff[0]] if diff else want[len(got):][:1])
    assert grecs == wrecs
    assert {x: st[x] for x in fm.STAT_KEYS} == wst
    assert st["n_positions"] == sum(max(len(s) - k + 1, 0) for s in seqs)
    calls2, none, st2 = idx.find_msnp_sequences(seqs, MAX_REPEAT, m, gaps=False)
    assert none is None and tuples(calls2) == want and {x: st2[x] for x in fm.STAT_KEYS} == wst
    if packed:
        total, dev, gtotal, dgaps, std = packed_device(idx, seqs, m, len(want) + 2, len(wrecs) + 2)
        assert total == len(want) and dev == want and gtotal == len(wrecs) and dgaps == wrecs and {x: std[x] for x in fm.STAT_KEYS} == wst
    return got, grecs, sc


def snp_case(rng, k, start, offsets, tail=None, donors=1):
    """(sequence, its donors): substitutions at g0 + o for o in offsets, g0 = start + k - 1, so that with offsets no more than k apart there
    is one gap from `start` of k + max(offsets) positions; the sequence ends tail nucleotides behind the gap's last position (default:
    k + 1 + something, the least is k + 1: two anchors and no more)"""
    g0 = start + k - 1
    length = start + k + max(offsets) + (k + 1 if tail is None else tail)
    seq = fc.rand_seq(rng, length)
    out = []
    for _ in range(donors):
        d = list(seq)
        for o in offsets:
            d[g0 + o] = fs.other(rng, seq[g0 + o])
        out.append("".join(d))
    return seq, out


# ------------------------------------------------------------------------------------------------ 1. the reference's goldens
@pytest.fixture(scope="module")
def golden(mtg):
    solid = fc.solid_of_files(FASTQ_PAIR, K, CUTOFF)
    ref = pc.read_fasta(REFERENCE)
    names, seqs = [n for n, _ in ref], [s for _, s in ref]
    idx = mtg.Index.from_reads(FASTQ_PAIR, K, CUTOFF)
    yield idx, solid, names, seqs
    idx.close()


def test_golden_calls_by_both_entries(mtg, golden):
    idx, solid, names, seqs = golden
    got, recs, sc = check(idx, solid, K, seqs)
    assert [(names[c[0]], c[1] + 1, chr(c[6] >> 8), chr(c[6] & 255)) for c in got] == GOLDEN_CALLS and all(c[2] == 6 and c[3] == 0 for c in got)
    assert [(names[r[0]],) + r[1:] for r in recs] == [("Seq0", 267, 144, 0, 0), ("Seq1", 175, 44, 44, 2), ("Seq1", 712, 136, 0, 0), ("Seq2", 289, 55, 55, 2),
                                                      ("Seq3", 735, 46, 16, 1), ("Seq4", 791, 50, 0, 0), ("Seq4", 856, 72, 0, 0)]
    assert fm.stats_of(sc) == {"n_gaps": 35, "n_candidates": 7, "n_calls": 5, "n_full": 2, "n_partial": 1, "n_long": 0}
    for cap in (7, 5, 3, 1, 0):   # cap below the number of calls: the count is the total, the leading records are the same
        calls, r2, st = idx.find_msnp_sequences(seqs, MAX_REPEAT, M, cap=cap)
        assert st["n_calls"] == 5 and tuples(calls) == got[:cap] and tuples(r2) == recs
        total, dev, gtotal, dgaps, std = packed_device(idx, seqs, M, cap, 3)
        assert total == 5 and dev == got[:cap] and gtotal == 7 and dgaps == recs[:3]
    for bad in (0, K + 1, -3):
        with pytest.raises(mtg.MtgError):
            idx.find_msnp_sequences(seqs, MAX_REPEAT, bad)
    with pytest.raises(mtg.MtgError):
        idx.find_msnp_sequences(seqs, -1, M)
    assert tuples(idx.find_msnp_sequences(seqs, 0, M)[0]) == got == tuples(idx.find_msnp_sequences(seqs, 1000, M)[0])   # max_repeat plays no part
    calls, r0, st0 = idx.find_msnp_sequences([])  # nseq = 0
    assert len(calls) == 0 and len(r0) == 0 and all(st0[x] == 0 for x in fm.STAT_KEYS) and st0["n_positions"] == 0
    check(idx, solid, K, seqs, m=1)
    check(idx, solid, K, seqs, m=K)


# ------------------------------------------------------------------------------------------------ 2. two SNPs d apart, the smallest candidate
@pytest.mark.parametrize("k", [31, 13, 11])
def test_two_snps_at_every_distance(mtg, k):
    """per d = 1 .. k + 1 a sequence with two SNPs d apart (a gap of k + d: no candidate up to d = m, the smallest candidate at d = m + 1)
    and one with a third SNP 9 behind the second (a gap of k + d + 9: for d < m the first SNP's best count d is below m and nothing is called).
    The starts run through the word alignments"""
    rng = np.random.default_rng(9100 + k)
    seqs, solid, shape = [], set(), []
    for d in range(1, k + 2):
        for third in (False, True):
            start = 40 + 3 * d + int(third)
            seq, donors = snp_case(rng, k, start, [0, d] + ([d + 9] if third else []), tail=k + 1 + int(rng.integers(0, 30)))
            seqs.append(seq)
            solid |= fc.solid_of_strings(donors, k)
            shape.append((start, d, third))
    idx = index_of(mtg, solid, k)
    try:
        got, recs, sc = check(idx, solid, k, seqs)
        if k == 31:   # chance plays no part: what the rule says, stated apart from the model
            by_seq = {s: [c for c in got if c[0] == s] for s in range(len(seqs))}
            rec_of = {r[0]: r for r in recs}
            for s, (start, d, third) in enumerate(shape):
                g0, L = start + k - 1, k + d + (9 if third else 0)
                if L <= k + M:
                    assert s not in rec_of and by_seq[s] == []
                elif d < M:
                    assert rec_of[s] == (s, start, L, 0, 0) and by_seq[s] == []
                elif d == k + 1:   # a step advances k at the most: the second step looks at g0 + k, which is no SNP, and the chain ends in part
                    assert rec_of[s] == (s, start, L, k, 1) and [c[1] for c in by_seq[s]] == [g0]
                else:
                    pos = [g0, g0 + d] + ([g0 + d + 9] if third else [])
                    assert [c[1] for c in by_seq[s]] == pos and rec_of[s] == (s, start, L, L, len(pos))
                    assert all(c[4] == start - 1 and c[5] == start + L for c in by_seq[s])
            assert (k + M + 1) in {r[2] for r in recs} and (k + M) not in {r[2] for r in recs}
        check(idx, solid, k, seqs, m=2)
        check(idx, solid, k, seqs, m=1)
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 3. chains, alignments, the 256-slot boundary
@pytest.mark.parametrize("k", [31, 11])
def test_chains_alignments_and_the_longest_gaps(mtg, k):
    """chains of 3 .. 8 SNPs m .. k apart; gaps of 254 (judged: a text of 9 or, from start % 32 = 31, 10 words), 255 and 256 positions
    (counted, no call) at start % 32 = 0, 1 and 31; every sequence ends k + 1 nucleotides behind its gap, so the gap's text ends in the
    sequence's last word but one or last word and no word behind the sequence may be read"""
    rng = np.random.default_rng(9200 + k)
    seqs, solid, long_gaps = [], set(), []
    for n in range(3, 9):
        for rep in range(2):
            step_hi = min(k, (fm.MAX_GAP - k) // (n - 1))
            offs = np.concatenate([[0], np.cumsum(rng.integers(M, step_hi + 1, n - 1))]).tolist()
            seq, donors = snp_case(rng, k, 33 + 7 * n + rep, offs)
            seqs.append(seq)
            solid |= fc.solid_of_strings(donors, k)
    for align in (0, 1, 31):
        for L in (254, 255, 256):
            start = 64 + align
            seq, donor_set, n_snps = fm.long_gap_case(rng, k, start, L, step_lo=max(M, k - 6))
            long_gaps.append((len(seqs), start, L, n_snps))
            seqs.append(seq)
            solid |= donor_set
    idx = index_of(mtg, solid, k)
    try:
        got, recs, sc = check(idx, solid, k, seqs)
        st = fm.stats_of(sc)
        rec_of = {r[0]: r for r in recs}
        if k == 31:
            assert sorted(r[4] for r in recs[:12]) == sorted(2 * list(range(3, 9))) and all(r[3] == r[2] for r in recs[:12])
            for s, start, L, n in long_gaps:
                assert rec_of[s] == ((s, start, L, L, n) if L == 254 else (s, start, L, 0, 0))
            assert st["n_long"] == 6 and st["n_full"] == 15 and st["n_partial"] == 0
        assert st["n_long"] >= 4 and any(r[2] == 254 and r[3] for r in recs) and sc.seen["gaps_with_several"] >= 12
        n = len(got)
        for cap in (0, 1, n - 1):
            calls, r2, stc = idx.find_msnp_sequences(seqs, MAX_REPEAT, M, cap=cap)
            assert stc["n_calls"] == n and tuples(calls) == got[:cap] and tuples(r2) == recs
        check(idx, solid, k, seqs, m=3)
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 4. competing alternatives, the beyond-the-gap stop
def competing_cases(k):
    """the competing donors of tests/find_msnp_cases.py, 24 sequences against the union of their sets: alternatives tie below k, two reach
    k, and a chain ends at a call that would go beyond the gap"""
    cases = fm.competing_cases(k, 9300 + 10 * k + 1, 24)
    return [c[0] for c in cases], set().union(*[c[1] for c in cases])


@pytest.mark.parametrize("k", [13, 11])
def test_competing_alternatives_and_the_stop_beyond_the_gap(mtg, k):
    seqs, solid = competing_cases(k)
    idx = index_of(mtg, solid, k)
    try:
        for m in (1, 2, 5):
            got, recs, sc = check(idx, solid, k, seqs, m=m)
            if m == 1:   # the model alone says that the cases are there
                assert sc.seen["tie_below_k"] >= 3 and sc.seen["two_reach_k"] >= 3 and sc.seen["beyond_stop"] >= 1 and sc.seen["reads_substitution"] >= 10, sc.seen
                assert fm.stats_of(sc)["n_partial"] >= 3 and fm.stats_of(sc)["n_full"] >= 3
                wrong = [fm.find_by_closed_form(solid, k, seqs, m, **w)[0] for w in ({"first_at_tie": True}, {"no_correction": True}, {"order": "ACGT"}, {"no_beyond_stop": True})]
                assert all(w != got for w in wrong)   # a device that did any of these would fail here
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 5. several sequences, N, lower case
def test_several_sequences_with_n_and_lower_case(mtg):
    rng = np.random.default_rng(9400)
    k = K
    seq, donors = snp_case(rng, k, 70, [0, 13, 30], tail=90)
    solid = fc.solid_of_strings(donors, k)
    g0 = 70 + k - 1
    put = lambda t, i, ch="N": t[:i] + ch + t[i + 1:]  # noqa: E731
    s = {"plain": seq, "lower_all": seq.lower(), "lower_snps": put(put(seq, g0, seq[g0].lower()), g0 + 13, seq[g0 + 13].lower()),
         "n_before": put(seq, 70 - 2), "n_further_before": put(seq, 70 - 3), "n_in_gap": put(seq, g0 + 5), "n_behind": put(seq, g0 + 30 + k + 20, "n"),
         "short": seq[:k - 1], "empty": "", "end_one_solid": seq[:70 + k + 30 + k], "end_two_solid": seq[:70 + k + 30 + k + 1], "starts_in_gap": seq[72:]}
    tags = list(s)
    seqs = [s[t] for t in tags]
    idx = index_of(mtg, solid, k)
    try:
        got, recs, sc = check(idx, solid, k, seqs, packed=False)   # N is not part of the packed alphabet
        of = lambda tag: [c[1:] for c in got if c[0] == tags.index(tag)]  # noqa: E731
        full = of("plain")
        assert [c[0] for c in full] == [g0, g0 + 13, g0 + 30] and all(c[1:5] == (6, 0, 69, 70 + k + 30) for c in full)
        assert all(chr(c[5] >> 8) == seq[c[0]] and chr(c[5] & 255) == donors[0][c[0]] for c in full)   # upper case whatever the text's case
        for tag in ("lower_all", "lower_snps", "n_further_before", "n_behind", "end_two_solid"):
            assert of(tag) == full, tag
        for tag in ("n_before", "n_in_gap", "short", "empty", "end_one_solid", "starts_in_gap"):
            assert of(tag) == [], tag
        check(idx, solid, k, [x for x in seqs if "N" not in x.upper()])
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 6. the other entries, the tool
def test_the_other_find_entries_are_unchanged_by_a_multi_run(mtg, golden):
    idx, solid, names, seqs = golden

    def others():
        return [tuples(idx.find_homo_sequences(seqs, MAX_REPEAT)[0]), tuples(idx.find_del_sequences(seqs, MAX_REPEAT)[0]), tuples(idx.find_snp_sequences(seqs, MAX_REPEAT)[0]),
                tuples(idx.find_het_sequences(seqs, None, MAX_REPEAT, BRANCHING)[0])]
    before = others()
    multi = tuples(idx.find_msnp_sequences(seqs, MAX_REPEAT, M)[0])
    packed_device(idx, seqs, M, 8, 8)   # asserts that the device input is unmodified
    assert others() == before
    assert before[0] == fc.find_homo(solid, K, seqs, MAX_REPEAT)[0] and before[1] == fd.find_del(solid, K, seqs, MAX_REPEAT)[0]
    assert before[2] == fs.find_snp(solid, K, seqs, MAX_REPEAT)[0] and before[3] == fh.find_het(solid, K, seqs, None, MAX_REPEAT, BRANCHING)[0]
    assert not {(c[0], c[1]) for c in multi} & {(c[0], c[1]) for c in before[2]} and len(multi) == 5


@pytest.mark.parametrize("flags", [["-multi-snps"], ["-solo-snps", "-multi-snps"], ["-multi-snps", "-snp-min-val", "3"]])
def test_find_tool_on_the_golden(mtg, golden, tmp_path, flags):
    idx, solid, names, seqs = golden
    m = 3 if "-snp-min-val" in flags else M
    config = "-solo-snps -multi-snps" if "-solo-snps" in flags else "-multi-snps"
    family = fm.scan(solid, K, seqs, m, MAX_REPEAT, config).calls   # one literal scan with both observers
    multi = fm.find_msnp(solid, K, seqs, m)[0]
    solo = fs.find_snp(solid, K, seqs, MAX_REPEAT)[0] if "-solo-snps" in flags else []
    assert family == fm.merge(solo, multi) and len(family) == len(solo) + len(multi)
    got_bk, got_vcf, stdout = run_tool(mtg, ["-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-abundance-min", str(CUTOFF)] + flags, str(tmp_path / "found"))
    assert got_bk == [] and got_vcf == fm.lines(family, names)
    assert ("SNPs                                     : %d" % len(family)) in stdout and "deletion                                 : no" in stdout
    assert ("snp                                      : " + ("isolated and close (forward)" if solo else "close only (forward)")) in stdout
    if m == M:
        gold = [l.split("\t") for l in open(os.path.join(GOLDEN, "full_test", "gold.othervariants.snp.vcf")).read().splitlines()]
        mine = [l.split("\t") for l in got_vcf]
        in_gold = [x for x in mine if any(g[:2] + g[3:] == x[:2] + x[3:] for g in gold)]
        assert len(mine) == len(solo) + 5 and len(in_gold) == len(solo) + 3   # Seq1/206 and Seq1/219 are not in gold: its graph differed there
        assert [x[:2] for x in mine if x not in in_gold] == [["Seq1", "206"], ["Seq1", "219"]]
    assert sorted(os.listdir(str(tmp_path))) == ["found.breakpoints", "found.othervariants.vcf"]
