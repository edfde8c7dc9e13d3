"""`find` for close homozygous SNPs with the reverse pass on the device (k_msnp_rev_judge, k_msnp_rev_emit, k_msnp_rev_gaps and
k_gap_mark<MultiRevObserver> in csrc/mtg_gpu_misc.hip behind mtg_index_find_msnp_rev_sequences / _packed_device and
`MindTheGap find [-solo-snps] [-multi-snps] -rev-snps`) against the plain model of tests/find_msnp_rev_cases.py: the literal
FindMultiSNPrev::update with the literal snp_at_begin behind the literal forward observer on a ring of 256 slots, the ring indices restored
after a gap and gaps of 255 positions and more not judged (the two documented deviations).  Every comparison is exact -- calls, per-gap
records and statistics -- through both entries.

A MEET CASE (meet_case) is the smallest text in which the left anchor's window decides.  Two donors A and B of a sequence, subs at
z < q < p < p + a < w with z = p - k, p - q >= m, a < m, m < w - p, w - q <= k: A has q (alpha), p, p + a, w; B has z, q (beta), w.  The gap is
[q - k + 1, w].  The forward pass calls alpha at q and stops at p (its next window holds p + a uncorrected: a < m).  The reverse pass calls w
along B, lands on q, and there B's beta holds for the k - (p - q) windows down to the residual gap's first k-mer; the next window is the k-mer
at p - k = start' - 1, the anchor: with z in B it fails and the passes meet exactly; with z - 1 in its place (with_z = False: the forward pass still
prefers alpha, its first window holds z - 1) the anchor's k-mer does not reach it, holds, and the chain stops without a call."""
import os

import numpy as np
import pytest

from tests import find_cases as fc
from tests import find_msnp_cases as fm
from tests import find_msnp_rev_cases as fr
from tests import find_snp_cases as fs
from tests import profile_cases as pc
from tests.test_gpu_find_snp import index_of, pack, run_tool, tuples

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FASTQ_PAIR = [os.path.join(GOLDEN, "data", "reads_r1.fastq"), os.path.join(GOLDEN, "data", "reads_r2.fastq")]
REFERENCE = os.path.join(GOLDEN, "full_test", "reference.fasta")
K, CUTOFF, MAX_REPEAT, M = 31, 7, 5, 5
SEEDS = {11: 9711, 13: 9713, 31: 9731}


@pytest.fixture(scope="module")
def mtg():
    import torch
    torch.cuda.init()  # torch bundles its own HIP runtime: initialise it before libmtgfill.so touches the device
    import mindthegap_amd
    mindthegap_amd.load_library()
    assert mindthegap_amd.device_count() >= 1, "these tests need a HIP device"
    return mindthegap_amd


def rev_dtype():
    from mindthegap_amd import lib as L
    return L.MSNP_REV_GAP_DTYPE


def packed_device(idx, seqs, m, passes, cap, gap_cap):
    """(total calls, calls, total gaps, gap records, stats) of the packed device entry; the input words are checked to be unchanged"""
    import torch
    packed, word_off, lens = pack(seqs)
    dev = torch.device("cuda", 0)
    d_w = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_wo = torch.from_numpy(word_off.view(np.int64)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_calls = torch.full((max(cap, 1) * 7 + 7,), -1, dtype=torch.int32, device=dev)
    d_gaps = torch.full((max(gap_cap, 1) * 7 + 7,), -1, dtype=torch.int32, device=dev)
    total, gtotal, st = idx.find_msnp_rev_packed_device(d_w.data_ptr(), d_wo.data_ptr(), d_ln.data_ptr(), len(seqs), MAX_REPEAT, m, passes, d_calls.data_ptr() if cap else None, cap,
                                                        d_gaps.data_ptr() if gap_cap else None, gap_cap)
    torch.cuda.synchronize()
    raw, graw = d_calls.cpu().numpy().view(np.uint32), d_gaps.cpu().numpy().view(np.uint32)
    n, gn = min(total, cap), min(gtotal, gap_cap)
    assert (raw[7 * n:] == 0xFFFFFFFF).all() and (graw[7 * gn:] == 0xFFFFFFFF).all()  # nothing behind the records that were asked for
    assert (d_w.cpu().numpy().view(np.uint64) == packed).all()                           # the input is read-only: a call corrects a private copy
    return total, tuples(raw[:7 * n].view(fc.CALL_DTYPE)), gtotal, tuples(graw[:7 * gn].view(rev_dtype())), st


def check(idx, solid, k, seqs, m=M, passes=3, packed=True):
    """the device against the restored literal model: calls, per-gap records and statistics, by the string entry, with a NULL gap output, and
    by the packed device entry; returns (calls, gap records, the model's scan)"""
    sc = fr.scan(solid, k, seqs, m, passes, MAX_REPEAT)
    want, wrecs, wst = sc.calls, sc.gap_records, fr.stats_of(sc)
    calls, recs, st = idx.find_msnp_rev_sequences(seqs, MAX_REPEAT, m, passes)
    got, grecs = tuples(calls), tuples(recs)
    assert calls.dtype == fc.CALL_DTYPE and recs.dtype == rev_dtype()
    diff = [i for i in range(min(len(got), len(want))) if got[i] != want[i]]
    assert not diff and len(got) == len(want), "passes %d: %d calls, expected %d; first difference: %r, expected %r" % (
        passes, len(got), len(want), got[diff[0]] if diff else got[len(want):][:1], want[diff[0]] if diff else want[len(got):][:1])
    assert grecs == wrecs
    assert {x: st[x] for x in fr.STAT_KEYS} == wst
    assert st["n_positions"] == sum(max(len(s) - k + 1, 0) for s in seqs)
    calls2, none, st2 = idx.find_msnp_rev_sequences(seqs, MAX_REPEAT, m, passes, gaps=False)
    assert none is None and tuples(calls2) == want and {x: st2[x] for x in fr.STAT_KEYS} == wst
    if packed:
        total, dev, gtotal, dgaps, std = packed_device(idx, seqs, m, passes, len(want) + 2, len(wrecs) + 2)
        assert total == len(want) and dev == want and gtotal == len(wrecs) and dgaps == wrecs and {x: std[x] for x in fr.STAT_KEYS} == wst
    return got, grecs, sc


def meet_case(rng, k, m, start, with_z=True):
    """(sequence, [donor A, donor B], (q, p, a, w)) of the module's docstring with the gap's first position at `start`"""
    delta = int(rng.integers(m, k - m))                          # p - q = m .. k - m - 1; k - delta > m windows for the reverse call at q
    a = int(rng.integers(1, m))                                  # 1 .. m - 1
    q = start + k - 1
    p = q + delta
    w = q + int(rng.integers(max(delta + m + 1, delta + a + 1), k + 1))
    z = p - k
    seq = fc.rand_seq(rng, w + k + 2 + int(rng.integers(0, 20)))
    alpha = fs.other(rng, seq[q])
    beta = [x for x in "ACGT" if x not in (seq[q], alpha)][int(rng.integers(2))]
    omega = fs.other(rng, seq[w])
    A, B = list(seq), list(seq)
    A[q], A[p], A[p + a], A[w] = alpha, fs.other(rng, seq[p]), fs.other(rng, seq[p + a]), omega
    B[q], B[w] = beta, omega
    zz = z if with_z else z - 1
    B[zz] = fs.other(rng, seq[zz])
    return seq, ["".join(A), "".join(B)], (q, p, a, w)


def competing_set(k, seed):
    """about 100 short sequences and the union of their donors' k-mers: 56 of tests/find_msnp_cases.py's competing donors, 24 meet cases and
    20 meet cases with z - 1 in place of z"""
    rng = np.random.default_rng(seed)
    cases = fm.competing_cases(k, seed, 56)
    seqs, solid = [c[0] for c in cases], set().union(*[c[1] for c in cases])
    for i in range(44):
        seq, donors, _ = meet_case(rng, k, M, 34 + int(rng.integers(0, 64)), with_z=i < 24)
        seqs.append(seq)
        solid |= fc.solid_of_strings(donors, k)
    return seqs, solid


# ------------------------------------------------------------------------------------------------ 1. competing donors, the three passes
@pytest.mark.parametrize("k", [31, 13, 11])
def test_competing_donors_by_the_three_passes(mtg, k):
    seqs, solid = competing_set(k, SEEDS[k])
    idx = index_of(mtg, solid, k)
    try:
        seen = {}
        for passes in (1, 2, 3):
            got, recs, sc = check(idx, solid, k, seqs, passes=passes)
            seen[passes] = sc.rev_seen
        # the model alone says that the cases are there
        assert seen[2]["full_take"] >= 10 and seen[2]["anchor_stop"] >= 10, seen[2]
        assert seen[3]["partial_fwd_then_rev_call"] >= 10 and seen[3]["meet_exactly"] >= 10 and seen[3]["anchor_stop"] >= 10, seen[3]
        # passes = 1 is the existing entry on the same input, bit for bit
        calls, recs, st = idx.find_msnp_sequences(seqs, MAX_REPEAT, M)
        calls1, recs1, st1 = idx.find_msnp_rev_sequences(seqs, MAX_REPEAT, M, 1)
        assert calls1.tobytes() == calls.tobytes() and [r[:5] for r in tuples(recs1)] == tuples(recs) and all(r[5:] == (0, 0) for r in tuples(recs1))
        assert {x: st1[x] for x in st if x != "kernel_ms"} == {x: st[x] for x in st if x != "kernel_ms"}
        check(idx, solid, k, seqs, m=1, passes=3)
        check(idx, solid, k, seqs, m=2, passes=2, packed=False)
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 2. the anchor window at every alignment
@pytest.mark.parametrize("k", [31, 11])
def test_the_anchor_window_decides_at_every_alignment(mtg, k):
    """per start % 32 = 0 .. 31 a meet case with z (the anchor's window fails: the gap is taken whole) and one with z - 1 in its place (it holds: the
    chain stops).  With start % 32 == 0 the nucleotide start - 1 of the anchor lies in a word the forward text never holds"""
    rng = np.random.default_rng(9800 + k)
    seqs, solid, shape = [], set(), []
    for align in range(32):
        for with_z in (True, False):
            start = 32 * (2 + align % 3) + align
            seq, donors, where = meet_case(rng, k, M, start, with_z)
            seqs.append(seq)
            solid |= fc.solid_of_strings(donors, k)
            shape.append((start, with_z) + where)
    idx = index_of(mtg, solid, k)
    try:
        got, recs, sc = check(idx, solid, k, seqs, passes=3)
        got2, recs2, sc2 = check(idx, solid, k, seqs, passes=2)
        if k == 31:   # chance plays no part: what the rule says, stated apart from the model
            rec_of = {r[0]: r for r in recs}
            for s, (start, with_z, q, p, a, w) in enumerate(shape):
                L, mine = w - start + 1, [c for c in got if c[0] == s]
                assert mine[0][1:6] == (q, 6, 0, start - 1, start + L)
                if with_z:
                    assert rec_of[s] == (s, start, L, p - q, 1, L - (p - q), 2) and [c[1:6] for c in mine[1:]] == [(w, 7, 0, p - k, start + L), (q, 7, 0, p - k, start + L)]
                    assert chr(mine[2][6] >> 8) == chr(mine[0][6] & 255)   # the reverse call's REF is the forward call's ALT: it read the corrected text
                else:
                    assert rec_of[s] == (s, start, L, p - q, 1, w - q, 1) and [c[1:6] for c in mine[1:]] == [(w, 7, 0, p - k, start + L)]
            assert sc.rev_seen["meet_exactly"] == 32 and sc.rev_seen["anchor_stop"] == 32
        assert {r[1] % 32 for r in recs if r[6]} == set(range(32))
        # the reverse pass alone ends every one of these gaps at the k-mer at start - 1, which holds: the anchor of the whole gap
        assert sc2.rev_seen["anchor_stop"] >= (64 if k == 31 else 32) and {r[1] % 32 for r in recs2 if 0 < r[5] < r[2]} == set(range(32))
        # a device that wrote ascending or skipped the forward substitutions would fail here; one that kept the forward text, where the
        # residual gap is the whole gap and its anchor is the nucleotide start - 1: under passes 2
        for wrong in ({"ascending": True}, {"no_forward_subst": True}):
            assert fr.find_by_closed_form(solid, k, seqs, M, 3, **wrong) != (sc.calls, sc.gap_records), wrong
        kept = fr.find_by_closed_form(solid, k, seqs, M, 2, forward_text=True)[1]
        told_apart = {r[1] % 32 for r, w in zip(recs2, kept) if tuple(r) != w}
        assert 0 in told_apart and len(told_apart) >= (32 if k == 31 else 28)   # (at k = 11 a chance k-mer decides a case or two: the model says which)
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 3. the longest gaps
@pytest.mark.parametrize("k", [31, 11])
def test_gaps_of_250_to_256_at_several_alignments(mtg, k):
    """gaps of 250 .. 254 positions (judged; from start % 32 = 0, 8, 20 and 31 a text of 10 words), 255 and 256 (counted in n_long by either
    pass, no call); every sequence ends k + 1 nucleotides behind its gap, so no word behind the sequence may be read"""
    rng = np.random.default_rng(9900 + k)
    seqs, solid, long_gaps = [], set(), []
    for align in (0, 1, 8, 20, 31):
        for L in (250, 251, 252, 253, 254, 255, 256):
            start = 64 + align
            seq, donor_set, n_snps = fm.long_gap_case(rng, k, start, L, step_lo=max(M, k - 6))
            long_gaps.append((len(seqs), start, L, n_snps))
            seqs.append(seq)
            solid |= donor_set
    idx = index_of(mtg, solid, k)
    try:
        for passes in (2, 3, 1):
            got, recs, sc = check(idx, solid, k, seqs, passes=passes)
            st = fr.stats_of(sc)
            if k == 31:
                rec_of = {r[0]: r for r in recs}
                for s, start, L, n in long_gaps:
                    want = (0, 0, 0, 0) if L > 254 else (0, 0, L, n) if passes == 2 else (L, n, 0, 0)
                    assert rec_of[s] == (s, start, L) + want
                assert st["n_long"] == 10 and st["n_full"] == 25 and st["n_partial"] == 0
            assert st["n_long"] >= 5   # (at k = 11 chance k-mers split some of the ten long gaps: the model decides)
        from mindthegap_amd import lib as L_
        assert L_.MSNP_REV_GAP_DTYPE.itemsize == 28
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 4. the reference's goldens, capacities
@pytest.fixture(scope="module")
def golden(mtg):
    solid = fc.solid_of_files(FASTQ_PAIR, K, CUTOFF)
    ref = pc.read_fasta(REFERENCE)
    names, seqs = [n for n, _ in ref], [s for _, s in ref]
    idx = mtg.Index.from_reads(FASTQ_PAIR, K, CUTOFF)
    yield idx, solid, names, seqs
    idx.close()


def named(calls, names):
    return [(names[c[0]], c[1] + 1, chr(c[6] >> 8), chr(c[6] & 255)) for c in calls]


def test_golden_calls_by_both_entries_and_capacities(mtg, golden):
    idx, solid, names, seqs = golden
    got, recs, sc = check(idx, solid, K, seqs, passes=3)
    assert fr.stats_of(sc) == {"n_gaps": 35, "n_candidates": 7, "n_calls": 6, "n_full": 2, "n_partial": 2, "n_long": 0}
    assert tuples(idx.find_msnp_sequences(seqs, MAX_REPEAT, M)[0]) == [c for c in got if c[2] == 6] and sum(1 for c in got if c[2] == 6) == 5
    rev = [c for c in got if c[2] == 7]
    assert named(rev, names) == [("Seq4", 841, "C", "T")] and rev[0][3:6] == (0, 790, 841)
    by = {(names[r[0]], r[1]): r[2:] for r in recs}
    assert by[("Seq4", 791)] == (50, 0, 0, 20, 1) and by[("Seq3", 735)] == (46, 16, 1, 0, 0)
    got2, recs2, sc2 = check(idx, solid, K, seqs, passes=2)
    assert named(got2, names) == [("Seq1", 219, "T", "A"), ("Seq1", 206, "G", "C"), ("Seq2", 344, "C", "A"), ("Seq2", 320, "T", "C"), ("Seq4", 841, "C", "T")]
    by2 = {(names[r[0]], r[1]): r[2:] for r in recs2}
    assert by2[("Seq1", 175)] == (44, 0, 0, 44, 2) and by2[("Seq2", 289)] == (55, 0, 0, 55, 2)
    check(idx, solid, K, seqs, passes=1)
    # capacities 0, 1, n, n + 2 and NULL for calls and gap records: the counts are the totals, the leading records are the same
    n, g = len(got), len(recs)
    for cap in (0, 1, n, n + 2):
        calls, r2, st = idx.find_msnp_rev_sequences(seqs, MAX_REPEAT, M, 3, cap=cap)
        assert st["n_calls"] == n and tuples(calls) == got[:cap] and tuples(r2) == recs
        for gap_cap in (0, 1, g, g + 2):
            total, dev, gtotal, dgaps, std = packed_device(idx, seqs, M, 3, cap, gap_cap)
            assert total == n and dev == got[:cap] and gtotal == g and dgaps == recs[:gap_cap] and std["n_calls"] == n
    for bad in (0, 4, -1):
        with pytest.raises(mtg.MtgError):
            idx.find_msnp_rev_sequences(seqs, MAX_REPEAT, M, bad)
    for bad in (0, K + 1):
        with pytest.raises(mtg.MtgError):
            idx.find_msnp_rev_sequences(seqs, MAX_REPEAT, bad, 3)
    calls, r0, st0 = idx.find_msnp_rev_sequences([], MAX_REPEAT, M, 3)  # nseq = 0
    assert len(calls) == 0 and len(r0) == 0 and all(st0[x] == 0 for x in fr.STAT_KEYS)


# ------------------------------------------------------------------------------------------------ 5. the tool
@pytest.mark.parametrize("flags", [["-rev-snps"], ["-multi-snps", "-rev-snps"], ["-solo-snps", "-multi-snps", "-rev-snps"]])
def test_find_tool_on_the_golden(mtg, golden, tmp_path, flags):
    idx, solid, names, seqs = golden
    passes = 3 if "-multi-snps" in flags else 2
    with_solo = "-solo-snps" in flags
    family = fr.scan(solid, K, seqs, M, passes, MAX_REPEAT, solo=with_solo).calls   # one literal scan with all observers of the configuration
    multi = fr.find_msnp_rev(solid, K, seqs, M, passes)[0]
    solo = fs.find_snp(solid, K, seqs, MAX_REPEAT)[0] if with_solo else []
    assert family == fr.merge(solo, multi) and len(family) == len(solo) + len(multi)
    got_bk, got_vcf, stdout = run_tool(mtg, ["-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-abundance-min", str(CUTOFF)] + flags, str(tmp_path / "found"))
    assert got_bk == [] and got_vcf == fr.lines(family, names)
    assert ("SNPs                                     : %d" % len(family)) in stdout and "deletion                                 : no" in stdout
    what = "forward, then reverse" if passes == 3 else "reverse"
    assert ("snp                                      : " + ("isolated and close (%s)" if with_solo else "close only (%s)") % what) in stdout
    if with_solo:
        gold = [l.split("\t") for l in open(os.path.join(GOLDEN, "full_test", "gold.othervariants.snp.vcf")).read().splitlines() if not l.startswith("#")]
        mine = [l.split("\t") for l in got_vcf]
        in_gold = [x for x in mine if any(g_[:2] + g_[3:] == x[:2] + x[3:] for g_ in gold)]
        assert len(mine) == 13 and len(gold) == 11 and [x[:2] + x[3:] for x in in_gold] == [g_[:2] + g_[3:] for g_ in gold]   # all eleven, in gold's order
    assert sorted(os.listdir(str(tmp_path))) == ["found.breakpoints", "found.othervariants.vcf"]
