"""`find` for homozygous insertions on the device (k_profile_count<true> / k_profile_write<true>, k_find_mark, k_mark_*, k_find_assemble,
k_find_emit in csrc/mtg_gpu_misc.hip behind mtg_index_find_homo_sequences / _packed_device and `MindTheGap find -homo-insertions`) against
the plain model of tests/find_cases.py: the literal loop of the reference's notify() and its four observers.  Every comparison is exact.

The synthetic cases index every k-mer of a donor text; the reference handed to `find` is the donor with stretches cut out (the donor's
insertions), with k-mers added to or taken from the index where a case needs an isolated solid k-mer or a missing window."""
import os
import subprocess

import numpy as np
import pytest

from tests import find_cases as fc
from tests import profile_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FASTQ_PAIR = [os.path.join(GOLDEN, "data", "reads_r1.fastq"), os.path.join(GOLDEN, "data", "reads_r2.fastq")]
REFERENCE = os.path.join(GOLDEN, "full_test", "reference.fasta")
K, CUTOFF, MAX_REPEAT = 31, 7, 5
STAT_KEYS = ("n_gaps", "n_candidates", "n_homo_clean", "n_homo_fuzzy", "n_small_clean", "n_small_fuzzy")


@pytest.fixture(scope="module")
def mtg():
    import torch
    torch.cuda.init()  # torch bundles its own HIP runtime: initialise it before libmtgfill.so touches the device
    import mindthegap_amd
    mindthegap_amd.load_library()
    assert mindthegap_amd.device_count() >= 1, "these tests need a HIP device"
    return mindthegap_amd


@pytest.fixture(scope="module")
def golden(mtg):
    solid = fc.solid_of_files(FASTQ_PAIR, K, CUTOFF)
    ref = pc.read_fasta(REFERENCE)
    names, seqs = [n for n, _ in ref], [s for _, s in ref]
    want, wst = fc.find_homo(solid, K, seqs, MAX_REPEAT)
    assert len(want) == 13  # tests/test_find_cpu.py holds the list itself
    idx = mtg.Index.from_reads(FASTQ_PAIR, K, CUTOFF)
    yield idx, names, seqs, want, wst
    idx.close()


def index_of(mtg, solid, k):
    kms = np.array(sorted(solid), dtype=np.uint64)
    return mtg.Index.from_kmers(kms, np.full(len(kms), 9, dtype=np.uint32), k)


def check(idx, solid, k, seqs, max_repeat):
    """find on the device against the model: calls and statistics; returns (calls as tuples, statistics of the model)"""
    calls, st = idx.find_homo_sequences(seqs, max_repeat)
    want, wst = fc.find_homo(solid, k, seqs, max_repeat)
    got = [tuple(int(x) for x in c) for c in calls]
    assert calls.dtype == fc.CALL_DTYPE
    diff = [i for i in range(min(len(got), len(want))) if got[i] != want[i]]
    assert not diff and len(got) == len(want), "%d calls, expected %d; first difference: %r, expected %r" % (
        len(got), len(want), got[diff[0]] if diff else got[len(want):][:1], want[diff[0]] if diff else want[len(got):][:1])
    assert {x: st[x] for x in STAT_KEYS} == wst and st["n_calls"] == len(want)
    assert st["n_positions"] == sum(max(len(s) - k + 1, 0) for s in seqs)
    return got, wst


def pack(seqs, k):
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


def packed_device_calls(idx, seqs, k, max_repeat, cap):
    import torch
    packed, word_off, lens = pack(seqs, k)
    dev = torch.device("cuda", 0)
    d_w = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_wo = torch.from_numpy(word_off.view(np.int64)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_calls = torch.full((max(cap, 1) * 7 + 7,), -1, dtype=torch.int32, device=dev)
    total, st = idx.find_homo_packed_device(d_w.data_ptr(), d_wo.data_ptr(), d_ln.data_ptr(), len(seqs), max_repeat, d_calls.data_ptr() if cap else None, cap)
    torch.cuda.synchronize()
    raw = d_calls.cpu().numpy().view(np.uint32)
    n = min(total, cap)
    assert (raw[7 * n:] == 0xFFFFFFFF).all()  # nothing behind the calls that were asked for
    return total, [tuple(int(x) for x in c) for c in raw[:7 * n].view(fc.CALL_DTYPE)], st


# ------------------------------------------------------------------------------------------------ 1. the reference's goldens
def test_golden_calls_by_both_entries(mtg, golden):
    idx, names, seqs, want, wst = golden
    calls, st = idx.find_homo_sequences(seqs, MAX_REPEAT)
    assert [tuple(int(x) for x in c) for c in calls] == want
    assert {x: st[x] for x in STAT_KEYS} == wst and st["n_calls"] == 13
    for cap in (20, 13, 5, 0):
        total, got, st2 = packed_device_calls(idx, seqs, K, MAX_REPEAT, cap)
        assert total == 13 and got == want[:cap] and {x: st2[x] for x in STAT_KEYS} == wst
    with pytest.raises(mtg.MtgError):
        idx.find_homo_sequences(seqs, -1)
    big = [tuple(int(x) for x in c) for c in idx.find_homo_sequences(seqs, 1000)[0]]  # above k - 2: as k - 2
    assert big == fc.find_homo(fc.solid_of_files(FASTQ_PAIR, K, CUTOFF), K, seqs, 1000)[0] == [tuple(int(x) for x in c) for c in idx.find_homo_sequences(seqs, K - 2)[0]]


def test_find_tool_writes_the_reference_s_two_files(mtg, golden, tmp_path):
    idx, names, seqs, want, wst = golden
    exe = os.path.join(os.path.dirname(mtg.build_library()), "MindTheGap")
    out = str(tmp_path / "found")
    r = subprocess.run([exe, "find", "-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-homo-insertions", "-abundance-min", str(CUTOFF), "-out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    bk, vcf = fc.breakpoint_lines(want, names, seqs, K)
    assert open(out + ".breakpoints").read().splitlines() == bk
    lines = open(out + ".othervariants.vcf").read().splitlines()
    assert lines[0] == "##fileformat=VCFv4.1" and lines[1].startswith("##filedate=") and lines[2].startswith("##source=MindTheGap find version ")
    assert lines[3] == "##SAMPLE=file:" + ",".join(FASTQ_PAIR) and lines[4] == "##REF=file:" + REFERENCE
    assert lines[5:10] == ['##INFO=<ID=TYPE,Number=1,Type=String,Description="SNP, INS, DEL or .">', '##INFO=<ID=LEN,Number=1,Type=Integer,Description="variant size">',
                           '##INFO=<ID=FUZZY,Number=1,Type=Integer,Description="repeat size at the breakpoint, only for INS and DEL">',
                           '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tG1"]
    assert lines[10:] == vcf
    assert sorted(os.listdir(str(tmp_path))) == ["found.breakpoints", "found.othervariants.vcf"]
    assert "homozygous                               : 3" in r.stdout and "clean                                    : 1" in r.stdout
    assert "fuzzy                                    : 2" in r.stdout and "Homozygous insertions 1-2 bp size        : 10" in r.stdout
    # find -> fill: the three golden sites are filled with the golden's sequences (matched by position: the ids differ)
    fill = str(tmp_path / "filled")
    r = subprocess.run([exe, "fill", "-in", ",".join(FASTQ_PAIR), "-bkpt", out + ".breakpoints", "-abundance-min", str(CUTOFF), "-out", fill], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]

    def by_pos(path):
        d, lines = {}, open(path).read().splitlines()
        for i in range(0, len(lines) - 1, 2):
            f = lines[i][1:].split()[0].split("_")
            d.setdefault((f[1], int(f[3])), []).append(lines[i + 1])
        return d
    mine, gold = by_pos(fill + ".insertions.fasta"), by_pos(os.path.join(GOLDEN, "full_test", "gold.insertions.fasta"))
    for key in (("Seq2", 535), ("Seq2", 835), ("Seq4", 603)):
        assert mine[key] == gold[key], key


# ------------------------------------------------------------------------------------------------ 2. gap lengths
@pytest.mark.parametrize("k", [31, 21, 13])
def test_planted_insertions_of_every_length_and_repeat(mtg, k):
    """insertions of 1, 2, 3 and 50 nt with junction repeats of 0 .. 6 planted 700 nt apart in a random donor of 20 kb; max_repeat 0 and 5"""
    rng = np.random.default_rng(1000 + k)
    donor = fc.rand_seq(rng, 20000)
    sites = []
    for i, (n, r) in enumerate((n, r) for n in (1, 2, 3, 50) for r in range(0, MAX_REPEAT + 2)):
        a = 300 + 700 * i
        donor = fc.with_repeat(rng, donor, a, n, r)
        sites.append((a, n))
    ref = fc.planted(rng, donor, k, sites)
    solid = fc.solid_of_strings([donor], k)
    idx = index_of(mtg, solid, k)
    try:
        got5, st5 = check(idx, solid, k, [ref], 5)
        got0, st0 = check(idx, solid, k, [ref], 0)
        assert st5["n_gaps"] >= 28 and st5["n_small_clean"] + st5["n_small_fuzzy"] >= 10 and st5["n_homo_clean"] + st5["n_homo_fuzzy"] >= 8
        assert set(c[3] for c in got5) >= {0, 1, 2, 3, 4, 5} and set(c[3] for c in got0) == {0} and 0 < len(got0) < len(got5)
        n = len(got5)
        for cap in (0, 1, n - 1, n, n + 3):  # capacity: the count is the total, the leading records are the same
            calls, st = idx.find_homo_sequences([ref], 5, cap=cap)
            assert st["n_calls"] == n and [tuple(int(x) for x in c) for c in calls] == got5[:cap]
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 3. one index for the hand-built shapes
class Shapes:
    """a donor of 6 kb with insertions of 50 nt (clean, r = 0) every 500 nt; the reference is the donor without them"""

    def __init__(self, mtg, k, seed):
        rng = np.random.default_rng(seed)
        self.k, self.rng = k, rng
        donor = fc.rand_seq(rng, 6000)
        self.sites = [(300 + 500 * i, 50) for i in range(10)]
        for j, (a, n) in enumerate(self.sites):
            donor = fc.with_repeat(rng, donor, a, n, 3 if j == 6 else 0)
        self.donor = donor
        self.ref = fc.planted(rng, donor, k, self.sites)
        self.junction = [a - 50 * j for j, (a, n) in enumerate(self.sites)]  # first reference character behind the j-th insertion
        solid = fc.solid_of_strings([donor], k)
        ref = self.ref
        kmer = lambda p: fc.canon_of(ref[p:p + k])  # noqa: E731
        g0 = self.junction[0] - k + 1            # the gap of site j spans the positions junction - k + 1 .. junction - 1
        solid.add(kmer(g0 + 10))                 # site 0: one isolated solid k-mer inside the gap: counted into it
        g1 = self.junction[1] - k + 1
        solid.update((kmer(g1 + 10), kmer(g1 + 11)))  # site 1: two adjacent ones: they split the gap
        # sites 2 and 3: the micro-assembly's order and its quirk, on the junction's two k-mers L and R
        j2 = self.junction[2]
        L, R = ref[j2 - k:j2], ref[j2:j2 + k]
        self.nt2 = next(c for c in "ACGT" if c != R[0])  # (a nucleotide equal to R's first would be a junction repeat instead)
        solid.update(fc.solid_of_strings([L + self.nt2 + R, L + 2 * self.nt2 + R], k))  # X and XX both assemble: X comes first
        j3 = self.junction[3]
        L, R = ref[j3 - k:j3], ref[j3:j3 + k]
        self.nt3 = next(c for c in "CGTA" if c != R[0])
        text = L + self.nt3 + R
        solid.update(fc.canon_of(text[j:j + k]) for j in range(k))  # the first k windows only: the window k, X + R[:k - 1], stays absent
        assert fc.canon_of(text[k:2 * k]) not in solid
        self.solid = solid
        self.idx = index_of(mtg, solid, k)


@pytest.fixture(scope="module")
def shapes(mtg):
    s = Shapes(mtg, K, 77)
    yield s
    s.idx.close()


def test_isolated_solid_kmers_and_the_order_of_the_micro_assembly(mtg, shapes):
    s = shapes
    got, st = check(s.idx, s.solid, K, [s.ref], MAX_REPEAT)
    by_right = {c[5]: c for c in got}
    j = s.junction
    assert by_right[j[0]][1:4] == (j[0] - 1, 0, 0)          # the isolated k-mer did not end the gap: still k - 1 positions, a clean site
    assert j[1] not in by_right                             # split in two: neither part has k - 1 - r positions
    assert by_right[j[2]][2] == 1 and by_right[j[2]][6] == "ACGT".index(s.nt2)  # X, not XX (an index of 4 or more)
    assert by_right[j[3]][2] == 1 and by_right[j[3]][6] == "ACGT".index(s.nt3)  # on its first k windows alone
    assert by_right[j[6] + 3][1:4] == (j[6] - 1 + 3, 0, 3)    # the planted repeat of 3: a fuzzy site, its right k-mer 3 behind the first solid position
    assert st["n_homo_clean"] >= 5


def test_invalid_characters_around_a_gap(mtg, shapes):
    s = shapes
    ref, k = s.ref, K
    j4, j6 = s.junction[4], s.junction[6]   # site 4: r = 0; site 6: r = 3, its right k-mer as written starts 3 behind the first solid position
    e4 = j4                                 # first solid position behind the gap of a clean site: the junction itself
    put = lambda t, p, ch="N": t[:p] + ch + t[p + 1:]  # noqa: E731
    seqs = [
        ref,
        put(ref, j4 - k - 5),               # before the gap, inside the left k-mer's solid stretch: the stretch restarts, the left k-mer stays valid
        put(ref, j4 - 2),                   # inside the left k-mer: the positions before the gap are invalid, no kmer_begin
        put(ref, j4 - 1, "n"),              # the same with a lower-case n
        put(ref, e4 + k),                   # right behind the k-mer at e: position e + 1 is invalid, e is no anchor
        put(ref, e4 + k + 1),               # one further: e and e + 1 stand, the gap is reported
        put(ref, j6 + k + 1),               # site 6: inside the shifted right k-mer but behind the k-mers at e and e + 1: reported, not called
        put(ref, j6 + k + 2),
        put(ref, j6 + k + 3),               # behind the shifted right k-mer
        ref[:j6 + k + 2],                   # the sequence ends inside the shifted right k-mer
        ref[:j6 + k + 3],
        ref[:j6 + k + 4],
    ]
    got, st = check(s.idx, s.solid, k, seqs, MAX_REPEAT)
    per = lambda i: [c for c in got if c[0] == i]  # noqa: E731
    base = len(per(0))
    assert len(per(2)) == base - 1 and len(per(3)) == base - 1 and len(per(4)) == base - 1 and len(per(5)) == base and len(per(1)) == base
    assert len(per(6)) == base - 1 and len(per(7)) == base - 1 and len(per(8)) == base
    assert len(per(9)) + 1 == len(per(10)) == len(per(11))


def test_sequence_boundaries_and_short_sequences(mtg, shapes):
    s = shapes
    ref, k, j = s.ref, K, s.junction
    rng = np.random.default_rng(5)
    seqs = [
        ref[j[4] - 10:j[4] + 200],           # starts inside the left k-mer: the gap touches the start, no kmer_begin
        ref[j[4] - k:j[4] + 200],            # the left k-mer is position 0: one solid position before the gap is no stretch of two
        ref[j[4] - k - 1:j[4] + 200],        # two: a kmer_begin
        ref[j[4] - 200:j[4] + k],            # ends with the k-mer at e: not reported
        ref[j[4] - 200:j[4] + k + 1],        # ends with the k-mer at e + 1: reported
        ref[j[4] - 200:j[4] + 5],            # the gap touches the end
        ref[100:100 + k - 1], ref[100:100 + k], ref[100:100 + k + 1], "", "A",
        fc.rand_seq(rng, k - 1), fc.rand_seq(rng, k), fc.rand_seq(rng, k + 1),
        ref[700:700 + k] + fc.rand_seq(rng, 40) + ref[1200:1300],  # an isolated solid first k-mer, then a gap: no kmer_begin
    ]
    got, st = check(s.idx, s.solid, k, seqs, MAX_REPEAT)
    assert [c[0] for c in got] == [2, 4]


def test_gaps_across_the_word_and_tile_seams_in_many_short_sequences(mtg, shapes):
    """the gap of a clean site slid over the positions 63 / 64 and 255 / 256 (the plane's word, the scan's tile): 200 sequences, so that the
    candidates also cross waves and workgroups of the observers' kernel"""
    s = shapes
    ref, k = s.ref, K
    seqs = []
    for site, seam in ((4, 64), (5, 256), (6, 64), (7, 256), (2, 64)):
        jn = s.junction[site]
        for d in range(40):  # the gap's first position jn - k + 1 lands on seam - 35 + d .. : every alignment across the seam
            start = jn - k + 1 - (seam - 35 + d)
            seqs.append(ref[start:jn + 120])
    assert len(seqs) == 200
    got, st = check(s.idx, s.solid, k, seqs, MAX_REPEAT)
    assert len(set(c[0] for c in got)) == 200


def test_one_long_sequence_with_2000_sites(mtg):
    """300 000 nt with an insertion of 1, 2, 3 or 50 nt every 150: the compaction of gaps, candidates and calls over many workgroups"""
    k = 21
    rng = np.random.default_rng(9)
    sites = [(200 + 160 * i, (1, 2, 3, 50)[i % 4]) for i in range(2000)]
    donor = fc.rand_seq(rng, 200 + 160 * 2000 + 8000)
    ref = fc.planted(rng, donor, k, sites)
    assert len(ref) > 300000
    solid = fc.solid_of_strings([donor], k)
    idx = index_of(mtg, solid, k)
    try:
        got, st = check(idx, solid, k, [ref], MAX_REPEAT)
        assert len(got) > 1500 and st["n_gaps"] >= 2000
        calls, st2 = idx.find_homo_sequences([ref], MAX_REPEAT, cap=700)
        assert st2["n_calls"] == len(got) and [tuple(int(x) for x in c) for c in calls] == got[:700]
        total, dev, st3 = packed_device_calls(idx, [ref], k, MAX_REPEAT, 300)
        assert total == len(got) and dev == got[:300]
    finally:
        idx.close()
