"""`find` for heterozygous insertions on the device (k_profile<true>, k_het_count / k_het_list, k_het_judge, k_het_chain, k_het_final, k_het_emit in
csrc/mtg_gpu_misc.hip behind mtg_index_find_het_sequences / _packed_device and `MindTheGap find -hete-only | -insert-only`) against the plain
model of tests/find_het_cases.py: the literal loop of FindHeteroInsertion::update with its ring of 256 history slots.  Every comparison is
exact, calls and statistics.

The synthetic cases index the k-mers of a reference and of donors, each donor the reference with one insertion (find_cases.planted /
with_repeat where the junction repeat matters); single k-mers are added where a case needs a branching node or a k-mer of out-degree 2 at a
chosen position."""
import os
import subprocess

import numpy as np
import pytest

from tests import find_cases as fc
from tests import find_het_cases as fh
from tests import profile_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FASTQ_PAIR = [os.path.join(GOLDEN, "data", "reads_r1.fastq"), os.path.join(GOLDEN, "data", "reads_r2.fastq")]
REFERENCE = os.path.join(GOLDEN, "full_test", "reference.fasta")
K, CUTOFF, MAX_REPEAT, BRANCHING = 31, 7, 5, 15


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
    want, wst = fh.find_het(solid, K, seqs, None, MAX_REPEAT, BRANCHING)
    assert len(want) == 9 and fh.repeated_set(seqs, K, 1) == set()  # tests/test_find_het_cpu.py holds the list itself
    idx = mtg.Index.from_reads(FASTQ_PAIR, K, CUTOFF)
    yield idx, solid, names, seqs, want, wst
    idx.close()


def index_of(mtg, solid, k):
    kms = np.array(sorted(solid), dtype=np.uint64)
    return mtg.Index.from_kmers(kms, np.full(len(kms), 9, dtype=np.uint32), k)


def tuples(calls):
    return [tuple(int(x) for x in c) for c in calls]


def check(idx, solid, k, seqs, flags=None, max_repeat=MAX_REPEAT, branching=BRANCHING):
    """find on the device against the model: calls and statistics; returns (calls as tuples, statistics of the model)"""
    rep = None if flags is None else [np.frombuffer(f, dtype=np.uint8) for f in flags]
    calls, st = idx.find_het_sequences(seqs, rep, max_repeat, branching)
    want, wst = fh.find_het(solid, k, seqs, flags, max_repeat, branching)
    got = tuples(calls)
    assert calls.dtype == fc.CALL_DTYPE
    diff = [i for i in range(min(len(got), len(want))) if got[i] != want[i]]
    assert not diff and len(got) == len(want), "%d calls, expected %d; first difference: %r, expected %r" % (
        len(got), len(want), got[diff[0]] if diff else got[len(want):][:1], want[diff[0]] if diff else want[len(got):][:1])
    assert {x: st[x] for x in fh.STAT_KEYS} == wst and st["n_calls"] == len(want)
    assert st["n_positions"] == sum(max(len(s) - k + 1, 0) for s in seqs)
    return got, wst


def pack(seqs, flags):
    """(packed words, word offsets, lengths, repeat plane) in the layout of mtg_index_profile_packed_device / mtg_index_scan_packed_device"""
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    word_off = np.zeros(len(seqs), dtype=np.uint64)
    nw = 0
    for i, n in enumerate(lens):
        word_off[i] = nw
        nw += (int(n) + 31) // 32 + 1
    packed, plane = np.zeros(nw + 1, dtype=np.uint64), np.zeros(nw + 1, dtype=np.uint64)
    for i, s in enumerate(seqs):
        codes = (np.frombuffer(s.encode(), dtype=np.uint8).astype(np.uint64) >> np.uint64(1)) & np.uint64(3)
        for j0 in range(0, len(s), 32):
            c = codes[j0:j0 + 32]
            packed[int(word_off[i]) + (j0 >> 5)] = np.bitwise_or.reduce(c << (np.arange(len(c), dtype=np.uint64) * np.uint64(2)))
        if flags is not None:
            for q, f in enumerate(flags[i]):
                if f:
                    plane[int(word_off[i]) + (q >> 6)] |= np.uint64(1) << np.uint64(q & 63)
    return packed, word_off, lens, plane


def packed_device_calls(idx, seqs, flags, max_repeat, branching, cap):
    import torch
    packed, word_off, lens, plane = pack(seqs, flags)
    dev = torch.device("cuda", 0)
    d_w = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_wo = torch.from_numpy(word_off.view(np.int64)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_rep = torch.from_numpy(plane.view(np.int64)).to(dev)
    d_calls = torch.full((max(cap, 1) * 7 + 7,), -1, dtype=torch.int32, device=dev)
    total, st = idx.find_het_packed_device(d_w.data_ptr(), d_wo.data_ptr(), d_ln.data_ptr(), len(seqs), d_rep.data_ptr() if flags is not None else None, max_repeat, branching,
                                           d_calls.data_ptr() if cap else None, cap)
    torch.cuda.synchronize()
    raw = d_calls.cpu().numpy().view(np.uint32)
    n = min(total, cap)
    assert (raw[7 * n:] == 0xFFFFFFFF).all()  # nothing behind the calls that were asked for
    return total, tuples(raw[:7 * n].view(fc.CALL_DTYPE)), st


def other(rng, *chars):
    return "ACGT"[[i for i in range(4) if "ACGT"[i] not in chars][int(rng.integers(4 - len(set(chars))))]]


def donor_with(rng, ref, a, n):
    """the reference with n random nucleotides inserted before position a, no junction repeat on either side"""
    ins = list(fc.rand_seq(rng, n))
    ins[0] = other(rng, ref[a])
    ins[-1] = other(rng, ref[a - 1]) if n > 1 else other(rng, ref[a], ref[a - 1])
    return ref[:a] + "".join(ins) + ref[a:]


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def second_successor(rng, ref, q, k):
    """a k-mer that gives the reference's k-mer at q a second successor (out-degree 2: a branching node, and a left k-mer for the observer)"""
    return fc.canon_of(ref[q + 1:q + k] + other(rng, ref[q + k]))


# ------------------------------------------------------------------------------------------------ 1. the reference's goldens
def test_golden_calls_by_both_entries(mtg, golden):
    idx, solid, names, seqs, want, wst = golden
    calls, st = idx.find_het_sequences(seqs, None, MAX_REPEAT, BRANCHING)
    assert tuples(calls) == want and {x: st[x] for x in fh.STAT_KEYS} == wst and st["n_calls"] == 9
    zero = [np.zeros(max(len(s) - K + 2, 0), dtype=np.uint8) for s in seqs]
    assert tuples(idx.find_het_sequences(seqs, zero, MAX_REPEAT, BRANCHING)[0]) == want
    for cap in (20, 9, 4, 0):
        total, got, st2 = packed_device_calls(idx, seqs, None, MAX_REPEAT, BRANCHING, cap)
        assert total == 9 and got == want[:cap] and {x: st2[x] for x in fh.STAT_KEYS} == wst
        calls, st3 = idx.find_het_sequences(seqs, None, MAX_REPEAT, BRANCHING, cap=cap)
        assert st3["n_calls"] == 9 and tuples(calls) == want[:cap]
    with pytest.raises(mtg.MtgError):
        idx.find_het_sequences(seqs, None, -1)
    big = tuples(idx.find_het_sequences(seqs, None, 1000, BRANCHING)[0])  # above k - 2: as k - 2
    assert big == fh.find_het(solid, K, seqs, None, 1000, BRANCHING)[0] == tuples(idx.find_het_sequences(seqs, None, K - 2, BRANCHING)[0])
    assert idx.find_het_sequences([], None)[1]["n_calls"] == 0  # nseq = 0


def test_find_tool_under_the_three_flags(mtg, golden, tmp_path):
    idx, solid, names, seqs, want, wst = golden
    exe = os.path.join(os.path.dirname(mtg.build_library()), "MindTheGap")
    homo, _ = fc.find_homo(solid, K, seqs, MAX_REPEAT)
    small = [c for c in homo if c[2] == 1]  # -hete-only keeps the observers of homozygous insertions of 1-2 nt (src/Finder.cpp:364-373,562-566)
    expected = {"-hete-only": fh.lines(fh.merge(small, want), names, seqs, K), "-insert-only": fh.lines(fh.merge(homo, want), names, seqs, K), "-homo-insertions": fc.breakpoint_lines(homo, names, seqs, K)}
    for flag, (bk, vcf) in expected.items():
        out = str(tmp_path / ("found" + flag))
        r = subprocess.run([exe, "find", "-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, flag, "-abundance-min", str(CUTOFF), "-out", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(out + ".breakpoints").read().splitlines() == bk, flag
        lines = open(out + ".othervariants.vcf").read().splitlines()
        assert lines[9] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tG1" and lines[10:] == vcf, flag
        if flag == "-homo-insertions":
            assert "heterozygous" not in r.stdout and "hete_insertions                          : no" in r.stdout and "homozygous                               : 3" in r.stdout
        else:
            assert "heterozygous                             : 2" in r.stdout and "Heterozygous insertions 1-2 bp size      : 7" in r.stdout
            assert "hete_insertions                          : yes" in r.stdout and "branching filter value                   : 15" in r.stdout
            assert ("homozygous                               : 3" if flag == "-insert-only" else "homozygous                               : 0") in r.stdout
            assert "Homozygous insertions 1-2 bp size        : 10" in r.stdout and ("homo_insertions                          : " + ("yes" if flag == "-insert-only" else "no")) in r.stdout
    assert len(os.listdir(str(tmp_path))) == 6


# ------------------------------------------------------------------------------------------------ 2. insertions of every length and repeat
@pytest.mark.parametrize("k", [31, 13])
def test_planted_insertions_of_every_length_and_repeat(mtg, k):
    """heterozygous insertions of 1, 2, 3, 10 and 40 nt with junction repeats 0 .. max_repeat, one per sequence of 300-700 nt; the junctions
    are put around the positions 64 n and 256 (the plane's word, the scan's tile)"""
    rng = np.random.default_rng(2000 + k)
    spots = [63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 258, 319, 320, 321, 383]
    seqs, solid = [], set()
    for i, (n, r) in enumerate((n, r) for n in (1, 2, 3, 10, 40) for r in range(0, MAX_REPEAT + 1)):
        a = spots[i % len(spots)] + (0, k, k + 3)[i % 3]          # the junction in the reference; the observer fires at k-mer position a
        length = int(rng.integers(max(300, a + 2 * k + 10), 701))
        donor = fc.with_repeat(rng, fc.rand_seq(rng, length + n), a, n, r)
        ref = fc.planted(rng, donor, k, [(a, n)])
        seqs.append(ref)
        solid |= fc.solid_of_strings([ref, donor], k)
    idx = index_of(mtg, solid, k)
    try:
        got, st = check(idx, solid, k, seqs)
        assert st["n_het_small"] >= 8 and st["n_het_clean"] >= 3 and st["n_het_fuzzy"] >= 10 and len(set(c[0] for c in got)) >= 28
        assert set(c[3] for c in got) == set(range(MAX_REPEAT + 1))
        assert {c[5] - c[3] < 256 for c in got} == {True, False} and {(c[5] - c[3]) % 64 for c in got} >= {63, 0, 1}
        got0, st0 = check(idx, solid, k, seqs, max_repeat=0)
        assert set(c[3] for c in got0) == {0} and 0 < len(got0) < len(got)
        n = len(got)
        for cap in (0, 1, n - 1, n, n + 3):  # capacity: the count is the total, the leading records are the same
            calls, stc = idx.find_het_sequences(seqs, None, MAX_REPEAT, BRANCHING, cap=cap)
            assert stc["n_calls"] == n and tuples(calls) == got[:cap]
        total, dev, std = packed_device_calls(idx, seqs, None, MAX_REPEAT, BRANCHING, n + 2)  # a packed device input against the host-string entry
        assert total == n and dev == got and {x: std[x] for x in fh.STAT_KEYS} == st
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 3. one index for the hand-built shapes
class Shapes:
    """random references of 500-700 nt, one per scenario, and donors that carry one insertion each"""

    def __init__(self, mtg, k, seed):
        rng = np.random.default_rng(seed)
        self.k, self.rng, self.seqs, self.solid, self.tag = k, rng, [], set(), {}

    def add(self, tag, ref, sites=(), small=(), branching=(), out2=(), index=True):
        """sites: junctions of insertions of 12 nt; small: junctions of insertions of 1 nt; branching / out2: positions whose k-mer gets a
        second successor"""
        k, rng = self.k, self.rng
        if index:
            self.solid |= fc.solid_of_strings([ref.upper().replace("N", "A")], k)  # (a sequence with an N or one that the graph is not to know: index=False)
        up = ref.upper().replace("N", "A")
        for a in sites:
            self.solid |= fc.solid_of_strings([donor_with(rng, up, a, 12)[a - k:a + 12 + k]], k)
        for a in small:
            self.solid |= fc.solid_of_strings([donor_with(rng, up, a, 1)[a - k:a + 1 + k]], k)
        for q in tuple(branching) + tuple(out2):
            self.solid.add(second_successor(rng, up, q, k))
        self.tag[tag] = len(self.seqs)
        self.seqs.append(ref)

    def build(self, mtg):
        self.idx = index_of(mtg, self.solid, self.k)


def calls_of(got, shapes, tag):
    return [c for c in got if c[0] == shapes.tag[tag]]


def test_raw_sites_close_to_each_other(mtg):
    """two and three raw sites 1 .. max_repeat + 1 apart: the second is silenced up to max_repeat and called at max_repeat + 1; of three sites 3
    apart the first and the third are called (a silenced site silences nothing); an insertion of 1 nt inside a site's window is silenced, one
    just outside is called, and an insertion silences nothing"""
    s = Shapes(mtg, K, 31)
    rng = s.rng
    for d in range(1, MAX_REPEAT + 2):
        s.add("two%d" % d, fc.rand_seq(rng, 500), sites=(250, 250 + d))
    s.add("three", fc.rand_seq(rng, 500), sites=(250, 253, 256))
    s.add("three_seam", fc.rand_seq(rng, 500), sites=(254, 257, 260))
    s.add("small_inside", fc.rand_seq(rng, 500), sites=(250,), small=(250 + MAX_REPEAT,))
    s.add("small_outside", fc.rand_seq(rng, 500), sites=(250,), small=(250 + MAX_REPEAT + 1,))
    s.add("small_then_site", fc.rand_seq(rng, 500), sites=(252,), small=(250,))
    s.build(mtg)
    try:
        got, st = check(s.idx, s.solid, K, s.seqs)
        for d in range(1, MAX_REPEAT + 2):
            assert [c[5] for c in calls_of(got, s, "two%d" % d)] == ([250] if d <= MAX_REPEAT else [250, 250 + d]), d
        assert [c[5] for c in calls_of(got, s, "three")] == [250, 256] and [c[5] for c in calls_of(got, s, "three_seam")] == [254, 260]
        assert [c[2] for c in calls_of(got, s, "small_inside")] == [2] and [c[2] for c in calls_of(got, s, "small_outside")] == [2, 3]
        assert [c[2] for c in calls_of(got, s, "small_then_site")] == [3, 2]
        assert st["n_suppressed"] == MAX_REPEAT + 3 and st["n_raw_sites"] == 2 * (MAX_REPEAT + 1) + 9
        got1, st1 = check(s.idx, s.solid, K, s.seqs, max_repeat=1)
        assert [c[5] for c in calls_of(got1, s, "two1")] == [250] and [c[5] for c in calls_of(got1, s, "two2")] == [250, 252]
        check(s.idx, s.solid, K, s.seqs, max_repeat=0)
    finally:
        s.idx.close()


def test_branching_filter(mtg):
    """branching nodes planted in the 100 history slots before the window: filter 0, 15 and none; the slots 100 and 101 back; a window clipped
    by the start of the sequence; a refused site silences nothing"""
    s = Shapes(mtg, K, 32)
    rng = s.rng
    p = 300
    s.add("none", fc.rand_seq(rng, 500), sites=(p,))
    s.add("at100", fc.rand_seq(rng, 500), sites=(p,), branching=(p - K - 100,))
    s.add("at101", fc.rand_seq(rng, 500), sites=(p,), branching=(p - K - 101,))
    s.add("at1", fc.rand_seq(rng, 500), sites=(p,), branching=(p - K - 1,))
    s.add("fifteen", fc.rand_seq(rng, 500), sites=(p,), branching=tuple(p - K - 3 - 6 * j for j in range(15)))
    s.add("sixteen", fc.rand_seq(rng, 500), sites=(p,), branching=tuple(p - K - 3 - 6 * j for j in range(16)))
    s.add("clipped", fc.rand_seq(rng, 500), sites=(K + 40,), branching=(0, 5, 38))
    # two branching slots 99 and 100 back for the first site, out of reach for the second, whose window holds the first site's left k-mer instead
    s.add("refused_then_site", fc.rand_seq(rng, 500), sites=(p, p + 3), branching=(p - K - 100, p - K - 99))
    s.build(mtg)
    try:
        sites = lambda got, tag: [c[5] for c in calls_of(got, s, tag)]  # noqa: E731
        got, st = check(s.idx, s.solid, K, s.seqs, branching=0)
        assert sites(got, "none") == [p] and sites(got, "at100") == [] and sites(got, "at101") == [p] and sites(got, "at1") == [] and sites(got, "clipped") == []
        assert sites(got, "refused_then_site") == [] and st["n_filtered"] == 7 and st["n_suppressed"] == 0
        got, st = check(s.idx, s.solid, K, s.seqs, branching=1)
        assert sites(got, "refused_then_site") == [p + 3] and st["n_suppressed"] == 0  # the refused site silences nothing
        got, st = check(s.idx, s.solid, K, s.seqs, branching=15)
        assert sites(got, "fifteen") == [p] and sites(got, "sixteen") == [] and sites(got, "clipped") == [K + 40] and st["n_filtered"] == 1
        assert sites(got, "refused_then_site") == [p] and st["n_suppressed"] == 1
        got, st = check(s.idx, s.solid, K, s.seqs, branching=2)
        assert sites(got, "clipped") == [] and st["n_filtered"] == 3
        got, st = check(s.idx, s.solid, K, s.seqs, branching=-1)
        assert st["n_filtered"] == 0 and len(got) == 8
    finally:
        s.idx.close()


def test_repeat_flags(mtg, tmp_path):
    """a repeat flag on the prefix of p, on the suffix of q, on both and next to them, passed through `repeated`; then through the tool, on a
    genome in which the (k-1)-mer is really there twice"""
    s = Shapes(mtg, K, 33)
    rng = s.rng
    p = 260
    base = fc.rand_seq(rng, 600)
    for tag in ("plain", "prefix", "suffix", "both", "beside"):
        s.add(tag, base if tag == "plain" else fc.rand_seq(rng, 600), sites=(p,))
    dup_prefix = fc.rand_seq(rng, 600)
    s.add("dup_prefix", dup_prefix, sites=(p,))
    # the prefix (k-1)-mer of position p once more, in a sequence the graph does not know (its k-mers would be further neighbours)
    s.add("copy_prefix", fc.rand_seq(rng, 100) + other(rng, dup_prefix[p - 1]) + dup_prefix[p:p + K - 1] + other(rng, dup_prefix[p + K - 1]) + fc.rand_seq(rng, 100), index=False)
    dup_suffix = fc.rand_seq(rng, 600)
    s.add("dup_suffix", dup_suffix, sites=(p,))
    s.add("copy_suffix", fc.rand_seq(rng, 90) + other(rng, revcomp(dup_suffix[p])) + revcomp(dup_suffix[p - K + 1:p]) + other(rng, revcomp(dup_suffix[p - K])) + fc.rand_seq(rng, 90),
          index=False)  # the suffix of q, on the other strand
    s.build(mtg)
    try:
        flags = [bytearray(max(len(x) - K + 2, 0)) for x in s.seqs]
        flags[s.tag["prefix"]][p] = 1
        flags[s.tag["suffix"]][p - K + 1] = 1
        flags[s.tag["both"]][p] = flags[s.tag["both"]][p - K + 1] = 1
        for q in (p - 1, p + 1, p - K, p - K + 2):
            flags[s.tag["beside"]][q] = 1
        flags = [bytes(f) for f in flags]
        got, st = check(s.idx, s.solid, K, s.seqs, flags)
        called = set(c[0] for c in got)
        assert called == {s.tag[t] for t in ("plain", "beside", "dup_prefix", "dup_suffix")}
        n = len(got)
        total, dev, std = packed_device_calls(s.idx, s.seqs, flags, MAX_REPEAT, BRANCHING, n + 1)  # the repeat plane in the scan's device layout
        assert total == n and dev == got and {x: std[x] for x in fh.STAT_KEYS} == st
        # the genome's own repeats: the exact set, as the tool makes it
        rep = fh.repeated_set(s.seqs, K, 1)
        assert len(rep) == 2
        real = fh.repeat_flags(s.seqs, K, rep)
        got2, st2 = check(s.idx, s.solid, K, s.seqs, real)
        assert set(c[0] for c in got2) == {s.tag[t] for t in ("plain", "prefix", "suffix", "both", "beside")}
        exe = os.path.join(os.path.dirname(mtg.build_library()), "MindTheGap")
        graph, genome, out = str(tmp_path / "g.mtg"), str(tmp_path / "genome.fa"), str(tmp_path / "found")
        s.idx.save(graph)
        names = ["chr%d" % i for i in range(len(s.seqs))]
        with open(genome, "w") as f:
            for n_, x in zip(names, s.seqs):
                f.write(">%s\n%s\n" % (n_, "\n".join(x[i:i + 70] for i in range(0, len(x), 70))))
        r = subprocess.run([exe, "find", "-graph", graph, "-ref", genome, "-hete-only", "-out", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        small = [c for c in fc.find_homo(s.solid, K, s.seqs, MAX_REPEAT)[0] if c[2] == 1]
        bk, vcf = fh.lines(fh.merge(small, got2), names, s.seqs, K)
        assert open(out + ".breakpoints").read().splitlines() == bk and open(out + ".othervariants.vcf").read().splitlines()[10:] == vcf
        # het-max-occ 2: twice is not repeated any more
        r = subprocess.run([exe, "find", "-graph", graph, "-ref", genome, "-hete-only", "-het-max-occ", "2", "-out", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got3, _ = check(s.idx, s.solid, K, s.seqs, None)
        assert open(out + ".breakpoints").read().splitlines() == fh.lines(fh.merge(small, got3), names, s.seqs, K)[0] and len(got3) == 7
    finally:
        s.idx.close()


def test_invalid_characters_and_sequence_ends(mtg):
    """N and lower case inside the left k-mer, in the window and in the right k-mer; a stale history slot that is really read (the window's
    positions invalid, a k-mer of out-degree 2 256 positions before); a right k-mer that runs past the end; a site within k of the start"""
    s = Shapes(mtg, K, 34)
    rng = s.rng
    p = 400
    put = lambda t, i, ch="N": t[:i] + ch + t[i + 1:]  # noqa: E731
    base = fc.rand_seq(rng, 700)
    s.add("plain", base, sites=(p,))
    s.add("n_in_left", put(base, p - K + 3), index=False)           # the k-mer at p - k is invalid: its slot holds what position p - k - 256 left there (nothing of out-degree 2)
    s.add("n_before_left", put(base, p - K - 1), index=False)       # the left k-mer stands
    s.add("n_in_right", put(base, p + 4), index=False)              # p itself is invalid: no observer
    s.add("n_behind_right", put(base, p + K), index=False)
    s.add("lower", base[:p - K] + base[p - K:p + K].lower() + base[p + K:])
    s.add("lower_n", put(base, p - K - 1, "n"), index=False)
    fuzzy = fc.rand_seq(rng, 700)                      # a site whose first qualifying slot is i = 2: the right k-mer as written starts at p + 2
    s.add("fuzzy", fuzzy, sites=(), out2=())
    s.solid |= fc.solid_of_strings([donor_with(rng, fuzzy, p, 12)[p:p + 12 + K]], K)   # in-degree 2 at p (the donor's way into the right flank)
    s.solid.add(second_successor(rng, fuzzy, p - K + 2, K))
    s.add("fuzzy_n_in_right", put(fuzzy, p + K + 1), index=False)   # inside the shifted right k-mer, behind the k-mer at p: the observer returns without a call
    s.add("fuzzy_n_behind", put(fuzzy, p + K + 2), index=False)
    s.add("fuzzy_end_short", fuzzy[:p + K + 1])        # the sequence ends inside the shifted right k-mer
    s.add("fuzzy_end", fuzzy[:p + K + 2])
    stale = fc.rand_seq(rng, 700)                      # the window p - k .. p - k + 5 invalid (an N at p - 1), out-degree 2 at p - k + 2 - 256
    s.solid |= fc.solid_of_strings([stale], K)
    s.add("stale", put(stale, p - 1), index=False)
    s.solid |= fc.solid_of_strings([donor_with(rng, stale, p, 12)[p:p + 12 + K]], K)
    s.solid.add(second_successor(rng, stale, p - K + 2 - 256, K))
    start = fc.rand_seq(rng, 300)
    s.add("start_k", start, sites=(K,))                # the left k-mer is position 0
    s.add("start_k1", fc.rand_seq(rng, 300), sites=(K + 1,))
    end = fc.rand_seq(rng, 300)
    s.add("end", end[:200 + K], sites=(200,))          # the right k-mer is the last one
    s.build(mtg)
    try:
        got, st = check(s.idx, s.solid, K, s.seqs)
        sites = lambda tag: [(c[2], c[3], c[4], c[5]) for c in calls_of(got, s, tag)]  # noqa: E731
        assert sites("plain") == [(2, 0, p - K, p)] == sites("n_before_left") == sites("n_behind_right") == sites("lower") == sites("lower_n")
        assert sites("n_in_left") == [] and sites("n_in_right") == []
        assert sites("fuzzy") == [(2, 2, p - K + 2, p + 2)] == sites("fuzzy_n_behind") == sites("fuzzy_end") and sites("fuzzy_n_in_right") == [] and sites("fuzzy_end_short") == []
        assert sites("stale") == [(2, 2, p - K + 2 - 256, p + 2)]
        assert sites("start_k") == [(2, 0, 0, K)] and sites("start_k1") == [(2, 0, 1, K + 1)] and sites("end") == [(2, 0, 200 - K, 200)]
        assert st["n_candidates"] == len(got) + 2  # the two early returns
    finally:
        s.idx.close()


def test_many_short_sequences(mtg):
    """300 sequences of 0 .. 120 nt around one site, slid so that it meets both ends and the word seam, among sequences shorter than k: the
    candidates cross waves and workgroups of the judging kernel"""
    rng = np.random.default_rng(35)
    ref = fc.rand_seq(rng, 400)
    p = 200
    solid = fc.solid_of_strings([ref, donor_with(rng, ref, p, 12)], K)
    seqs = []
    for i in range(300):
        if i % 10 == 9:
            seqs.append(ref[:int(rng.integers(0, K))])
        else:
            a = p - K - (i % 70)
            seqs.append(ref[max(a, 0):p + K + (i % 7) - 2])
    idx = index_of(mtg, solid, K)
    try:
        got, st = check(idx, solid, K, seqs)
        assert 150 < len(got) < 270 and st["n_candidates"] == len(got) and len(set(c[5] for c in got)) > 40 and {c[5] < 64 for c in got} == {True, False}
        total, dev, std = packed_device_calls(idx, seqs, None, MAX_REPEAT, BRANCHING, 100)
        assert total == len(got) and dev == got[:100]
    finally:
        idx.close()
