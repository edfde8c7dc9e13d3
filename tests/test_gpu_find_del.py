"""`find` for homozygous deletions on the device (k_del_mark, k_del_judge, k_del_emit in csrc/mtg_gpu_misc.hip behind
mtg_index_find_del_sequences / _packed_device and `MindTheGap find -deletion-only | -homo-only -no-snp | -no-snp`) against the plain model of
tests/find_del_cases.py: the literal FindDeletion::update inside the literal loop of the scan.  Every comparison is exact, calls and
statistics.

The synthetic cases index the k-mers of donors, each donor a sequence with one stretch cut out (a homozygous deletion: the graph does not
know the sequence's own allele); find_cases.with_repeat makes the junction repeat where it matters."""
import os
import subprocess

import numpy as np
import pytest

from tests import find_cases as fc
from tests import find_del_cases as fd
from tests import find_het_cases as fh
from tests import profile_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FASTQ_PAIR = [os.path.join(GOLDEN, "data", "reads_r1.fastq"), os.path.join(GOLDEN, "data", "reads_r2.fastq")]
REFERENCE = os.path.join(GOLDEN, "full_test", "reference.fasta")
K, CUTOFF, MAX_REPEAT, BRANCHING = 31, 7, 5, 15
VCF_COLUMNS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tG1"


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
    want, wst = fd.find_del(solid, K, seqs, MAX_REPEAT)
    assert len(want) == 3  # tests/test_find_del_cpu.py holds the list itself
    idx = mtg.Index.from_reads(FASTQ_PAIR, K, CUTOFF)
    yield idx, solid, names, seqs, want, wst
    idx.close()


def index_of(mtg, solid, k):
    kms = np.array(sorted(solid), dtype=np.uint64)
    return mtg.Index.from_kmers(kms, np.full(len(kms), 9, dtype=np.uint32), k)


def tuples(calls):
    return [tuple(int(x) for x in c) for c in calls]


def check(idx, solid, k, seqs, max_repeat=MAX_REPEAT):
    """find on the device against the model: calls and statistics; returns (calls as tuples, statistics of the model)"""
    calls, st = idx.find_del_sequences(seqs, max_repeat)
    want, wst = fd.find_del(solid, k, seqs, max_repeat)
    got = tuples(calls)
    assert calls.dtype == fc.CALL_DTYPE
    diff = [i for i in range(min(len(got), len(want))) if got[i] != want[i]]
    assert not diff and len(got) == len(want), "%d calls, expected %d; first difference: %r, expected %r" % (
        len(got), len(want), got[diff[0]] if diff else got[len(want):][:1], want[diff[0]] if diff else want[len(got):][:1])
    assert {x: st[x] for x in fd.STAT_KEYS} == wst
    assert st["n_positions"] == sum(max(len(s) - k + 1, 0) for s in seqs)
    return got, wst


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


def packed_device_calls(idx, seqs, max_repeat, cap):
    import torch
    packed, word_off, lens = pack(seqs)
    dev = torch.device("cuda", 0)
    d_w = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_wo = torch.from_numpy(word_off.view(np.int64)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_calls = torch.full((max(cap, 1) * 7 + 7,), -1, dtype=torch.int32, device=dev)
    total, st = idx.find_del_packed_device(d_w.data_ptr(), d_wo.data_ptr(), d_ln.data_ptr(), len(seqs), max_repeat, d_calls.data_ptr() if cap else None, cap)
    torch.cuda.synchronize()
    raw = d_calls.cpu().numpy().view(np.uint32)
    n = min(total, cap)
    assert (raw[7 * n:] == 0xFFFFFFFF).all()  # nothing behind the calls that were asked for
    return total, tuples(raw[:7 * n].view(fc.CALL_DTYPE)), st


def sequence_with_deletion(rng, length, a, n, r):
    """(sequence, donor): a random sequence of length + n nt whose stretch [a, a + n) the donor lacks, with a junction repeat of exactly r"""
    seq = fd.with_del_repeat(rng, fc.rand_seq(rng, length + n), a, n, r)
    return seq, fd.deleted(seq, a, n)


# ------------------------------------------------------------------------------------------------ 1. the reference's goldens
def test_golden_calls_by_both_entries(mtg, golden):
    idx, solid, names, seqs, want, wst = golden
    calls, st = idx.find_del_sequences(seqs, MAX_REPEAT)
    assert tuples(calls) == want and {x: st[x] for x in fd.STAT_KEYS} == wst and st["n_calls"] == 3
    assert st["n_positions"] == sum(max(len(s) - K + 1, 0) for s in seqs)
    for cap in (5, 3, 1, 0):
        total, got, st2 = packed_device_calls(idx, seqs, MAX_REPEAT, cap)
        assert total == 3 and got == want[:cap] and {x: st2[x] for x in fd.STAT_KEYS} == wst
        calls, st3 = idx.find_del_sequences(seqs, MAX_REPEAT, cap=cap)
        assert st3["n_calls"] == 3 and tuples(calls) == want[:cap]
    with pytest.raises(mtg.MtgError):
        idx.find_del_sequences(seqs, -1)
    big = tuples(idx.find_del_sequences(seqs, 1000)[0])  # above k - 2: as k - 2
    assert big == fd.find_del(solid, K, seqs, 1000)[0] == tuples(idx.find_del_sequences(seqs, K - 2)[0])
    calls, st0 = idx.find_del_sequences([])  # nseq = 0
    assert len(calls) == 0 and all(st0[x] == 0 for x in fd.STAT_KEYS) and st0["n_positions"] == 0


# ------------------------------------------------------------------------------------------------ 2. deletions of every length and repeat
def planted_cases(k):
    """the sequences and the solid set of test 2; ([sequence], solid, index of the first tandem case, index of the fallback case)"""
    rng = np.random.default_rng(3000 + k)
    spots = [63, 64, 65, 127, 128, 255, 256, 257]
    seqs, solid = [], set()
    for i, (n, r) in enumerate((n, r) for n in (1, 2, 5, k - 1, k, k + 1, 60, 300) for r in range(0, MAX_REPEAT + 1)):
        a = spots[i % len(spots)] + (0, k, k + 3)[i % 3]          # the junction: the last nucleotide before the deleted text is a - 1
        length = int(rng.integers(max(300, a + 2 * k + 10), 601))
        seq, donor = sequence_with_deletion(rng, length, a, n, r)
        seqs.append(seq)
        solid |= fc.solid_of_strings([donor], k)
    tandem = len(seqs)
    for d in range(1, 6):                                          # one copy of a unit of d nt deleted from two or three
        for copies in (2, 3):
            seq, donor = fd.tandem_case(rng, d, copies, flank=150)
            seqs.append(seq)
            solid |= fc.solid_of_strings([donor], k)
    fallback = len(seqs)
    a, b, u = fc.rand_seq(rng, 200), fc.rand_seq(rng, 200), "ACG"  # the graph holds ...u u..., the sequence ...u D u...
    d = "T" + fc.rand_seq(rng, 38) + "T"
    seqs.append(a[:-1] + "T" + u + d + u + "T" + b[1:])
    solid |= fc.solid_of_strings([a[:-1] + "T" + u + u + "T" + b[1:]], k)
    return seqs, solid, tandem, fallback


@pytest.mark.parametrize("k", [31, 13])
def test_planted_deletions_of_every_length_and_repeat(mtg, k):
    """deletions of 1, 2, 5, k - 1, k, k + 1, 60 and 300 nt with junction repeats 0 .. max_repeat, one per sequence of 300-900 nt, the
    junctions around the positions 64 n and 256 (the plane's word, the scan's tile); a deleted copy of a tandem unit, which the insertion
    observers would call too; the fallback; max_repeat = 0; capacities; the packed device entry"""
    seqs, solid, tandem, fallback = planted_cases(k)
    idx = index_of(mtg, solid, k)
    try:
        got, st = check(idx, solid, k, seqs)
        plain = [c for c in got if c[0] < tandem]
        assert len(plain) >= 44 and set(c[3] for c in plain) == set(range(MAX_REPEAT + 1)) and set(c[6] for c in plain) == {1, 2, 5, k - 1, k, k + 1, 60, 300}
        assert {c[5] < 256 for c in got} == {True, False} and {(c[1] + 1) % 64 for c in plain} >= {63, 0, 1}
        in_range = [c for c in got if tandem <= c[0] < fallback and k - MAX_REPEAT <= c[5] - c[4] - 1 <= k - 1]
        assert len(in_range) >= 4   # deletion candidates in the insertion observers' length range
        homo = fc.find_homo(solid, k, seqs, MAX_REPEAT)[0]
        assert len(set((c[0], c[4]) for c in homo) & set((c[0], c[4]) for c in in_range)) >= 4   # and they call them
        assert st["n_fallback"] >= 1 and [c[3] for c in got if c[0] == fallback] == [0] and [c[6] for c in got if c[0] == fallback] == [40]   # D alone: what is left is the donor
        got0, st0 = check(idx, solid, k, seqs, max_repeat=0)
        assert set(c[3] for c in got0) == {0} and 0 < len(got0) < len(got) and st0["n_fallback"] == 0
        n = len(got)
        for cap in (0, 1, n - 1, n, n + 3):  # capacity: the count is the total, the leading records are the same
            calls, stc = idx.find_del_sequences(seqs, MAX_REPEAT, cap=cap)
            assert stc["n_calls"] == n and tuples(calls) == got[:cap]
        total, dev, std = packed_device_calls(idx, seqs, MAX_REPEAT, n + 2)  # a packed device input against the host-string entry
        assert total == n and dev == got and {x: std[x] for x in fd.STAT_KEYS} == st
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 3. invalid characters and the ends
def shapes_cases(k):
    """{tag: sequence}, solid: one deletion of 40 nt behind position p - 1 of a base sequence, and variants of it"""
    rng = np.random.default_rng(3400 + k)
    p, n = 300, 40
    base, donor = sequence_with_deletion(rng, 600, p, n, 0)
    solid = fc.solid_of_strings([donor], k)
    put = lambda t, i, ch="N": t[:i] + ch + t[i + 1:]  # noqa: E731
    low = lambda t, i, j: t[:i] + t[i:j].lower() + t[j:]  # noqa: E731
    s = {"plain": base}
    s["n_in_begin"] = put(base, p - 3)                  # the gap has no left anchor any more
    s["n_before_begin"] = put(base, p - k - 2)          # the two k-mers before the gap stand
    s["n_one_before_begin"] = put(base, p - k - 1)      # a single solid k-mer before the gap is no anchor
    s["n_in_gap"] = put(base, p + n // 2)               # two gaps without anchors
    s["lower_n_in_gap"] = put(base, p + n // 2, "n")
    s["n_in_end"] = put(base, p + n + 4)
    s["n_behind_end"] = put(base, p + n + k + 1)        # the second solid k-mer behind the gap stands
    s["n_in_second"] = put(base, p + n + k)             # it does not: the observers are never called
    s["lower_begin"] = low(base, p - k, p)
    s["lower_gap"] = low(base, p, p + n)
    s["lower_end"] = low(base, p + n, p + n + k)
    s["lower_all"] = base.lower()
    s["begin_at_0"] = base[p - k:]                      # kmer_begin would be position 0: one solid k-mer, no anchor
    s["begin_at_1"] = base[p - k - 1:]
    s["end_is_last"] = base[:p + n + k]                 # the right k-mer is the sequence's last: the observers are not called
    s["end_is_last_but_one"] = base[:p + n + k + 1]
    # an isolated present k-mer inside the deleted text is counted into the gap; two adjacent ones end it
    inner, donor2 = sequence_with_deletion(rng, 600, p, 2 * k + 20, 0)
    solid |= fc.solid_of_strings([donor2], k)
    solid.add(fc.canon_of(inner[p + k + 3:p + 2 * k + 3]))
    s["isolated_inside"] = inner
    inner2, donor3 = sequence_with_deletion(rng, 600, p, 2 * k + 20, 0)
    solid |= fc.solid_of_strings([donor3, inner2[p + k + 3:p + 2 * k + 4]], k)
    s["two_inside"] = inner2
    return s, solid, p, n


@pytest.mark.parametrize("k", [31, 13])
def test_invalid_characters_and_sequence_ends(mtg, k):
    s, solid, p, n = shapes_cases(k)
    tags = list(s)
    seqs = [s[t] for t in tags]
    idx = index_of(mtg, solid, k)
    try:
        got, st = check(idx, solid, k, seqs)
        of = lambda tag: [c[1:] for c in got if c[0] == tags.index(tag)]  # noqa: E731
        call = [(p - 1, 4, 0, p - k, p + n, n)]
        for tag in ("plain", "n_before_begin", "n_behind_end", "lower_begin", "lower_gap", "lower_end", "lower_all"):
            assert of(tag) == call, tag
        for tag in ("n_in_begin", "n_one_before_begin", "n_in_gap", "lower_n_in_gap", "n_in_end", "n_in_second", "begin_at_0", "end_is_last"):
            assert of(tag) == [], tag
        assert of("begin_at_1") == [(k, 4, 0, 1, k + 1 + n, n)] and of("end_is_last_but_one") == call
        assert of("isolated_inside") == [(p - 1, 4, 0, p - k, p + 2 * k + 20, 2 * k + 20)] and of("two_inside") == []
        check(idx, solid, k, seqs, max_repeat=0)
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 4. many short sequences
def short_cases():
    rng = np.random.default_rng(38)
    p, n = 200, 20
    ref, donor = sequence_with_deletion(rng, 400, p, n, 2)
    solid = fc.solid_of_strings([donor], K)
    assert fd.find_del(solid, K, [ref], MAX_REPEAT)[0] == [(0, p - 1, 4, 2, p - K + 2, p + n, n)]
    seqs = []
    for i in range(300):
        if i % 10 == 9:
            seqs.append(ref[:int(rng.integers(0, K))])
        else:
            seqs.append(ref[max(p - K - (i % 60), 0):p + n + K + (i % 7) - 2])
    return seqs, solid


def test_many_short_sequences(mtg):
    """300 sequences of 0 .. 150 nt around one deletion, slid so that it meets both ends and the word seam, among sequences shorter than k:
    the candidates cross waves and workgroups of the judging kernel"""
    seqs, solid = short_cases()
    assert max(len(x) for x in seqs) <= 150 and min(len(x) for x in seqs) == 0
    idx = index_of(mtg, solid, K)
    try:
        got, st = check(idx, solid, K, seqs)
        assert 150 < len(got) < 270 and st["n_candidates"] >= len(got) and len(set(c[5] for c in got)) > 40 and {c[5] < 64 for c in got} == {True, False}
        total, dev, std = packed_device_calls(idx, seqs, MAX_REPEAT, 100)
        assert total == len(got) and dev == got[:100]
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 5. the tool
def run_tool(mtg, args, out):
    exe = os.path.join(os.path.dirname(mtg.build_library()), "MindTheGap")
    r = subprocess.run([exe, "find"] + args + ["-out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    vcf = open(out + ".othervariants.vcf").read().splitlines()
    assert vcf[9] == VCF_COLUMNS
    return open(out + ".breakpoints").read().splitlines(), vcf[10:], r.stdout


@pytest.mark.parametrize("flags", [["-deletion-only"], ["-homo-only", "-no-snp"], ["-no-snp"]])
def test_find_tool_on_the_golden(mtg, golden, tmp_path, flags):
    idx, solid, names, seqs, want, wst = golden
    homo, _ = fc.find_homo(solid, K, seqs, MAX_REPEAT)
    het = fh.find_het(solid, K, seqs, None, MAX_REPEAT, BRANCHING)[0] if flags == ["-no-snp"] else []
    layer = homo if "-no-snp" in flags else [c for c in homo if c[2] == 1]   # -deletion-only keeps the observers of insertions of 1-2 nt only
    merged = fd.merge(layer, want, het)
    assert [c for c in merged if c[2] not in (2, 3)] == fd.find_gap_family(solid, K, seqs, MAX_REPEAT, " ".join(flags))   # one literal scan with all gap observers
    bk, vcf = fd.lines(merged, names, seqs, K)
    got_bk, got_vcf, stdout = run_tool(mtg, ["-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-abundance-min", str(CUTOFF)] + flags, str(tmp_path / "found"))
    assert got_bk == bk and got_vcf == vcf
    assert "deletions                                : 3" in stdout and "deletion                                 : yes" in stdout
    assert ("homo_insertions                          : " + ("yes" if "-no-snp" in flags else "no")) in stdout
    assert ("hete_insertions                          : " + ("yes" if flags == ["-no-snp"] else "no")) in stdout and "snp                                      : no" in stdout
    assert ("homozygous                               : %d" % sum(c[2] == 0 for c in merged)) in stdout
    assert ("Homozygous insertions 1-2 bp size        : %d" % sum(c[2] == 1 for c in merged)) in stdout
    if flags == ["-no-snp"]:
        gold = [l.split("\t") for l in open(os.path.join(GOLDEN, "full_test", "gold.othervariants.del.vcf")).read().splitlines()]
        mine = [l.split("\t") for l in got_vcf if "TYPE=DEL" in l]
        assert len(gold) == 2 and all(any(g[:2] + g[3:] == m[:2] + m[3:] for m in mine) for g in gold)   # the two gold DEL lines except for the id
        assert "heterozygous                             : 2" in stdout
    assert sorted(os.listdir(str(tmp_path))) == ["found.breakpoints", "found.othervariants.vcf"]


def test_find_tool_insert_only_is_unchanged(mtg, golden, tmp_path):
    idx, solid, names, seqs, want, wst = golden
    homo, _ = fc.find_homo(solid, K, seqs, MAX_REPEAT)
    het, _ = fh.find_het(solid, K, seqs, None, MAX_REPEAT, BRANCHING)
    bk, vcf = fh.lines(fh.merge(homo, het), names, seqs, K)
    got_bk, got_vcf, stdout = run_tool(mtg, ["-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-abundance-min", str(CUTOFF), "-insert-only"], str(tmp_path / "found"))
    assert got_bk == bk and got_vcf == vcf
    assert "deletions" not in stdout and "deletion                                 : no" in stdout


@pytest.mark.parametrize("reads, reference", [("deleted.fasta", "ref_master.fasta"), ("deletionfuzzy.fasta", "ref_deletionfuzzy.fasta")])
def test_find_tool_on_the_micro_cases(mtg, tmp_path, reads, reference):
    reads, reference = os.path.join(GOLDEN, "micro", reads), os.path.join(GOLDEN, "micro", reference)
    ref = pc.read_fasta(reference)
    names, seqs = [n.split()[0] for n, _ in ref], [s for _, s in ref]
    solid = fc.solid_of_files([reads], K, 3)
    merged = fd.find_gap_family(solid, K, seqs, MAX_REPEAT, "-deletion-only")
    assert len(merged) == 1 and merged[0][2] == 4 and merged[0][6] == 20
    bk, vcf = fd.lines(merged, names, seqs, K)
    got_bk, got_vcf, stdout = run_tool(mtg, ["-in", reads, "-ref", reference, "-abundance-min", "3", "-deletion-only"], str(tmp_path / "found"))
    assert got_bk == bk == [] and got_vcf == vcf and "deletions                                : 1" in stdout


def tool_genome():
    """a genome for the tool through -graph: two deleted tandem copies that the site observers would call, a deletion in lower case, a deletion
    with a junction repeat and an insertion site of its own"""
    rng = np.random.default_rng(37)
    seqs, solid = [], set()
    for d, copies in ((2, 2), (4, 2)):
        seq, donor = fd.tandem_case(rng, d, copies, flank=150)
        seqs.append(seq)
        solid |= fc.solid_of_strings([donor], K)
    seq, donor = sequence_with_deletion(rng, 400, 130, 25, 0)
    seqs.append(seq[:125] + seq[125:160].lower() + seq[160:])
    solid |= fc.solid_of_strings([donor], K)
    seq, donor = sequence_with_deletion(rng, 500, 257, 70, 3)
    site = fc.with_repeat(rng, fc.rand_seq(rng, 40) + seq[300:], 120, 12, 0)        # the donor carries 12 nt more behind position 299 + 120
    seqs.append(seq[:300] + fc.planted(rng, site, K, [(120, 12)])[40:])
    solid |= fc.solid_of_strings([donor[:230] + site[40:]], K)
    return seqs, solid


def test_find_tool_on_a_genome_where_the_overlap_rule_drops_sites(mtg, tmp_path):
    seqs, solid = tool_genome()
    names = ["chr%d" % i for i in range(len(seqs))]
    dels, _ = fd.find_del(solid, K, seqs, MAX_REPEAT)
    homo, _ = fc.find_homo(solid, K, seqs, MAX_REPEAT)
    merged = fd.merge(homo, dels)
    assert merged == fd.find_gap_family(solid, K, seqs, MAX_REPEAT, "-homo-only -no-snp")
    assert len(dels) == 4 and len(homo) == 3 and len(merged) == 5 and [c[2] for c in merged] == [4, 4, 4, 4, 0]   # two sites dropped
    idx = index_of(mtg, solid, K)
    try:
        graph, genome = str(tmp_path / "g.mtg"), str(tmp_path / "genome.fa")
        idx.save(graph)
    finally:
        idx.close()
    with open(genome, "w") as f:
        for n_, x in zip(names, seqs):
            f.write(">%s\n%s\n" % (n_, "\n".join(x[i:i + 70] for i in range(0, len(x), 70))))
    bk, vcf = fd.lines(merged, names, seqs, K)
    got_bk, got_vcf, stdout = run_tool(mtg, ["-graph", graph, "-ref", genome, "-homo-only", "-no-snp"], str(tmp_path / "found"))
    assert got_bk == bk and got_vcf == vcf and len(bk) == 4
    assert "deletions                                : 4" in stdout and "homozygous                               : 1" in stdout
    ref_field = got_vcf[2].split("\t")[3]
    assert ref_field == seqs[2][129:155] and ref_field[1:] == ref_field[1:].lower() and ref_field[0] == ref_field[0].lower()   # REF keeps the case
    # without the deletion observer the sites are there: -homo-insertions is as it was
    got_bk2, got_vcf2, _ = run_tool(mtg, ["-graph", graph, "-ref", genome, "-homo-insertions"], str(tmp_path / "homo"))
    assert (got_bk2, got_vcf2) == fc.breakpoint_lines(homo, names, seqs, K) and len(got_bk2) == 12
