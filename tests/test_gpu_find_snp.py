"""`find` for isolated homozygous SNPs on the device (k_gap_mark<SoloObserver>, k_snp_judge, k_gap_emit<SoloObserver> in
csrc/mtg_gpu_misc.hip behind mtg_index_find_snp_sequences / _packed_device and `MindTheGap find -solo-snps | -homo-only -solo-snps`) against
the plain model of tests/find_snp_cases.py: the literal FindSoloSNP::update with the literal snp_at_end inside the literal loop of the scan.
Every comparison is exact, calls and statistics, through both entries.

The synthetic cases index the k-mers of donors, each donor a sequence with one nucleotide substituted (a homozygous SNP: the graph does not
know the sequence's own allele), or a set of k-mers with windows of chosen alternatives added or removed."""
import os
import subprocess

import numpy as np
import pytest

from tests import find_cases as fc
from tests import find_del_cases as fd
from tests import find_het_cases as fh
from tests import find_snp_cases as fs
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
    want, wst = fs.find_snp(solid, K, seqs, MAX_REPEAT)
    assert len(want) == 7  # tests/test_find_snp_cpu.py holds the list itself
    idx = mtg.Index.from_reads(FASTQ_PAIR, K, CUTOFF)
    yield idx, solid, names, seqs, want, wst
    idx.close()


def index_of(mtg, solid, k):
    kms = np.array(sorted(solid), dtype=np.uint64)
    return mtg.Index.from_kmers(kms, np.full(len(kms), 9, dtype=np.uint32), k)


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


def packed_device_calls(idx, seqs, max_repeat, cap):
    import torch
    packed, word_off, lens = pack(seqs)
    dev = torch.device("cuda", 0)
    d_w = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_wo = torch.from_numpy(word_off.view(np.int64)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_calls = torch.full((max(cap, 1) * 7 + 7,), -1, dtype=torch.int32, device=dev)
    total, st = idx.find_snp_packed_device(d_w.data_ptr(), d_wo.data_ptr(), d_ln.data_ptr(), len(seqs), max_repeat, d_calls.data_ptr() if cap else None, cap)
    torch.cuda.synchronize()
    raw = d_calls.cpu().numpy().view(np.uint32)
    n = min(total, cap)
    assert (raw[7 * n:] == 0xFFFFFFFF).all()  # nothing behind the calls that were asked for
    return total, tuples(raw[:7 * n].view(fc.CALL_DTYPE)), st


def check(idx, solid, k, seqs, packed=True):
    """find on the device against the model: calls and statistics, by the string entry and (for sequences without N) the packed device
    entry; returns (calls as tuples, statistics of the model)"""
    calls, st = idx.find_snp_sequences(seqs, MAX_REPEAT)
    want, wst = fs.find_snp(solid, k, seqs, MAX_REPEAT)
    got = tuples(calls)
    assert calls.dtype == fc.CALL_DTYPE
    diff = [i for i in range(min(len(got), len(want))) if got[i] != want[i]]
    assert not diff and len(got) == len(want), "%d calls, expected %d; first difference: %r, expected %r" % (
        len(got), len(want), got[diff[0]] if diff else got[len(want):][:1], want[diff[0]] if diff else want[len(got):][:1])
    assert {x: st[x] for x in fs.STAT_KEYS} == wst
    assert st["n_positions"] == sum(max(len(s) - k + 1, 0) for s in seqs)
    if packed:
        total, dev, std = packed_device_calls(idx, seqs, MAX_REPEAT, len(want) + 2)
        assert total == len(want) and dev == want and {x: std[x] for x in fs.STAT_KEYS} == wst
    return got, wst


# ------------------------------------------------------------------------------------------------ 1. the reference's goldens
def test_golden_calls_by_both_entries(mtg, golden):
    idx, solid, names, seqs, want, wst = golden
    calls, st = idx.find_snp_sequences(seqs, MAX_REPEAT)
    assert tuples(calls) == want and {x: st[x] for x in fs.STAT_KEYS} == wst and st["n_calls"] == 7 and st["n_candidates"] == 7
    assert st["n_positions"] == sum(max(len(s) - K + 1, 0) for s in seqs)
    for cap in (9, 7, 3, 0):
        total, got, st2 = packed_device_calls(idx, seqs, MAX_REPEAT, cap)
        assert total == 7 and got == want[:cap] and {x: st2[x] for x in fs.STAT_KEYS} == wst
        calls, st3 = idx.find_snp_sequences(seqs, MAX_REPEAT, cap=cap)
        assert st3["n_calls"] == 7 and tuples(calls) == want[:cap]
    with pytest.raises(mtg.MtgError):
        idx.find_snp_sequences(seqs, -1)
    assert tuples(idx.find_snp_sequences(seqs, 0)[0]) == want == tuples(idx.find_snp_sequences(seqs, 1000)[0])   # max_repeat plays no part
    calls, st0 = idx.find_snp_sequences([])  # nseq = 0
    assert len(calls) == 0 and all(st0[x] == 0 for x in fs.STAT_KEYS) and st0["n_positions"] == 0


# ------------------------------------------------------------------------------------------------ 2. planted SNPs
def planted_cases(k):
    """one SNP per sequence of 2k + 120 .. 2k + 200 nt: the gap's start k-mer position slid over 64 + 33 values from 60 on (every start
    mod 32, the word seams at 64 and 96, the plane-word seams at 64 and 128), the twelve REF -> ALT pairs in turn, every other donor given
    as its reverse complement"""
    rng = np.random.default_rng(8100 + k)
    seqs, solid, pairs = [], set(), []
    all_pairs = [(r, a) for r in "ACGT" for a in "ACGT" if a != r]
    for i, start in enumerate(range(60, 60 + 97)):
        g = start + k - 1
        ref_nt, alt = all_pairs[i % 12]
        seq = fs.substituted(fc.rand_seq(rng, g + k + 40 + int(rng.integers(0, 80))), g, ref_nt)
        donor = fs.substituted(seq, g, alt)
        seqs.append(seq)
        solid |= fc.solid_of_strings([fs.revcomp(donor) if i % 2 else donor], k)
        pairs.append((g, ref_nt, alt))
    return seqs, solid, pairs


@pytest.mark.parametrize("k", [31, 13])
def test_planted_snps_at_every_alignment(mtg, k):
    seqs, solid, pairs = planted_cases(k)
    idx = index_of(mtg, solid, k)
    try:
        got, st = check(idx, solid, k, seqs)
        # every planted SNP whose gap is exactly k (a chance k-mer can shorten or split a gap at k = 13: the model decides) is called as planted
        by_seq = {c[0]: c for c in got}
        assert len(got) >= (97 if k == 31 else 90)
        for s, c in by_seq.items():
            g, ref_nt, alt = pairs[s]
            assert c == (s, g, 5, 0, g - k, g + 1, ord(alt) | ord(ref_nt) << 8)
        assert {(chr(c[6] >> 8), chr(c[6] & 255)) for c in got} == {(r, a) for r in "ACGT" for a in "ACGT" if a != r}
        assert {(c[4] + 1) % 32 for c in got} == set(range(32)) and {(c[4] + 1) // 64 for c in got} >= {0, 1, 2}
        n = len(got)
        for cap in (0, 1, n - 1, n, n + 3):  # capacity: the count is the total, the leading records are the same
            calls, stc = idx.find_snp_sequences(seqs, MAX_REPEAT, cap=cap)
            assert stc["n_calls"] == n and tuples(calls) == got[:cap]
            total, dev, std = packed_device_calls(idx, seqs, MAX_REPEAT, cap)
            assert total == n and dev == got[:cap]
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 3. competing alternatives, missing windows
def competing_set(ref, k, g, hold, hole):
    """the flanks of position g of ref and all k windows of every alternative in `hold`; hole = (alternative, window): taken out again"""
    start = g - k + 1
    solid = fc.solid_of_strings([ref[:start + k - 1], ref[g + 1:]], k)
    for a in hold:
        solid |= fc.solid_of_strings([fs.substituted(ref, g, a)[start:g + k]], k)
    if hole is not None:
        solid.discard(fc.canon_of(fs.substituted(ref, g, hole[0])[start + hole[1]:start + hole[1] + k]))
    return solid


@pytest.mark.parametrize("k", [31, 13])
def test_competing_alternatives_and_missing_windows(mtg, k):
    """two or three alternatives hold all k windows: the first in A, C, T, G order is called -- T before G; an alternative that lacks
    window 0, window k - 1 or a middle window is not called and the next that holds is.  One index per case, a few hundred k-mers each"""
    rng = np.random.default_rng(8200 + k)
    g = 2 * k + 17
    base = fc.rand_seq(rng, 4 * k + 30)
    cases = []
    for r in "ACTG":
        alts = [a for a in "ACTG" if a != r]
        for hold in ("".join(alts), alts[0] + alts[1], alts[1] + alts[2], alts[0] + alts[2], alts[2], ""):
            cases.append((r, hold, None))
        for j in (0, k - 1, k // 2, 1, k - 2):
            cases += [(r, alts[0], (alts[0], j)), (r, alts[0] + alts[1], (alts[0], j)), (r, "".join(alts), (alts[1], j)), (r, alts[1] + alts[2], (alts[1], j))]
        cases.append((r, "".join(alts), (alts[0], k // 3)))
    seen = set()
    for r, hold, hole in cases:
        ref = fs.substituted(base, g, r)
        solid = competing_set(ref, k, g, hold, hole)
        idx = index_of(mtg, solid, k)
        try:
            got, st = check(idx, solid, k, [ref])
        finally:
            idx.close()
        left = [a for a in "ACTG" if a in hold and not (hole and hole[0] == a)]
        assert [chr(c[6] & 255) for c in got] == left[:1] and st["n_candidates"] == 1, (r, hold, hole)   # what the rule says, stated apart from the model
        seen.add((tuple(left[:2]), hole is not None))
    assert (("T", "G"), False) in seen and (("T", "G"), True) in seen and (("C", "T"), False) in seen


# ------------------------------------------------------------------------------------------------ 4. edges
def edge_cases(k):
    rng = np.random.default_rng(8300 + k)
    g = 200
    base = fc.rand_seq(rng, 420)
    alt = fs.other(rng, base[g])
    donor = fs.substituted(base, g, alt)
    solid = fc.solid_of_strings([donor], k)
    put = lambda t, i, ch="N": t[:i] + ch + t[i + 1:]  # noqa: E731
    s = {"plain": base}
    s["lower_all"] = base.lower()
    s["lower_snp"] = base[:g] + base[g].lower() + base[g + 1:]
    s["near_start"] = base[g - k + 2:]            # the SNP at k - 2: no position before the gap
    s["start_plus_one"] = base[g - k:]            # one solid position before the gap: no anchor
    s["start_plus_two"] = base[g - k - 1:]        # two: the first gap with a left anchor
    s["n_before"] = put(base, g - k - 1)          # the N leaves one valid position before the gap
    s["n_further_before"] = put(base, g - k - 2)  # two
    s["lower_n_before"] = put(base, g - k - 1, "n")
    s["n_in_gap"] = put(base, g + 3)
    s["end_one_solid"] = base[:g + k + 1]         # one solid position follows the gap: the observers are never called
    s["end_two_solid"] = base[:g + k + 2]
    s["end_in_gap"] = base[:g + k]
    # an isolated present position inside the gap is counted into it: the gap is still k long and is judged.  Another sequence, whose own
    # k-mer at the gap's fifth position is in the graph
    base2 = fc.rand_seq(rng, 420)
    alt2 = fs.other(rng, base2[g])
    solid |= fc.solid_of_strings([fs.substituted(base2, g, alt2)], k)
    solid.add(fc.canon_of(base2[g - k + 5:g + 5]))
    s["isolated_inside"] = base2
    return s, solid, g, base[g], alt, base2[g], alt2


@pytest.mark.parametrize("k", [31, 13])
def test_edges_of_sequences_invalid_characters_and_case(mtg, k):
    s, solid, g, ref_nt, alt, ref2, alt2 = edge_cases(k)
    tags = list(s)
    seqs = [s[t] for t in tags]
    idx = index_of(mtg, solid, k)
    try:
        got, st = check(idx, solid, k, seqs, packed=False)   # N is not part of the packed alphabet
        of = lambda tag: [c[1:] for c in got if c[0] == tags.index(tag)]  # noqa: E731
        ins = ord(alt) | ord(ref_nt) << 8   # upper case
        call = [(g, 5, 0, g - k, g + 1, ins)]
        for tag in ("plain", "lower_all", "lower_snp", "n_further_before", "end_two_solid"):
            assert of(tag) == call, tag
        for tag in ("near_start", "start_plus_one", "n_before", "lower_n_before", "n_in_gap", "end_one_solid", "end_in_gap"):
            assert of(tag) == [], tag
        assert of("start_plus_two") == [(k + 1, 5, 0, 1, k + 2, ins)]
        assert of("isolated_inside") == [(g, 5, 0, g - k, g + 1, ord(alt2) | ord(ref2) << 8)]
        clean = [x for x in seqs if "N" not in x.upper()]
        check(idx, solid, k, clean)   # the same without N through the packed device entry too
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 5. many short sequences, none, no gap
def test_many_short_sequences_no_sequence_and_no_gap(mtg):
    """300 sequences of 0 .. 160 nt around one SNP, slid so that it meets both ends and the word seams, among sequences shorter than k and
    sequences without the SNP: the candidates cross waves and workgroups of the judging kernel"""
    rng = np.random.default_rng(8400)
    g = 200
    ref = fc.rand_seq(rng, 400)
    donor = fs.substituted(ref, g, fs.other(rng, ref[g]))
    solid = fc.solid_of_strings([donor], K)
    seqs = []
    for i in range(300):
        if i % 10 == 9:
            seqs.append(ref[:(i // 10) % K])
        elif i % 10 == 8:
            seqs.append(donor[g - 60:g + 60])   # no gap at all
        else:
            seqs.append(ref[max(g - K - 1 - (i % 60), 0):g + K + (i % 7) - 1])
    assert max(len(x) for x in seqs) <= 160 and min(len(x) for x in seqs) == 0
    idx = index_of(mtg, solid, K)
    try:
        got, st = check(idx, solid, K, seqs)
        assert 120 < len(got) < 200 and st["n_candidates"] == len(got) < st["n_gaps"] + 1 and len(set(c[1] for c in got)) > 40 and {c[4] < 31 for c in got} == {True, False}
        total, dev, std = packed_device_calls(idx, seqs, MAX_REPEAT, 100)
        assert total == len(got) and dev == got[:100]
        got0, st0 = check(idx, solid, K, [donor, donor[50:300]])   # no gap
        assert got0 == [] and st0 == {"n_gaps": 0, "n_candidates": 0, "n_calls": 0}
        total, dev, std = packed_device_calls(idx, [], MAX_REPEAT, 4)   # no sequence
        assert total == 0 and dev == [] and all(std[x] == 0 for x in fs.STAT_KEYS)
    finally:
        idx.close()


# ------------------------------------------------------------------------------------------------ 6. the overlap and the tool
def run_tool(mtg, args, out):
    exe = os.path.join(os.path.dirname(mtg.build_library()), "MindTheGap")
    r = subprocess.run([exe, "find"] + args + ["-out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    vcf = open(out + ".othervariants.vcf").read().splitlines()
    assert vcf[9] == VCF_COLUMNS
    return open(out + ".breakpoints").read().splitlines(), vcf[10:], r.stdout


@pytest.mark.parametrize("flags", [["-solo-snps"], ["-homo-only", "-solo-snps"]])
def test_find_tool_on_the_golden(mtg, golden, tmp_path, flags):
    idx, solid, names, seqs, want, wst = golden
    family = fs.find_gap_family(solid, K, seqs, MAX_REPEAT, " ".join(flags))   # one literal scan with all gap observers of the configuration
    if "-homo-only" in flags:
        assert family == fs.merge(fc.find_homo(solid, K, seqs, MAX_REPEAT)[0], fd.find_del(solid, K, seqs, MAX_REPEAT)[0], want) and len(family) == 23
    else:
        assert family == want
    bk, vcf = fs.lines(family, names, seqs, K)
    got_bk, got_vcf, stdout = run_tool(mtg, ["-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-abundance-min", str(CUTOFF)] + flags, str(tmp_path / "found"))
    assert got_bk == bk and got_vcf == vcf
    assert "SNPs                                     : 7" in stdout and "snp                                      : isolated only" in stdout
    assert ("deletion                                 : " + ("yes" if "-homo-only" in flags else "no")) in stdout and "hete_insertions                          : no" in stdout
    assert ("deletions                                : 3" in stdout) == ("-homo-only" in flags)
    assert ("homozygous                               : %d" % sum(c[2] == 0 for c in family)) in stdout
    assert ("Homozygous insertions 1-2 bp size        : %d" % sum(c[2] == 1 for c in family)) in stdout
    gold = [l.split("\t") for l in open(os.path.join(GOLDEN, "full_test", "gold.othervariants.snp.vcf")).read().splitlines()]
    mine = [l.split("\t") for l in got_vcf if "TYPE=SNP" in l]
    assert len(mine) == 7 and all(any(g[:2] + g[3:] == m[:2] + m[3:] for g in gold) for m in mine)   # seven of the eleven gold SNP lines except for the id
    assert sorted(os.listdir(str(tmp_path))) == ["found.breakpoints", "found.othervariants.vcf"]


def test_find_tool_insert_only_and_no_snp_are_unchanged(mtg, golden, tmp_path):
    idx, solid, names, seqs, want, wst = golden
    homo, _ = fc.find_homo(solid, K, seqs, MAX_REPEAT)
    het, _ = fh.find_het(solid, K, seqs, None, MAX_REPEAT, BRANCHING)
    dels, _ = fd.find_del(solid, K, seqs, MAX_REPEAT)
    args = ["-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-abundance-min", str(CUTOFF)]
    got_bk, got_vcf, stdout = run_tool(mtg, args + ["-insert-only"], str(tmp_path / "ins"))
    assert (got_bk, got_vcf) == fh.lines(fh.merge(homo, het), names, seqs, K) and "SNPs" not in stdout and "snp                                      : no" in stdout
    got_bk, got_vcf, stdout = run_tool(mtg, args + ["-no-snp"], str(tmp_path / "nosnp"))
    assert (got_bk, got_vcf) == fd.lines(fd.merge(homo, dels, het), names, seqs, K) and "SNPs" not in stdout and "TYPE=SNP" not in "\n".join(got_vcf)


def test_find_tool_gives_the_snp_and_not_the_deletion_on_a_gap_both_would_call(mtg, tmp_path):
    rng = np.random.default_rng(8500)
    g = 161
    ref, snp_donor, del_donor, alt = fs.overlap_case(rng, 400, g)
    plain = fc.rand_seq(rng, 300)
    seqs, names = [plain, ref.lower()], ["chr0", "chr1"]
    solid = fc.solid_of_strings([snp_donor, del_donor, plain], K)
    assert fd.find_del(solid, K, seqs, MAX_REPEAT)[0] == [(1, g - 1, 4, 0, g - K, g + 1, 1)]
    snp = (1, g, 5, 0, g - K, g + 1, ord(alt) | ord(ref[g]) << 8)
    assert fs.find_gap_family(solid, K, seqs, MAX_REPEAT, "-homo-only -solo-snps") == [snp]
    idx = index_of(mtg, solid, K)
    try:
        check(idx, solid, K, seqs)
        graph, genome = str(tmp_path / "g.mtg"), str(tmp_path / "genome.fa")
        idx.save(graph)
    finally:
        idx.close()
    with open(genome, "w") as f:
        for n_, x in zip(names, seqs):
            f.write(">%s\n%s\n" % (n_, "\n".join(x[i:i + 70] for i in range(0, len(x), 70))))
    got_bk, got_vcf, stdout = run_tool(mtg, ["-graph", graph, "-ref", genome, "-homo-only", "-solo-snps"], str(tmp_path / "both"))
    assert got_bk == [] and got_vcf == ["chr1\t%d\tbkpt1\t%s\t%s\t.\tPASS\tTYPE=SNP;LEN=1;FUZZY=0\tGT\t1/1" % (g + 1, ref[g], alt)]   # upper case from lower-case text
    assert "SNPs                                     : 1" in stdout and "deletions                                : 0" in stdout
    got_bk, got_vcf, stdout = run_tool(mtg, ["-graph", graph, "-ref", genome, "-homo-only", "-no-snp"], str(tmp_path / "del"))
    assert got_bk == [] and len(got_vcf) == 1 and "TYPE=DEL;LEN=1;FUZZY=0" in got_vcf[0] and "TYPE=SNP" not in got_vcf[0]
    assert got_vcf == fd.lines(fd.find_del(solid, K, seqs, MAX_REPEAT)[0], names, seqs, K)[1]
