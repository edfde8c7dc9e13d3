"""`find` for isolated homozygous SNPs (include/mtg_fill.h: mtg_index_find_snp_sequences) without a GPU: the plain model
(tests/find_snp_cases.py) against the reference's golden records, the closed form of the rule against the literal map-and-erase loop, the
overlap with the deletion observer, the logic the kernels share with tests/emu/find_snp.cpp against literal loops (also under
AddressSanitizer + UBSan, as a program of its own), the exports, and the refusals.

Data fixture, copied from the reference's test data as it stands (results of its `find`, no program text):
tests/golden/full_test/gold.othervariants.snp.vcf holds the eleven `TYPE=SNP` record lines of test/full_test/gold.othervariants.vcf (made on
tests/golden/full_test/reference.fasta and the golden reads with every observer on)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import find_cases as fc
from tests import find_del_cases as fd
from tests import find_snp_cases as fs
from tests import profile_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HARNESS = os.path.join(ROOT, "tests", "emu", "find_snp.cpp")
FASTQ_PAIR = [os.path.join(G, "data", "reads_r1.fastq"), os.path.join(G, "data", "reads_r2.fastq")]
REFERENCE = os.path.join(G, "full_test", "reference.fasta")
K, CUTOFF, MAX_REPEAT = 31, 7, 5

# the model's solo calls on the golden reference: (name, POS, REF, ALT, start of the gap)
SOLO_ON_GOLDEN = [
    ("Seq0", 101, "T", "C", 70), ("Seq0", 816, "C", "A", 785), ("Seq2", 379, "G", "C", 348), ("Seq3", 256, "A", "T", 225),
    ("Seq3", 511, "C", "A", 480), ("Seq4", 257, "C", "T", 226), ("Seq4", 512, "A", "G", 481),
]
# the gold SNPs of gaps longer than k + 5: the multi observers', a later layer
MULTI_IN_GOLD = [("Seq2", 320), ("Seq2", 344), ("Seq3", 766), ("Seq4", 841)]


class AcgtScan(fs.SnpScan):
    """a wrong model: the map's keys in the order A, C, G, T"""
    CODES = "ACGT"


class NoStopScan(fs.SnpScan):
    """a wrong model: an alternative that misses a window stays in the map, and the best count need not reach the limit"""

    def snp_at_end(self, beginpos, limit):
        k = self.k
        ref = self.het_kmer_history(beginpos)[-1]
        for n, a in enumerate(self.CODES):
            if a != ref and sum(self.g.contains(self.mutate_kmer(self.het_kmer_history(beginpos + j), n, k - j)) for j in range(k)) >= k - 1:
                return True, beginpos + k, n, self.CODES.index(ref)
        return False, beginpos, None, self.CODES.index(ref)


@pytest.fixture(scope="module")
def golden():
    solid = fc.solid_of_files(FASTQ_PAIR, K, CUTOFF)
    ref = pc.read_fasta(REFERENCE)
    names, seqs = [n for n, _ in ref], [s for _, s in ref]
    calls, st = fs.find_snp(solid, K, seqs, MAX_REPEAT)
    return solid, names, seqs, calls, st


def test_model_on_the_golden_gives_the_seven_solo_snps(golden):
    solid, names, seqs, calls, st = golden
    assert [(names[c[0]], c[1] + 1, chr(c[6] >> 8), chr(c[6] & 255), c[4] + 1) for c in calls] == SOLO_ON_GOLDEN
    assert all(c[2] == 5 and c[3] == 0 and c[5] == c[4] + 1 + K and c[1] == c[4] + K for c in calls)
    assert st == {"n_gaps": 35, "n_candidates": 7, "n_calls": 7}
    # record for record against gold: name, POS, REF, ALT, TYPE, LEN, FUZZY, GT (ids aside)
    bk, vcf = fs.lines(calls, names, seqs, K)
    assert bk == []
    gold = fc.parse_vcf(open(os.path.join(G, "full_test", "gold.othervariants.snp.vcf")).read())
    assert len(gold) == 11 and all(r[4] == "SNP" and r[5] == 1 and r[6] == 0 and r[7] == "1/1" for r in gold)
    mine = fc.parse_vcf("\n".join(vcf))
    assert mine == [r for r in gold if (r[0], r[1]) not in MULTI_IN_GOLD] and len(mine) == 7
    assert vcf[0] == "Seq0\t101\tbkpt1\tT\tC\t.\tPASS\tTYPE=SNP;LEN=1;FUZZY=0\tGT\t1/1"
    # the literal loop over the literal gaps says the same, and one gap of k has no kmer_begin
    gaps = fc.literal_gaps(solid, K, seqs)
    assert [(names[s], p) for s, p, n, fresh in gaps if n == K and fresh] == [(c[0], c[4]) for c in SOLO_ON_GOLDEN]
    assert [(names[s], p) for s, p, n, fresh in gaps if n == K and not fresh] == [("Seq2", 0)]
    # the four other gold SNPs lie in gaps longer than k + 5
    for name, pos in MULTI_IN_GOLD:
        inside = [n for s, p, n, fresh in gaps if names[s] == name and p <= pos - 1 - (K - 1) and pos - 1 < p + n]
        assert len(inside) == 1 and inside[0] > K + 5, (name, pos, inside)


def test_insertions_and_deletions_of_the_golden_are_unchanged_in_the_family(golden):
    solid, names, seqs, calls, st = golden
    homo, _ = fc.find_homo(solid, K, seqs, MAX_REPEAT)
    dels, _ = fd.find_del(solid, K, seqs, MAX_REPEAT)
    family = fs.find_gap_family(solid, K, seqs, MAX_REPEAT, "-homo-only -solo-snps")
    assert len(homo) == 13 and len(dels) == 3
    assert [c for c in family if c[2] in (0, 1)] == homo and [c for c in family if c[2] == 4] == dels and [c for c in family if c[2] == 5] == calls
    assert fs.merge(homo, dels, calls) == family and fs.find_gap_family(solid, K, seqs, MAX_REPEAT, "-solo-snps") == calls
    assert fs.find_gap_family(solid, K, seqs, MAX_REPEAT, "-homo-only -no-snp") == fd.find_gap_family(solid, K, seqs, MAX_REPEAT, "-homo-only -no-snp")


# ---------------------------------------------------------------------------------------------------------------- the closed form
def competing_case_on(ref, k, hold, hole):
    """(reference of 4k nt, start of the gap, solid set): position g = 2k is a SNP; the set holds the flanks and all k windows of every
    alternative in `hold`; hole = (alternative, window): that window is taken out again (it stays absent only if no other text holds the
    same k-mer: the model decides)"""
    g = 2 * k
    start = g - k + 1
    solid = fc.solid_of_strings([ref[:start + k - 1], ref[g + 1:]], k)   # the flanks: anchors on both sides, the gap's own k-mers absent
    for a in hold:
        solid |= fc.solid_of_strings([fs.substituted(ref, g, a)[start:g + k]], k)
    if hole is not None:
        a, j = hole
        solid.discard(fc.canon_of(fs.substituted(ref, g, a)[start + j:start + j + k]))
    return ref, start, solid


@pytest.mark.parametrize("k", [5, 7])
def test_closed_form_equals_the_literal_loop(k):
    """random solid sets at small k, where the windows of several alternatives hold often and by chance: the call of the literal
    snp_at_end is the first alternative in A, C, T, G order whose k windows are all in the graph.  Both wrong models fail here"""
    rng = np.random.default_rng(7100 + k)
    seen = {"two_hold": 0, "t_before_g": 0, "hole_0": 0, "hole_last": 0, "hole_middle": 0, "none": 0}
    acgt_differs = nostop_differs = 0
    for t in range(400):
        n_hold = int(rng.integers(0, 4))
        ref = fc.rand_seq(rng, 4 * k)
        alts = [a for a in "ACTG" if a != ref[2 * k]]
        hold = [alts[i] for i in sorted(rng.choice(3, n_hold, replace=False))]
        hole = None
        if hold and t % 2:
            hole = (hold[int(rng.integers(len(hold)))], (0, k - 1, 1 + int(rng.integers(k - 2)))[t // 2 % 3])
        ref, start, solid = competing_case_on(ref, k, hold, hole)
        graph = fc.Graph(solid, k)
        calls, st = fs.find_snp(solid, k, [ref])
        mine = [c for c in calls if c[4] == start - 1]
        want = fs.closed_form(graph, ref, start, k)
        gaps = [x for x in fc.literal_gaps(solid, k, [ref]) if x[1] == start and x[2] == k and x[3]]
        if not gaps:
            assert mine == []   # chance k-mers changed the gap: no candidate at this start
            continue
        assert [chr(c[6] & 255) for c in mine] == ([want] if want else []), (t, hold, hole)
        assert all(c[1] == start + k - 1 and chr(c[6] >> 8) == ref[start + k - 1] for c in mine)
        holding = [a for a in "ACTG" if a != ref[2 * k] and fs.closed_form(graph, ref, start, k, order=a) == a]
        seen["two_hold"] += len(holding) >= 2
        seen["t_before_g"] += "T" in holding and "G" in holding and want == "T"
        seen["none"] += not holding
        if hole and hole[0] not in holding:
            seen["hole_0" if hole[1] == 0 else "hole_last" if hole[1] == k - 1 else "hole_middle"] += 1
            assert want != hole[0]
        acgt = [chr(c[6] & 255) for c in fs.find_snp(solid, k, [ref], cls=AcgtScan)[0] if c[4] == start - 1]
        acgt_differs += acgt != ([want] if want else [])
        nostop = [chr(c[6] & 255) for c in fs.find_snp(solid, k, [ref], cls=NoStopScan)[0] if c[4] == start - 1]
        nostop_differs += nostop != ([want] if want else [])
    assert all(v >= 5 for v in seen.values()), seen
    assert acgt_differs >= 5 and nostop_differs >= 5   # a model in A, C, G, T order, or one that does not stop at a missing window, is told apart


@pytest.mark.parametrize("k", [31, 13])
def test_named_cases_of_order_and_missing_windows(k):
    """at k = 31 and 13 chance plays no part: two alternatives hold, the first in A, C, T, G order wins; T and G hold, T wins (the wrong
    order says G); an alternative that lacks window 0, window k - 1 or a middle window is not called, and the next one that holds is"""
    rng = np.random.default_rng(7200 + k)
    ref = fc.rand_seq(rng, 4 * k)
    g = 2 * k
    ref = fs.substituted(ref, g, "A")
    call = lambda hold, hole=None, cls=fs.SnpScan: [chr(c[6] & 255) for c in fs.find_snp(competing_case_on(ref, k, hold, hole)[2], k, [ref], cls=cls)[0]]  # noqa: E731
    assert call("C") == ["C"] and call("T") == ["T"] and call("G") == ["G"] and call("") == []
    assert call("CT") == ["C"] and call("CG") == ["C"] and call("CTG") == ["C"]
    assert call("TG") == ["T"] and call("TG", cls=AcgtScan) == ["G"]
    for j in (0, k - 1, k // 2):
        assert call("C", ("C", j)) == [] and call("CT", ("C", j)) == ["T"] and call("TG", ("T", j)) == ["G"] and call("CTG", ("T", j)) == ["C"]
        assert call("C", ("C", j), cls=NoStopScan) == ["C"]
    for r, alts in (("C", "ATG"), ("T", "ACG"), ("G", "ACT")):
        ref2 = fs.substituted(ref, g, r)
        for i, a in enumerate(alts):
            got = fs.find_snp(competing_case_on(ref2, k, alts[i:], None)[2], k, [ref2])[0]
            assert [(c[1], chr(c[6] >> 8), chr(c[6] & 255)) for c in got] == [(g, r, a)]


# ---------------------------------------------------------------------------------------------------------------- the overlap with deletion
def test_a_gap_of_k_goes_to_the_solo_observer_before_the_deletion_observer():
    """the solid set holds a donor with a SNP at g and a donor with ref[g] deleted: one gap of 31, which the deletion observer alone calls
    with del_size 1 and the solo observer with the SNP; the family reports the SNP and no deletion.  With the deletion donor alone it is
    the deletion"""
    rng = np.random.default_rng(7300)
    for g in (150, 161, 200):
        ref, snp_donor, del_donor, alt = fs.overlap_case(rng, 400, g)
        both = fc.solid_of_strings([snp_donor, del_donor], K)
        gaps = [x for x in fc.literal_gaps(both, K, [ref]) if x[3]]
        assert gaps == [(0, g - K + 1, K, True)]
        dels, _ = fd.find_del(both, K, [ref], MAX_REPEAT)
        assert dels == [(0, g - 1, 4, 0, g - K, g + 1, 1)]
        snps, st = fs.find_snp(both, K, [ref], MAX_REPEAT)
        assert snps == [(0, g, 5, 0, g - K, g + 1, ord(alt) | ord(ref[g]) << 8)] and st["n_candidates"] == 1
        homo, _ = fc.find_homo(both, K, [ref], MAX_REPEAT)
        family = fs.find_gap_family(both, K, [ref], MAX_REPEAT, "-homo-only -solo-snps")
        assert family == snps == fs.merge(homo, dels, snps)
        only_del = fc.solid_of_strings([del_donor], K)
        assert fs.find_gap_family(only_del, K, [ref], MAX_REPEAT, "-homo-only -solo-snps") == dels
        assert fs.find_snp(only_del, K, [ref])[0] == [] and fs.merge([], dels, []) == dels


def test_merge_and_lines():
    snp, dele, hom = (0, 60, 5, 0, 29, 61, ord("C") | ord("T") << 8), (0, 59, 4, 0, 29, 61, 1), (0, 90, 0, 0, 60, 91, 0)
    assert fs.detected_at(snp) == (0, 62, 1) and fs.merge([hom], [dele], [snp]) == [snp, hom]
    assert fs.merge([hom], [(1, 59, 4, 0, 29, 61, 1)], [snp]) == [snp, hom, (1, 59, 4, 0, 29, 61, 1)]
    seq = "acgt" * 40
    assert fs.lines([snp], ["chr"], [seq], K) == ([], ["chr\t61\tbkpt1\tT\tC\t.\tPASS\tTYPE=SNP;LEN=1;FUZZY=0\tGT\t1/1"])   # upper case whatever the text's case


# ---------------------------------------------------------------------------------------------------------------- the product without a GPU
def test_product_exports_the_snp_entries():
    import mindthegap_amd
    lib = C.CDLL(mindthegap_amd.build_library())
    for name in ("mtg_index_find_snp_sequences", "mtg_index_find_snp_packed_device"):
        assert hasattr(lib, name), "missing export: " + name
    assert hasattr(mindthegap_amd.Index, "find_snp_sequences") and hasattr(mindthegap_amd.Index, "find_snp_packed_device")
    from mindthegap_amd import lib as L
    assert C.sizeof(L.FindSnpStats) == 64 == C.sizeof(L.FindDelStats)
    assert [f[0] for f in L.FindSnpStats._fields_][:5] == ["n_positions", "n_gaps", "n_candidates", "n_calls", "kernel_ms"]
    hdr = open(os.path.join(ROOT, "include", "mtg_fill.h")).read()
    assert "typedef struct mtg_find_snp_stats {" in hdr and "uint64_t reserved[3];" in hdr


def test_bad_arguments_are_refused_before_anything_else():
    import mindthegap_amd
    from mindthegap_amd import lib as L
    L._lib = None
    lib = mindthegap_amd.load_library()
    n = C.c_size_t()
    assert lib.mtg_index_find_snp_sequences(None, None, 0, 5, None, 0, C.byref(n), None) == 2  # MTG_ERR_ARG: no index
    assert lib.mtg_index_find_snp_packed_device(None, None, None, None, 0, 5, None, 0, C.byref(n), None) == 2


def test_find_tool_refusals(tmp_path):
    import mindthegap_amd
    exe = os.path.join(os.path.dirname(mindthegap_amd.build_library()), "MindTheGap")
    out = str(tmp_path / "f")
    base = [exe, "find", "-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-out", out]
    for extra in (["-solo-snps", "-hete-only"], ["-solo-snps", "-insert-only"], ["-solo-snps", "-no-snp"], ["-homo-only", "-solo-snps", "-no-snp"], ["-solo-snps", "-deletion-only"],
                  ["-solo-snps", "-homo-insertions"], ["-solo-snps", "-snp-only"], ["-solo-snps", "-max-rep", "-1"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "EXCEPTION" in r.stderr and os.listdir(str(tmp_path)) == [], extra
        if "-max-rep" not in extra:
            assert "-solo-snps" in r.stderr and "heterozygous observer" in r.stderr and "not an option of the reference" in r.stderr
    # what was refused before is refused with the message it had
    for extra in (["-snp-only"], ["-homo-only"], ["-no-snp", "-homo-only", "-hete-only"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "SNPs and -bed are not built" in r.stderr and "heterozygous observer" not in r.stderr
    r = subprocess.run([exe, "find", "-help"], capture_output=True, text=True)
    assert "-solo-snps | -homo-only -solo-snps" in r.stderr


def test_host_code_without_the_device_unit_says_so(tmp_path):
    """the product's host code linked against the emulated backend has no device code for find: the entry answers MTG_ERR_NO_DEVICE through the
    weak stand-in, after the argument checks, and the tool writes nothing"""
    from tests import emu_lib
    m = emu_lib.product_on_emulator()
    try:
        lib = C.CDLL(emu_lib.FULL_SO)
        n = C.c_size_t()
        kms = np.array(sorted(fc.solid_of_strings(["ACGTTGCAAGGCTTAACCGGATGCAT"], 11)), dtype=np.uint64)
        idx = m.Index.from_kmers(kms, np.full(len(kms), 9, dtype=np.uint32), 11)
        try:
            arr = (C.c_char_p * 1)(b"ACGTTGCAAGGCTTAACCGGATGCAT")
            lib.mtg_index_find_snp_sequences.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
            assert lib.mtg_index_find_snp_sequences(idx.h, arr, 1, 5, None, 0, C.byref(n), None) == 1   # MTG_ERR_NO_DEVICE
            assert lib.mtg_index_find_snp_sequences(idx.h, arr, 1, -1, None, 0, C.byref(n), None) == 2  # the argument checks come first
            assert lib.mtg_index_find_snp_sequences(idx.h, None, 1, 5, None, 0, C.byref(n), None) == 2
        finally:
            idx.close()
        out = str(tmp_path / "f")
        for flags in (["-solo-snps"], ["-homo-only", "-solo-snps"]):
            assert m.find_main(["-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE] + flags + ["-abundance-min", str(CUTOFF), "-out", out]) == 1
            assert os.listdir(str(tmp_path)) == []
    finally:
        from mindthegap_amd import lib as L
        L._lib = None


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-g", "-std=c++17", "-Wall"] + flags + ["-o", exe, HARNESS])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stderr == ""  # UBSan reports on stderr and goes on
    return r.stdout


def test_windows_closed_form_and_candidates_equal_the_literal_loops(tmp_path):
    """mtg_find_snp.h by g++: every window of every gap start against the word seams of a packed sequence, the closed form against the
    literal snp_at_end, the candidate test and the record's fields"""
    out = _build_and_run(tmp_path, "find_snp", ["-O2"]).split()
    assert int(out[1]) > 200000 and int(out[3]) >= 18000 and int(out[5]) > 100000


def test_windows_closed_form_and_candidates_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "find_snp_san", ["-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
