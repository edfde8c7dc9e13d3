"""`find` for homozygous deletions (include/mtg_fill.h: mtg_index_find_del_sequences) without a GPU: the plain model (tests/find_del_cases.py)
against the reference's golden records and its two deletion micro-cases, hand-made cases at k = 5, the overlap with the insertion observers,
the logic the kernels share with tests/emu/find_del.cpp against literal loops (also under AddressSanitizer + UBSan, as a program of its own),
the exports, and the refusals.

Data fixtures, copied from the reference's test data as they stand (results and inputs of its `find`, no program text):
tests/golden/full_test/gold.othervariants.del.vcf holds the two `TYPE=DEL` record lines of test/full_test/gold.othervariants.vcf (made on
tests/golden/full_test/reference.fasta and the golden reads with every observer on); tests/golden/full_test/variants.txt is
test/full_test/variants.txt, the simulation's own list of what was planted; tests/golden/micro/ref_master.fasta, deletionfuzzy.fasta and
ref_deletionfuzzy.fasta are test/references/master.fasta, test/reads/deletionfuzzy.fasta and test/references/deletionfuzzy.fasta, the inputs
of the cases "deletion" and "fuzzy-deletion" of test/simple_test.sh:94-99 (their truth files are empty and pin nothing)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import find_cases as fc
from tests import find_del_cases as fd
from tests import profile_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HARNESS = os.path.join(ROOT, "tests", "emu", "find_del.cpp")
FASTQ_PAIR = [os.path.join(G, "data", "reads_r1.fastq"), os.path.join(G, "data", "reads_r2.fastq")]
REFERENCE = os.path.join(G, "full_test", "reference.fasta")
K, CUTOFF, MAX_REPEAT = 31, 7, 5

# the model's deletions on the golden reference, (name, pos 0-based, kind, repeat, left, right, del_size)
MODEL_ON_GOLDEN = [
    ("Seq0", 296, 4, 0, 266, 411, 114),
    ("Seq1", 739, 4, 2, 711, 848, 108),   # not in gold, which was made with the SNP observers on; variants.txt has it
    ("Seq4", 883, 4, 2, 855, 928, 44),
]


@pytest.fixture(scope="module")
def golden():
    solid = fc.solid_of_files(FASTQ_PAIR, K, CUTOFF)
    ref = pc.read_fasta(REFERENCE)
    names, seqs = [n for n, _ in ref], [s for _, s in ref]
    calls, st = fd.find_del(solid, K, seqs, MAX_REPEAT)
    return solid, names, seqs, calls, st


def test_model_on_the_golden_gives_the_three_deletions(golden):
    solid, names, seqs, calls, st = golden
    assert [(names[c[0]],) + c[1:] for c in calls] == MODEL_ON_GOLDEN
    # the two fallbacks are insertions of one nucleotide that repeats the one before it: begin + end holds, del_size = -1, no call
    assert st == {"n_gaps": 35, "n_candidates": 27, "n_del_clean": 1, "n_del_fuzzy": 2, "n_fallback": 2, "n_calls": 3}
    assert fd.find_del(solid, K, seqs, 1000)[0] == fd.find_del(solid, K, seqs, K - 2)[0]


def test_model_matches_gold_and_the_planted_list(golden):
    solid, names, seqs, calls, st = golden
    bk, vcf = fd.lines(calls, names, seqs, K)
    assert bk == []  # a deletion writes nothing to .breakpoints
    mine = fc.parse_vcf("\n".join(vcf))
    gold = fc.parse_vcf(open(os.path.join(G, "full_test", "gold.othervariants.del.vcf")).read())
    assert len(gold) == 2 and all(r[4] == "DEL" and r[7] == "1/1" for r in gold)
    assert [mine[0], mine[2]] == gold  # record for record: name, POS, REF, ALT, TYPE, LEN, FUZZY, GT
    planted = [l.split() for l in open(os.path.join(G, "full_test", "variants.txt")).read().splitlines() if " DEL " in l]
    assert ["Seq1", "739", "DEL", "end=847", "fuzzy=2"] in planted
    name, pos, ref, alt, typ, length, fuzzy, gt = mine[1]
    assert (name, pos - 1, pos - 1 + length, fuzzy) == ("Seq1", 739, 847, 2) and alt == ref[0] and len(ref) == length + 1
    assert vcf[0].startswith("Seq0\t297\tbkpt1\tCTAGCTTGAGAG") and vcf[0].endswith("\tC\t.\tPASS\tTYPE=DEL;LEN=114;FUZZY=0\tGT\t1/1")


def test_insertion_calls_on_the_golden_are_unchanged(golden):
    """no gap of the golden is called by both families: the 13 homozygous insertion calls stand next to the three deletions, in one literal
    scan with all five observers and through merge"""
    solid, names, seqs, calls, st = golden
    homo, _ = fc.find_homo(solid, K, seqs, MAX_REPEAT)
    family = fd.find_gap_family(solid, K, seqs, MAX_REPEAT, "-no-snp")
    assert len(homo) == 13 and [c for c in family if c[2] != 4] == homo and [c for c in family if c[2] == 4] == calls
    assert fd.merge(homo, calls) == family
    small = [c for c in homo if c[2] == 1]
    assert fd.find_gap_family(solid, K, seqs, MAX_REPEAT, "-deletion-only") == fd.merge(small, calls)


@pytest.mark.parametrize("reads, reference, want", [
    ("deleted.fasta", "ref_master.fasta", (0, 51, 4, 0, 21, 72, 20)),
    ("deletionfuzzy.fasta", "ref_deletionfuzzy.fasta", (0, 109, 4, 3, 82, 130, 20)),   # the sequence's name says del_between_110_130
])
def test_the_two_micro_cases(reads, reference, want):
    ref = pc.read_fasta(os.path.join(G, "micro", reference))
    seqs = [s for _, s in ref]
    for cutoff in (3, 2, 5):
        solid = fc.solid_of_files([os.path.join(G, "micro", reads)], K, cutoff)
        calls, st = fd.find_del(solid, K, seqs, MAX_REPEAT)
        assert calls == [want] and st["n_candidates"] == 1 and st["n_fallback"] == 0, cutoff
    if want[3]:
        assert "del_between_110_130" in ref[0][0]


# ---------------------------------------------------------------------------------------------------------------- hand-made cases, k = 5
A, B = "CCGTAACCAC", "TGGCAATCGGA"


def run5(ref, donors, max_repeat=2):
    return fd.find_del(fc.solid_of_strings(donors, 5), 5, [ref], max_repeat)


def test_hand_made_clean_and_fuzzy():
    """the graph holds A + B, the sequence A + D + B.  Clean: kmer_begin = AACCAC's last five at 5, kmer_end = TGGCA at 17, a gap of 11
    positions, del_size 11 - 5 + 1 = 7, pos = 9 (the C before D).  Fuzzy: D begins with TG as B does, so the k-mers CCACT and CACTG are solid
    too: kmer_begin moves to 7, the gap has 9 positions, r = 2, del_size 9 - 5 + 2 + 1 = 7, pos is the same"""
    calls, st = run5(A + "GAGTTCT" + B, [A + B])
    assert calls == [(0, 9, 4, 0, 5, 17, 7)] and st == {"n_gaps": 1, "n_candidates": 1, "n_del_clean": 1, "n_del_fuzzy": 0, "n_fallback": 0, "n_calls": 1}
    assert fd.lines(calls, ["chr"], [A + "gagTTCT" + B], 5)[1] == ["chr\t10\tbkpt1\tCgagTTCT\tC\t.\tPASS\tTYPE=DEL;LEN=7;FUZZY=0\tGT\t1/1"]  # the case is kept
    calls, st = run5(A + "TGAGTTA" + B, [A + B])
    assert calls == [(0, 9, 4, 2, 7, 17, 7)] and st["n_del_fuzzy"] == 1 and st["n_fallback"] == 0
    # the repeat is longer than max_repeat allows: begin + end does not hold, no call
    for mr in (0, 1):
        calls, st = run5(A + "TGAGTTA" + B, [A + B], mr)
        assert calls == [] and st["n_candidates"] == 1


def test_hand_made_fallback():
    """the graph holds ...TG TG..., the sequence ...TG D TG...: kmer_begin ends with TG, kmer_end begins with TG, r = 2, but the joined text
    with one TG is not in the graph; begin + end is: a clean deletion of the gap's length - k + 1"""
    a, b, d = "CCGTAACCAC", "GCAATCGGA", "ACAGTCA"
    calls, st = run5(a + "TG" + d + "TG" + b, [a + "TGTG" + b])
    assert calls == [(0, 11, 4, 0, 7, 19, 7)] and st["n_fallback"] == 1 and st["n_del_clean"] == 1 and st["n_del_fuzzy"] == 0


def test_hand_made_del_size_not_positive_and_the_length_threshold():
    """the graph holds A + C + B', the sequence A + B' (the C repeats A's last character): a gap of k - 2 = 3 positions, r = 1, the joined
    text with r = 1 is the sequence itself and fails, begin + end holds, del_size = 3 - 5 + 1 = -1: counted as a fallback, no call.  The
    insertion observers call the gap.  With max_repeat = 1 the gap is one short of k - max_repeat = 4 and no candidate"""
    b = "GCAATCGGA"
    solid = fc.solid_of_strings([A + "C" + b], 5)
    calls, st = fd.find_del(solid, 5, [A + b], 2)
    assert calls == [] and st == {"n_gaps": 1, "n_candidates": 1, "n_del_clean": 0, "n_del_fuzzy": 0, "n_fallback": 1, "n_calls": 0}
    assert fd.find_gap_family(solid, 5, [A + b], 2, "-no-snp") == [(0, 8, 1, 1, 5, 10, 1)]
    calls, st = fd.find_del(solid, 5, [A + b], 1)
    assert calls == [] and st["n_gaps"] == 1 and st["n_candidates"] == 0 and st["n_fallback"] == 0


def test_hand_made_gap_without_a_left_anchor():
    """a deletion at the very start of the sequence, and one behind an N that leaves fewer than two solid k-mers before the gap: the observers
    are called, kmer_begin is not valid, no candidate.  An N further back leaves the call alone"""
    d = "GAGTTCT"
    calls, st = run5(d + B + "ACCAGT", [A + B + "ACCAGT"])
    assert calls == [] and st["n_gaps"] == 1 and st["n_candidates"] == 0
    calls, st = run5(A[:6] + "N" + A[7:] + d + B, [A + B])
    assert calls == [] and st["n_gaps"] == 1 and st["n_candidates"] == 0
    calls, st = run5(A[:3] + "n" + A[4:] + d + B, [A + B])
    assert calls == [(0, 9, 4, 0, 5, 17, 7)]


# ---------------------------------------------------------------------------------------------------------------- the overlap rule
@pytest.mark.parametrize("k", [31, 13])
def test_deleted_tandem_copy_is_a_deletion_before_it_is_an_insertion_site(k):
    """one copy of a unit of d nt deleted from two or three: where the gap's length falls into [k - max_repeat, k - 1] the deletion observer
    calls it and, without that observer, a site observer does; with both the reference reports the deletion alone, and merge drops exactly
    that site"""
    rng = np.random.default_rng(500 + k)
    both = 0
    for d in range(1, 6):
        for copies in (2, 3):
            ref, donor = fd.tandem_case(rng, d, copies)
            solid = fc.solid_of_strings([donor], k)
            dels, st = fd.find_del(solid, k, [ref], MAX_REPEAT)
            homo, _ = fc.find_homo(solid, k, [ref], MAX_REPEAT)
            family = fd.find_gap_family(solid, k, [ref], MAX_REPEAT, "-no-snp")
            assert fd.merge(homo, dels) == family, (d, copies)
            if dels and homo:
                both += 1
                assert len(dels) == 1 and len(homo) == 1 and homo[0][2] == 0 and dels[0][4] == homo[0][4] and dels[0][6] == d, (d, copies)
                assert k - MAX_REPEAT <= dels[0][5] - dels[0][4] - 1 <= k - 1   # the gap's length
                assert family == dels and fd.find_gap_family(solid, k, [ref], MAX_REPEAT, "insertions") == homo
            elif dels:
                assert family == dels and dels[0][6] == d
    assert both >= 4


def test_merge_orders_by_detection_position():
    het, dele, hom = (0, 49, 2, 0, 19, 50, 0), (0, 40, 4, 2, 12, 49, 10), (0, 60, 0, 0, 30, 61, 0)
    assert fd.detected_at(dele) == (0, 50, 1) and fd.merge([hom], [dele], [het]) == [het, dele, hom]
    assert fd.merge([(0, 48, 0, 0, 12, 43, 0), hom], [dele]) == [dele, hom]  # the same (seq, left): dropped
    assert fd.merge([(1, 48, 0, 0, 12, 43, 0)], [dele]) == [dele, (1, 48, 0, 0, 12, 43, 0)]


# ---------------------------------------------------------------------------------------------------------------- the product without a GPU
def test_product_exports_the_del_entries():
    import mindthegap_amd
    lib = C.CDLL(mindthegap_amd.build_library())
    for name in ("mtg_index_find_del_sequences", "mtg_index_find_del_packed_device"):
        assert hasattr(lib, name), "missing export: " + name
    assert hasattr(mindthegap_amd.Index, "find_del_sequences") and hasattr(mindthegap_amd.Index, "find_del_packed_device")
    from mindthegap_amd import lib as L
    assert C.sizeof(L.FindDelStats) == 64 and [f[0] for f in L.FindDelStats._fields_][1:7] == list(fd.STAT_KEYS)
    hdr = open(os.path.join(ROOT, "include", "mtg_fill.h")).read()
    assert "uint64_t n_del_clean, n_del_fuzzy" in hdr and "typedef struct mtg_find_del_stats {" in hdr


def test_bad_arguments_are_refused_before_anything_else():
    import mindthegap_amd
    from mindthegap_amd import lib as L
    L._lib = None
    lib = mindthegap_amd.load_library()
    n = C.c_size_t()
    assert lib.mtg_index_find_del_sequences(None, None, 0, 5, None, 0, C.byref(n), None) == 2  # MTG_ERR_ARG: no index
    assert lib.mtg_index_find_del_packed_device(None, None, None, None, 0, 5, None, 0, C.byref(n), None) == 2


def test_find_tool_refusals(tmp_path):
    import mindthegap_amd
    exe = os.path.join(os.path.dirname(mindthegap_amd.build_library()), "MindTheGap")
    out = str(tmp_path / "f")
    base = [exe, "find", "-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-out", out]
    for extra in (["-deletion-only", "-max-rep", "-1"], ["-homo-only"], ["-snp-only"], ["-deletion-only", "-insert-only"], ["-homo-only", "-no-snp", "-hete-only"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "EXCEPTION" in r.stderr and os.listdir(str(tmp_path)) == [], extra
    r = subprocess.run(base + ["-homo-only"], capture_output=True, text=True)
    assert "SNPs" in r.stderr and "-deletion-only" in r.stderr and "-no-snp" in r.stderr


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
            lib.mtg_index_find_del_sequences.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
            assert lib.mtg_index_find_del_sequences(idx.h, arr, 1, 5, None, 0, C.byref(n), None) == 1   # MTG_ERR_NO_DEVICE
            assert lib.mtg_index_find_del_sequences(idx.h, arr, 1, -1, None, 0, C.byref(n), None) == 2  # the argument checks come first
        finally:
            idx.close()
        out = str(tmp_path / "f")
        for flags in (["-deletion-only"], ["-homo-only", "-no-snp"], ["-no-snp"]):
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


def test_repeat_joined_kmers_and_candidates_equal_the_literal_loops(tmp_path):
    """mtg_find_del.h by g++: the junction repeat for every k, max_repeat and agreement, every k-mer of every joined text with the two k-mers
    read across the word seams of a packed sequence, the candidate test, del_size and pos"""
    out = _build_and_run(tmp_path, "find_del", ["-O2"]).split()
    assert int(out[1]) > 40000 and int(out[3]) > 2000000 and int(out[5]) > 60000


def test_repeat_joined_kmers_and_candidates_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "find_del_san", ["-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
