"""`find` for heterozygous insertions (include/mtg_fill.h: mtg_index_find_het_sequences) without a GPU: the plain model (tests/find_het_cases.py)
against the reference's golden records, the word-level logic the kernels share with tests/emu/find_het.cpp against literal loops (also under
AddressSanitizer + UBSan, as a program of its own), the merge rule of -insert-only, the exports, and the refusals.

tests/golden/full_test/gold.othervariants.het_ins.vcf is a data fixture: the `0/1` record lines of the reference's
test/full_test/gold.othervariants.vcf (results of its `find` on tests/golden/full_test/reference.fasta and the golden reads)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import find_cases as fc
from tests import find_het_cases as fh
from tests import profile_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HARNESS = os.path.join(ROOT, "tests", "emu", "find_het.cpp")
FASTQ_PAIR = [os.path.join(G, "data", "reads_r1.fastq"), os.path.join(G, "data", "reads_r2.fastq")]
REFERENCE = os.path.join(G, "full_test", "reference.fasta")
K, CUTOFF, MAX_REPEAT, BRANCHING = 31, 7, 5, 15

# The model's calls on the golden reference, (name, pos 0-based, kind, repeat, left, right, ins).  Against the reference's gold files (made with
# every observer on): the HET sites Seq1/342 and Seq4/351 and all seven 0/1 insertions are here as gold has them.  Gold's third HET site,
# Seq0/123, is missing: its left k-mer covers the homozygous SNP at Seq0/101 and has out-degree 2 only once FindSoloSNP::correct_history has
# rewritten the history, which no observer in scope does.
MODEL_ON_GOLDEN = [
    ("Seq1", 341, 2, 0, 311, 342, 0),
    ("Seq4", 350, 2, 2, 320, 351, 0),
    ("Seq5", 599, 3, 0, 569, 600, 0),
    ("Seq5", 699, 3, 0, 669, 700, 1),
    ("Seq5", 799, 3, 2, 771, 802, 1),
    ("Seq5", 899, 3, 2, 871, 902, 2),
    ("Seq6", 599, 3, 0, 569, 600, 8),
    ("Seq6", 698, 3, 2, 670, 701, 15),
    ("Seq6", 799, 3, 0, 769, 800, 14),
]


@pytest.fixture(scope="module")
def golden():
    solid = fc.solid_of_files(FASTQ_PAIR, K, CUTOFF)
    ref = pc.read_fasta(REFERENCE)
    names, seqs = [n for n, _ in ref], [s for _, s in ref]
    rep = fh.repeated_set(seqs, K, 1)
    calls, st = fh.find_het(solid, K, seqs, fh.repeat_flags(seqs, K, rep), MAX_REPEAT, BRANCHING)
    return solid, names, seqs, rep, calls, st


def test_model_on_the_golden_gives_the_nine_calls(golden):
    solid, names, seqs, rep, calls, st = golden
    assert rep == set()  # the golden genome has no 30-mer that occurs twice: the repeat test decides nothing there
    assert [(names[c[0]],) + c[1:] for c in calls] == MODEL_ON_GOLDEN
    assert st == {"n_candidates": 9, "n_raw_sites": 2, "n_filtered": 0, "n_suppressed": 0, "n_het_clean": 1, "n_het_fuzzy": 1, "n_het_small": 7}
    assert fh.find_het(solid, K, seqs, None, MAX_REPEAT, -1)[0] == calls  # without the branching filter: the same


def test_model_matches_the_golden_records(golden):
    solid, names, seqs, rep, calls, st = golden
    bk, vcf = fh.lines(calls, names, seqs, K)
    gold_ins = fc.parse_vcf(open(os.path.join(G, "full_test", "gold.othervariants.het_ins.vcf")).read())
    assert len(gold_ins) == 7 and all(r[7] == "0/1" for r in gold_ins)
    assert fc.parse_vcf("\n".join(vcf)) == gold_ins  # record for record: name, POS, REF, ALT, TYPE, LEN, FUZZY, GT
    mine = {(n, p, f): (l, r) for n, p, f, t, l, r in fc.parse_breakpoints("\n".join(bk)) if t == "HET"}
    gold = {(n, p, f): (l, r) for n, p, f, t, l, r in fc.parse_breakpoints(open(os.path.join(G, "full_test", "gold.breakpoints")).read()) if t == "HET"}
    assert sorted(mine) == [("Seq1", 342, 0), ("Seq4", 351, 2)] and sorted(gold) == [("Seq0", 123, 0)] + sorted(mine)
    for key in mine:
        assert mine[key] == gold[key], key  # the left and the right k-mer strings
    assert bk[0] == ">bkpt1_Seq1_pos_342_fuzzy_0_HET  left_kmer" and vcf[0] == "Seq5\t600\tbkpt3\tG\tGA\t.\tPASS\tTYPE=INS;LEN=1;FUZZY=0\tGT\t0/1"


def test_merge_rule_of_insert_only(golden):
    """both layers in detection order: a heterozygous call is made at right - repeat, a homozygous one at right - repeat + 1, heterozygous first
    at equal positions; ids count across the merged list"""
    solid, names, seqs, rep, calls, st = golden
    homo, _ = fc.find_homo(solid, K, seqs, MAX_REPEAT)
    both = fh.merge(homo, calls)
    assert len(both) == 22 and [c for c in both if c[2] >= 2] == calls and [c for c in both if c[2] < 2] == homo
    assert [(names[c[0]], c[1], c[2]) for c in both[:5]] == [("Seq1", 341, 2), ("Seq2", 534, 0), ("Seq2", 834, 0), ("Seq4", 350, 2), ("Seq4", 602, 0)]
    bk, vcf = fh.lines(both, names, seqs, K)
    assert len(bk) == 20 and len(vcf) == 17 and bk[4].startswith(">bkpt2_Seq2_pos_535_fuzzy_0_HOM") and vcf[5].startswith("Seq5\t600\tbkpt11\t")
    # a homozygous call detected at p + 1 and a heterozygous one at p + 1: the heterozygous one first; at p: before the homozygous one of p
    het, hom = (0, 49, 2, 0, 19, 50, 0), (0, 48, 0, 0, 18, 49, 0)
    assert fh.detected_at(het)[:2] == fh.detected_at(hom)[:2] == (0, 50) and fh.merge([hom], [het]) == [het, hom]
    assert fh.merge([(0, 47, 0, 0, 17, 48, 0)], [het]) == [(0, 47, 0, 0, 17, 48, 0), het]


def test_model_on_a_hand_made_case():
    """k = 5, one sequence, two haplotypes in the graph: the reference's own text and the text with GACGAGTA behind ...AACCAC.  The k-mer
    ACCAC (position 5) then has out-degree 2, TGGCA (position 10) in-degree 2; at p = 10 the slot p - k holds ACCAC: a clean site, pos p - 1.
    With GT instead of the eight nucleotides the micro-assembly finds an insertion (its first string that assembles)."""
    k = 5
    ref = "CCGTAACCAC" + "TGGCAATCGGA"
    solid = fc.solid_of_strings([ref, "CCGTAACCAC" + "GACGAGTA" + "TGGCAATCGGA"], k)
    calls, st = fh.find_het(solid, k, [ref], None, 2, -1)
    assert calls == [(0, 9, 2, 0, 5, 10, 0)] and st["n_het_clean"] == 1 and st["n_candidates"] == 1
    bk, vcf = fh.lines(calls, ["chr"], [ref], k)
    assert bk == [">bkpt1_chr_pos_10_fuzzy_0_HET  left_kmer", "ACCAC", ">bkpt1_chr_pos_10_fuzzy_0_HET  right_kmer", "TGGCA"] and vcf == []
    # the repeat flags silence it: on the prefix of p, on the suffix of q
    for q in (10, 6):
        flags = [bytes(1 if i == q else 0 for i in range(len(ref) - k + 2))]
        assert fh.find_het(solid, k, [ref], flags, 2, -1)[0] == []
    solid2 = fc.solid_of_strings([ref, "CCGTAACCAC" + "GT" + "TGGCAATCGGA"], k)
    calls2, st2 = fh.find_het(solid2, k, [ref], None, 2, -1)
    assert [c[:4] for c in calls2] == [(0, 9, 3, 0)] and st2["n_het_small"] == 1
    assert fh.lines(calls2, ["chr"], [ref], k)[1][0].endswith("\tGT\t0/1")


def test_product_exports_the_het_entries():
    import mindthegap_amd
    lib = C.CDLL(mindthegap_amd.build_library())
    for name in ("mtg_index_find_het_sequences", "mtg_index_find_het_packed_device", "mtg_index_find_homo_sequences", "mtg_find_main"):
        assert hasattr(lib, name), "missing export: " + name
    assert hasattr(mindthegap_amd.Index, "find_het_sequences") and hasattr(mindthegap_amd.Index, "find_het_packed_device")
    from mindthegap_amd import CALL_DTYPE, decode_find_calls
    raw = np.array([1, 341, 2, 0, 311, 342, 0, 5, 599, 3, 0, 569, 600, 8], dtype=np.uint32)
    got = decode_find_calls(raw.tobytes(), 2)
    assert got.dtype == CALL_DTYPE and got["kind"].tolist() == [2, 3] and got["ins"].tolist() == [0, 8]
    hdr = open(os.path.join(ROOT, "include", "mtg_fill.h")).read()
    assert "typedef struct mtg_find_call { uint32_t seq, pos, kind, repeat, left, right, ins; } mtg_find_call;" in hdr
    from mindthegap_amd import lib as L
    assert C.sizeof(L.FindHetStats) == 72 and [f[0] for f in L.FindHetStats._fields_][1:8] == list(fh.STAT_KEYS)


def test_bad_arguments_are_refused_before_anything_else():
    import mindthegap_amd
    from mindthegap_amd import lib as L
    L._lib = None
    lib = mindthegap_amd.load_library()
    n = C.c_size_t()
    assert lib.mtg_index_find_het_sequences(None, None, 0, None, 5, 15, None, 0, C.byref(n), None) == 2  # MTG_ERR_ARG: no index
    assert lib.mtg_index_find_het_packed_device(None, None, None, None, 0, None, 5, 15, None, 0, C.byref(n), None) == 2


def test_find_tool_refusals(tmp_path):
    import mindthegap_amd
    exe = os.path.join(os.path.dirname(mindthegap_amd.build_library()), "MindTheGap")
    out = str(tmp_path / "f")
    base = [exe, "find", "-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-out", out]
    for extra in (["-hete-only", "-max-rep", "-1"], ["-insert-only", "-kmer-size", "11"], ["-hete-only", "-het-max-occ"], ["-insert-only", "-branching-filter"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "EXCEPTION" in r.stderr and os.listdir(str(tmp_path)) == [], extra
    r = subprocess.run(base + ["-insert-only", "-kmer-size", "11"], capture_output=True, text=True)
    assert "k-mer size of at least 12" in r.stderr


def test_host_code_without_the_device_unit_says_so(tmp_path):
    """the product's host code linked against the emulated backend has no device code for find: the entry answers MTG_ERR_NO_DEVICE through the
    weak stand-in (before it looks at its arguments' contents) and the tool writes nothing"""
    from tests import emu_lib
    m = emu_lib.product_on_emulator()
    try:
        lib = C.CDLL(emu_lib.FULL_SO)
        n = C.c_size_t()
        kms = np.array(sorted(fc.solid_of_strings(["ACGTTGCAAGGCTTAACCGGATGCAT"], 11)), dtype=np.uint64)
        idx = m.Index.from_kmers(kms, np.full(len(kms), 9, dtype=np.uint32), 11)
        try:
            arr = (C.c_char_p * 1)(b"ACGTTGCAAGGCTTAACCGGATGCAT")
            lib.mtg_index_find_het_sequences.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
            assert lib.mtg_index_find_het_sequences(idx.h, arr, 1, None, 5, 15, None, 0, C.byref(n), None) == 1  # MTG_ERR_NO_DEVICE
            assert lib.mtg_index_find_het_sequences(idx.h, arr, 1, None, -1, 15, None, 0, C.byref(n), None) == 2  # the argument checks come first
        finally:
            idx.close()
        out = str(tmp_path / "f")
        for flag in ("-hete-only", "-insert-only"):
            assert m.find_main(["-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, flag, "-abundance-min", str(CUTOFF), "-out", out]) == 1
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


def test_candidate_words_and_chains_equal_the_literal_loops(tmp_path):
    """mtg_find_het.h by g++: every alignment of a site against the 64-bit seams, windows clipped at both sequence ends, chains of 1 to 4 raw
    sites at spacings max_repeat and max_repeat + 1, the ring of 256 history slots, random planes"""
    out = _build_and_run(tmp_path, "find_het", ["-O2"]).split()
    assert int(out[1]) > 50000 and int(out[3]) > 100000 and int(out[5]) > 500000


def test_candidate_words_and_chains_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "find_het_san", ["-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
