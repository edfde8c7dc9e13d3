"""`find` for homozygous insertions (include/mtg_fill.h: mtg_index_find_homo_sequences) without a GPU: the plain model (tests/find_cases.py)
against the reference's golden records, the gap rule's two statements against each other, the word-level gap extraction the kernels share
with tests/emu/find_gaps.cpp against the literal loop (also under AddressSanitizer + UBSan, as a program of its own), the exports, and the
tool's refusals.

tests/golden/full_test/gold.othervariants.hom_ins.vcf is a data fixture: the `1/1` TYPE=INS record lines of the reference's
test/full_test/gold.othervariants.vcf (results of its `find` on tests/golden/full_test/reference.fasta and the golden reads)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import find_cases as fc
from tests import profile_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HARNESS = os.path.join(ROOT, "tests", "emu", "find_gaps.cpp")
FASTQ_PAIR = [os.path.join(G, "data", "reads_r1.fastq"), os.path.join(G, "data", "reads_r2.fastq")]
REFERENCE = os.path.join(G, "full_test", "reference.fasta")
K, CUTOFF, MAX_REPEAT = 31, 7, 5

# The model's calls on the golden reference, (name, pos 0-based, kind, repeat, left, right, ins).  Against the reference's gold files
# (gold.breakpoints, gold.othervariants.vcf, made with every observer on):
#   + the three HOM sites Seq2/535, Seq2/835, Seq4/603 and the nine 1/1 insertions of 1-2 nt are here as gold has them;
#   - Seq3/781 and Seq4/821 (HOM in gold) are missing: each lies next to a SNP ("HOM clean after SNP" / "before SNP" in the reference's
#     variants.txt), its gap is 46 resp. 50 positions long, and only the SNP observers, which are not run here, cut such a gap to k - 1;
#   - Seq4/884 (a deletion in gold) does not surface as a fuzzy site: its gap is longer than k - 1;
#   + Seq6/500 G -> GTC is a call gold does not list.  The reads do carry it -- all k + 3 windows of left + TC + right are solid and the 30
#     reference k-mers across the junction are absent, like its neighbour Seq6/400 -- so the four observers, taken literally, call it; why
#     the gold run (version 2.2.3) did not has not been established.
MODEL_ON_GOLDEN = [
    ("Seq2", 534, 0, 0, 504, 535, 0),
    ("Seq2", 834, 0, 1, 804, 835, 0),
    ("Seq4", 602, 0, 3, 572, 603, 0),
    ("Seq5", 99, 1, 1, 70, 101, 1),
    ("Seq5", 198, 1, 1, 169, 200, 2),
    ("Seq5", 299, 1, 0, 269, 300, 1),
    ("Seq5", 399, 1, 2, 371, 402, 3),
    ("Seq5", 499, 1, 0, 469, 500, 3),
    ("Seq6", 97, 1, 3, 70, 101, 7),
    ("Seq6", 199, 1, 1, 170, 201, 10),
    ("Seq6", 299, 1, 1, 270, 301, 16),
    ("Seq6", 399, 1, 0, 369, 400, 8),
    ("Seq6", 499, 1, 0, 469, 500, 17),
]


@pytest.fixture(scope="module")
def golden():
    solid = fc.solid_of_files(FASTQ_PAIR, K, CUTOFF)
    assert len(solid) == 7419
    ref = pc.read_fasta(REFERENCE)
    names, seqs = [n for n, _ in ref], [s for _, s in ref]
    calls, st = fc.find_homo(solid, K, seqs, MAX_REPEAT)
    return solid, names, seqs, calls, st


def test_model_holds_the_twelve_golden_records(golden):
    solid, names, seqs, calls, st = golden
    bk, vcf = fc.breakpoint_lines(calls, names, seqs, K)
    mine = {(n, p, f): (l, r) for n, p, f, t, l, r in fc.parse_breakpoints("\n".join(bk)) if t == "HOM"}
    gold = {(n, p, f): (l, r) for n, p, f, t, l, r in fc.parse_breakpoints(open(os.path.join(G, "full_test", "gold.breakpoints")).read()) if t == "HOM"}
    for key in (("Seq2", 535, 0), ("Seq2", 835, 1), ("Seq4", 603, 3)):
        assert mine[key] == gold[key], key  # the left and the right k-mer strings
    gold_ins = fc.parse_vcf(open(os.path.join(G, "full_test", "gold.othervariants.hom_ins.vcf")).read())
    assert [(n, p) for n, p, *_ in gold_ins] == [("Seq5", 100), ("Seq5", 199), ("Seq5", 300), ("Seq5", 400), ("Seq5", 500), ("Seq6", 98), ("Seq6", 200), ("Seq6", 300), ("Seq6", 400)]
    mine_ins = fc.parse_vcf("\n".join(vcf))
    for rec in gold_ins:  # POS, REF, ALT, TYPE, LEN, FUZZY, GT
        assert rec in mine_ins, rec


def test_model_on_the_golden_in_full(golden):
    solid, names, seqs, calls, st = golden
    assert [(names[c[0]],) + c[1:] for c in calls] == MODEL_ON_GOLDEN
    assert st == {"n_gaps": 35, "n_candidates": 13, "n_homo_clean": 1, "n_homo_fuzzy": 2, "n_small_clean": 4, "n_small_fuzzy": 6}
    bk, vcf = fc.breakpoint_lines(calls, names, seqs, K)
    assert bk[0] == ">bkpt1_Seq2_pos_535_fuzzy_0_HOM  left_kmer" and bk[1] == "GGCATGCGTAAGTTATCGTGAAACCATGATG" and len(bk) == 12
    assert vcf[0] == "Seq5\t100\tbkpt4\tT\tTC\t.\tPASS\tTYPE=INS;LEN=1;FUZZY=1\tGT\t1/1" and len(vcf) == 10


def test_the_two_statements_of_the_gap_rule_agree(golden):
    """the literal loop of notify() and the anchors of csrc/mtg_find_gaps.h: same reported gaps, same validity of kmer_begin -- on the golden
    and on strings with isolated solid k-mers, N and short sequences"""
    solid, names, seqs, calls, st = golden
    assert fc.gaps_by_anchors(solid, K, seqs) == fc.literal_gaps(solid, K, seqs) and len(fc.literal_gaps(solid, K, seqs)) == 35
    rng = np.random.default_rng(3)
    k = 5
    donor = fc.rand_seq(rng, 400)
    small = fc.solid_of_strings([donor], k)
    strings = []
    for i in range(300):
        s = list(donor[int(rng.integers(0, 200)):][:int(rng.integers(0, 200))])
        for _ in range(int(rng.integers(0, 8))):
            if s:
                s[int(rng.integers(len(s)))] = "ACGTN"[int(rng.integers(5))]
        strings.append("".join(s))
    a, b = fc.gaps_by_anchors(small, k, strings), fc.literal_gaps(small, k, strings)
    assert a == b and len(a) > 300 and any(not fresh for _, _, _, fresh in a)


def test_model_on_a_hand_made_case():
    """k = 5; the donor carries GT between ...ACCAC and TGGCA...: the reference lacks it.  Gap of k - 1 = 4 positions (CCACT, CACTG, ACTGG,
    CTGGC are not the donor's), r = 0, first solid position behind it e = 10.  The micro-assembly stops at "G" (index 2), before it
    gets to "GT": of ACCAC + G + TGGCA the first five windows ACCAC, CCACG, CACGT, ACGTG (the reverse complement of CACGT) and CGTGG (that
    of CCACG) are all nodes, and the sixth, GTGGC, is not looked at -- the reference's rule, taken literally"""
    k = 5
    donor = "CCGTAACCAC" + "GT" + "TGGCAATCGGA"
    ref = "CCGTAACCAC" + "TGGCAATCGGA"
    solid = fc.solid_of_strings([donor], k)
    calls, st = fc.find_homo(solid, k, [ref], 2)
    assert calls == [(0, 9, 1, 0, 5, 10, 2)] and st["n_gaps"] == 1 and st["n_candidates"] == 1 and st["n_small_clean"] == 1
    bk, vcf = fc.breakpoint_lines(calls, ["chr"], [ref], k)
    assert bk == [] and vcf == ["chr\t10\tbkpt1\tC\tCG\t.\tPASS\tTYPE=INS;LEN=1;FUZZY=0\tGT\t1/1"]
    # a longer insertion at the same place is a site: nothing assembles in 1-2 nt
    donor2 = "CCGTAACCAC" + "GACGAGTA" + "TGGCAATCGGA"
    calls2, st2 = fc.find_homo(fc.solid_of_strings([donor2], k), k, [ref], 2)
    assert calls2 == [(0, 9, 0, 0, 5, 10, 0)] and st2["n_homo_clean"] == 1


def test_product_exports_the_find_entries():
    import mindthegap_amd
    lib = C.CDLL(mindthegap_amd.build_library())
    for name in ("mtg_index_find_homo_sequences", "mtg_index_find_homo_packed_device", "mtg_find_main"):
        assert hasattr(lib, name), "missing export: " + name
    from mindthegap_amd import CALL_DTYPE, FIND_INSERTIONS, decode_find_calls, find_main  # noqa: F401
    assert hasattr(mindthegap_amd.Index, "find_homo_sequences") and hasattr(mindthegap_amd.Index, "find_homo_packed_device")
    assert CALL_DTYPE == fc.CALL_DTYPE and CALL_DTYPE.itemsize == 28 and list(FIND_INSERTIONS) == fc.INSERTIONS
    raw = np.arange(14, dtype=np.uint32)
    assert decode_find_calls(raw.tobytes(), 2).tolist() == [tuple(range(7)), tuple(range(7, 14))]
    hdr = open(os.path.join(ROOT, "include", "mtg_fill.h")).read()
    assert "typedef struct mtg_find_call { uint32_t seq, pos, kind, repeat, left, right, ins; } mtg_find_call;" in hdr


def test_bad_arguments_are_refused_before_anything_else():
    import mindthegap_amd
    from mindthegap_amd import lib as L
    L._lib = None
    lib = mindthegap_amd.load_library()
    n = C.c_size_t()
    assert lib.mtg_index_find_homo_sequences(None, None, 0, 5, None, 0, C.byref(n), None) == 2  # MTG_ERR_ARG: no index
    assert lib.mtg_index_find_homo_packed_device(None, None, None, None, 0, 5, None, 0, C.byref(n), None) == 2


def test_find_tool_names_what_is_not_built(tmp_path):
    """without -homo-insertions the tool stops before it reads anything: the subset is not to be mistaken for the reference's default find"""
    import mindthegap_amd
    exe = os.path.join(os.path.dirname(mindthegap_amd.build_library()), "MindTheGap")
    out = str(tmp_path / "f")
    r = subprocess.run([exe, "find", "-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-out", out], capture_output=True, text=True)
    assert r.returncode == 1 and os.listdir(str(tmp_path)) == []
    for word in ("SNPs", "deletions", "heterozygous", "-bed", "-homo-insertions"):
        assert word in r.stderr, word
    r = subprocess.run([exe, "find", "-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-homo-insertions", "-max-rep", "-1", "-out", out], capture_output=True, text=True)
    assert r.returncode == 1 and "EXCEPTION" in r.stderr and os.listdir(str(tmp_path)) == []
    from mindthegap_amd import lib as L
    L._lib = None
    assert mindthegap_amd.find_main(["-graph", "x", "-ref", REFERENCE, "-out", out]) == 1 and os.listdir(str(tmp_path)) == []


def test_host_code_without_the_device_unit_says_so(tmp_path):
    """the product's host code linked against the emulated backend has no device code for find (the micro-assembly lives in the HIP unit, as
    the profile does): the entry answers MTG_ERR_NO_DEVICE through the weak stand-in and the tool writes nothing"""
    from tests import emu_lib
    m = emu_lib.product_on_emulator()
    try:
        out = str(tmp_path / "f")
        assert m.find_main(["-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-homo-insertions", "-abundance-min", str(CUTOFF), "-out", out]) == 1
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


def test_gap_extraction_equals_the_literal_loop(tmp_path):
    """mtg_find_gaps.h by g++: every alignment of a gap against the 64-bit seams, isolated present bits at the word edges, a gap as long as
    the input, 0 and 1 sequences, random planes"""
    out = _build_and_run(tmp_path, "find_gaps", ["-O2"])
    assert int(out.split()[1]) > 50000 and int(out.split()[3]) > 100000


def test_gap_extraction_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "find_gaps_san", ["-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
