"""The sequence profile (include/mtg_fill.h: mtg_index_profile_sequences) without a GPU: the product exports it and the Python names import,
the tool refuses to run without a device and leaves no files, and the run extraction and the bad-bit test the kernels share with
tests/emu/profile_runs.cpp equal literal loops (also under AddressSanitizer + UBSan, as a program of its own)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import profile_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HARNESS = os.path.join(ROOT, "tests", "emu", "profile_runs.cpp")


def test_product_exports_the_profile_entries():
    import mindthegap_amd
    lib = C.CDLL(mindthegap_amd.build_library())
    for name in ("mtg_index_profile_sequences", "mtg_index_profile_packed_device", "mtg_profile_main"):
        assert hasattr(lib, name), "missing export: " + name
    from mindthegap_amd import RUN_DTYPE, profile_abundance, profile_main, profile_pred, profile_present, profile_succ, profile_valid  # noqa: F401
    assert hasattr(mindthegap_amd.Index, "profile_sequences") and hasattr(mindthegap_amd.Index, "profile_packed_device")
    assert RUN_DTYPE.itemsize == 16 and RUN_DTYPE.names == ("seq", "start", "length", "flags")
    # the decoders and the header agree on the layout of the word
    w = np.array([(1 << 17) | (1 << 16) | (0b1001 << 12) | (0b0110 << 8) | 200, 1 << 16, 0], dtype=np.uint32)
    assert list(profile_abundance(w)) == [200, 0, 0] and list(profile_succ(w)) == [6, 0, 0] and list(profile_pred(w)) == [9, 0, 0]
    assert list(profile_valid(w)) == [1, 1, 0] and list(profile_present(w)) == [1, 0, 0]
    hdr = open(os.path.join(ROOT, "include", "mtg_fill.h")).read()
    for macro, sh in (("ABUNDANCE(w) ((w) & 255u)", None), ("SUCC", 8), ("PRED", 12), ("VALID", 16), ("PRESENT", 17)):
        assert ("MTG_PROFILE_" + macro) in hdr and (sh is None or "MTG_PROFILE_%s(w) (((w) >> %d)" % (macro, sh) in hdr)


def test_null_arguments_are_refused_before_anything_else():
    import mindthegap_amd
    from mindthegap_amd import lib as L
    L._lib = None
    lib = mindthegap_amd.load_library()
    n = C.c_size_t()
    assert lib.mtg_index_profile_sequences(None, None, 0, None, None, 0, C.byref(n), None) == 2  # MTG_ERR_ARG: no index
    assert lib.mtg_index_profile_packed_device(None, None, None, None, 0, None, None, None, 0, C.byref(n), None) == 2


def test_profile_tool_without_a_device_writes_nothing(tmp_path):
    import mindthegap_amd
    from mindthegap_amd import lib as L
    L._lib = None
    mindthegap_amd.load_library()
    if mindthegap_amd.device_count() > 0:
        pytest.skip("a HIP device is present")
    out = str(tmp_path / "p")
    reads = os.path.join(G, "data", "reads_r1.fastq") + "," + os.path.join(G, "data", "reads_r2.fastq")
    assert mindthegap_amd.profile_main(["-in", reads, "-ref", os.path.join(G, "full_test", "reference.fasta"), "-abundance-min", "7", "-out", out]) == 1
    assert os.listdir(str(tmp_path)) == []
    exe = os.path.join(os.path.dirname(mindthegap_amd.build_library()), "MindTheGap")
    r = subprocess.run([exe, "profile", "-in", reads, "-ref", os.path.join(G, "full_test", "reference.fasta"), "-out", out], capture_output=True, text=True)
    assert r.returncode == 1 and "EXCEPTION" in r.stderr and os.listdir(str(tmp_path)) == []


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-g", "-std=c++17", "-Wall"] + flags + ["-o", exe, HARNESS])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stderr == ""  # UBSan reports on stderr and goes on
    return r.stdout


def test_run_extraction_equals_the_literal_loop(tmp_path):
    """mtg_profile_runs.h by g++: every alignment of a run against the 64-bit and the 256-position seams, random planes of 0 .. 1100 positions"""
    out = _build_and_run(tmp_path, "profile_runs", ["-O2"])
    assert int(out.split()[1]) > 100000 and int(out.split()[3]) > 100000
    assert int(out.split()[5]) > 22 * 131 * 7  # covers_bad: 22 values of k, 131 of p, four random planes, the zero plane, two to four single bits


def test_run_extraction_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "profile_runs_san", ["-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


def test_model_on_a_hand_made_case():
    """the model itself, on a case small enough to do by hand: k = 3, solid = {ACG (and CGT, its reverse complement), CGA (TCG)}"""
    from tests.reads_cases import canon, encode
    solid = {canon(encode("ACG"), 3): 5, canon(encode("CGA"), 3): 255}
    words, runs = profile_cases.profile(solid, 3, ["ACGAnACGTT", "AC", ""])
    w = words[0]
    assert len(w) == 8 and len(words[1]) == 0 and len(words[2]) == 0
    # ACG: present, abundance 5, successors CGA (A = bit 0) and CGT (T = bit 2, the reverse complement of ACG), no predecessor (xAC: none)
    assert int(w[0]) == (1 << 17) | (1 << 16) | (0b0101 << 8) | 5
    # CGA: present, 255, predecessors ACG (A) and TCG (T, the reverse complement of CGA), successors GAx: none
    assert int(w[1]) == (1 << 17) | (1 << 16) | (0b0101 << 12) | 255
    assert [int(x) for x in w[2:5]] == [0, 0, 0]                       # GAn, AnA, nAC: invalid
    assert int(w[5]) == int(w[0]) and int(w[6]) == (1 << 17) | (1 << 16) | (0b0101 << 12) | 5   # ACG again; CGT = rc(ACG): predecessors ACG and TCG, successors GTx: none
    assert int(w[7]) == 1 << 16                                        # GTT: valid, absent
    assert [tuple(int(x) for x in r) for r in runs] == [(0, 7, 1, 1)]
