"""The packed link path of a batch's sequence arena, on the CPU: the host's expander (AVX2 and scalar), the NULs it puts back from the records,
and the device's packed writer (mtg_emit.h, one lane) followed by the expansion against the all-ASCII arena."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_tail_expansion_matches_the_ascii_arena(tmp_path):
    """expand_codes for every start offset modulo 32 and every length up to 300, expand_packed_tail over random batches and shares, and
    emit_ascii_g's packed form + expansion against emit_ascii, with and without the vector path (MTG_NO_VEC)"""
    exe = str(tmp_path / "packed_tail")
    csrc = os.path.join(ROOT, "mindthegap_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "emu", f) for f in ("packed_tail.cpp", "emu_backend.cpp")] + [os.path.join(csrc, "mtg_cli.cpp")]
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-pthread", "-o", exe] + srcs + ["-lz"])
    for extra in ({}, {"MTG_NO_VEC": "1"}):
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **extra))
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (extra, r.stdout[-300:], r.stderr[-1000:])
