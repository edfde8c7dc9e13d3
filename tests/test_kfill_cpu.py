"""The whole fill at k below 31 and with off-default limits, on the emulator: the product's host code and tool linked against the host emulation of
the device code (tests/emu), against the oracle.  The cases are tests/kfill_cases.py; tests/test_gpu_kfill.py runs them through the HIP kernels."""
import os
import subprocess

import pytest

from tests import emu_lib, kfill_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu_product():
    from mindthegap_amd import lib as L
    saved = L._lib
    yield emu_lib.product_on_emulator()
    L._lib = saved


@pytest.mark.parametrize("het", [0, 2])
@pytest.mark.parametrize("k", K.BKPT_KS)
def test_bkpt_sweep_on_emulator(emu_product, tmp_path, k, het):
    """(k = 16 with default parameters: several launches, the multi-contig cross-check of the emulation compares launch by launch)"""
    K.bkpt_sweep(emu_product, tmp_path, k, het)


@pytest.mark.parametrize("host_format", [False, True])
@pytest.mark.parametrize("k", K.SHORT_KS)
def test_short_fills_every_alignment_on_emulator(emu_product, tmp_path, monkeypatch, k, host_format):
    if host_format:
        monkeypatch.setenv("MTG_HOST_FORMAT", "1")
    K.short_fills(emu_product, tmp_path, k)


@pytest.mark.parametrize("k", K.MIS_KS)
def test_nb_mis_allowed_on_emulator(emu_product, tmp_path, k):
    K.nb_mis_case(emu_product, tmp_path, k)


@pytest.mark.parametrize("k", K.CONTIG_KS)
def test_contig_mode_sixteen_targets_on_emulator(emu_product, tmp_path, monkeypatch, k):
    """(the emulation has no shared target table: every seed takes the per-seed path, so one run per overlap)"""
    K.contig_case(emu_product, tmp_path, k, monkeypatch, per_seed_too=False)


@pytest.mark.parametrize("k", K.TEXT_KS)
def test_text_entry_on_emulator(emu_product, tmp_path, k):
    K.text_case(emu_product, tmp_path, k)


def test_pieces_of_the_terminal_search_index(tmp_path):
    """tests/emu/piece_layout.cpp: for every k and nb_mis_allowed the pieces tile the k-mer (unequal lengths where nb_mis + 1 does not divide k), and
    the indexed search finds a target with substitutions at every set of up to nb_mis positions"""
    exe = str(tmp_path / "piece_layout")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "emu", "piece_layout.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout[-500:], r.stderr[-1000:])
    assert int(r.stdout.split()[1]) == 21 * 4 and int(r.stdout.split()[3]) > 3000  # every (k, nb_mis); the pairs of positions at k >= 24
