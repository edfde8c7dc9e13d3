"""Contig mode's shared target table (include/mtg_fill.h: mtg_targets_create / mtg_fill_seeds) without a GPU: the product exports it, the device's
terminal search for a seed of the table equals the reference's search over the seed's own dictionary (emulation build of mtg_post.h), and the host
side of mtg_fill_seeds -- per-seed dictionaries in the order of a fresh unordered_map, table numbers in the results -- on the emulator."""
import ctypes as C
import os
import subprocess

import pytest

from tests import emu_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_product_exports_the_seed_table_entries():
    import mindthegap_amd
    lib = C.CDLL(mindthegap_amd.build_library())
    for name in ("mtg_targets_create", "mtg_targets_free", "mtg_targets_device_bytes", "mtg_fill_seeds"):
        assert hasattr(lib, name), "missing export: " + name
    from mindthegap_amd import Seed, Targets  # noqa: F401  (the Python side of the table)
    assert any(t["name"] == "CONTIG_PER_SEED" for t in mindthegap_amd.tuning())


def test_terminal_search_of_a_table_seed_equals_the_reference(tmp_path):
    """mtg_post.h's indexed search with the table's piece index and the seed's exclusions, against a literal find_nodes_containing_multiple_R over
    the per-seed unordered_map: 3 000 random tables of 2 .. 2 000 targets (mutated, N, lower case, short keys, built ties), 0 .. 2 exclusions; the tie
    flag is up exactly where the seed's dictionary order decides; the early-stop pattern with the excluded keys cut out equals the concatenation"""
    exe = str(tmp_path / "seed_table")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "emu", "seed_table.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout[-500:], r.stderr[-1000:])
    ties = int(r.stdout.split(" ties")[0].split()[-1])
    assert ties >= 20  # the built ties do reach the flag


@pytest.fixture
def emu_product():
    from mindthegap_amd import lib as L
    saved = L._lib
    yield emu_lib.product_on_emulator()
    L._lib = saved


def test_fill_seeds_on_emulator_equals_fill_batch(emu_product):
    """the bundled contig case through fill_seeds (the emulation has no device table: every seed takes the per-seed path, with its dictionary in
    the order of a fresh unordered_map) equals fill_batch with explicit dictionaries, target numbers mapped to the table's"""
    from tests.test_gpu_seed_table import _compare_with_fill_batch, _table_of_contigs
    idx = emu_product.Index.from_reads([os.path.join(G, "data", "contig-reads.fasta.gz")], 31, 3)
    try:
        entries, seeds, own = _table_of_contigs(os.path.join(G, "data", "contigs.fasta"))
        assert _compare_with_fill_batch(emu_product, idx, entries, seeds, own) > 0
        with pytest.raises(emu_product.MtgError):  # excluded entries must be ascending table numbers
            t = idx.targets(entries)
            try:
                idx.fill_seeds(t, [emu_product.Seed(seeds[0][1], [len(entries)])])
            finally:
                t.close()
    finally:
        idx.close()
