"""The whole fill at k below 31 and with off-default limits, through the HIP kernels: the cases of tests/kfill_cases.py (which
tests/test_kfill_cpu.py runs on the emulator) against the oracle, plus the index built on the device from packed sequences as a second source of the
graph.  Bit-exact everywhere."""
import numpy as np
import pytest

from tests import kfill_cases as K, oracle_lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mtg():
    import torch
    torch.cuda.init()  # torch bundles its own HIP runtime: initialise it before libmtgfill.so touches the device
    import mindthegap_amd
    mindthegap_amd.load_library()
    assert mindthegap_amd.device_count() >= 1, "these tests need a HIP device"
    return mindthegap_amd


@pytest.mark.parametrize("het", [0, 2])
@pytest.mark.parametrize("k", K.BKPT_KS)
def test_bkpt_sweep(mtg, tmp_path, k, het):
    K.bkpt_sweep(mtg, tmp_path, k, het)


@pytest.mark.parametrize("host_format", [False, True])
@pytest.mark.parametrize("k", K.SHORT_KS)
def test_short_fills_every_alignment(mtg, tmp_path, monkeypatch, k, host_format):
    """through the device's formatter and through the host's writers"""
    if host_format:
        monkeypatch.setenv("MTG_HOST_FORMAT", "1")
    K.short_fills(mtg, tmp_path, k)


@pytest.mark.parametrize("k", K.MIS_KS)
def test_nb_mis_allowed(mtg, tmp_path, k):
    K.nb_mis_case(mtg, tmp_path, k)


@pytest.mark.parametrize("k", K.CONTIG_KS)
def test_contig_mode_sixteen_targets(mtg, tmp_path, monkeypatch, k):
    """with the shared target table and with a dictionary per seed (CONTIG_PER_SEED=1); k = 24 / 23: the piece index usable / not usable"""
    K.contig_case(mtg, tmp_path, k, monkeypatch, per_seed_too=True)


@pytest.mark.parametrize("k", K.TEXT_KS)
def test_text_entry(mtg, tmp_path, k):
    K.text_case(mtg, tmp_path, k)


def _revcomp(km, k):
    """reverse complements of k-mers in the index's code (A 0, C 1, T 2, G 3: the complement is code ^ 2; first nucleotide in the highest bits)"""
    km = km.astype(np.uint64)
    out = np.zeros_like(km)
    for i in range(k):
        out = (out << np.uint64(2)) | (((km >> np.uint64(2 * i)) & np.uint64(3)) ^ np.uint64(2))
    return out


@pytest.mark.parametrize("het", [0, 2])
@pytest.mark.parametrize("k", K.BKPT_KS)
def test_packed_built_index_as_the_graph_of_the_bkpt_sweep(mtg, tmp_path, k, het):
    """mtg_index_create_from_packed_device at k: the sequences of the sweep's set (for even k plus one that holds a k-mer equal to its own reverse
    complement) packed on the device; statistics, contains / abundance / neighbourhood of every k-mer of the set, of their reverse complements,
    of their eight neighbours and of 5 000 random k-mers against the oracle; then the sweep with a container saved from that index."""
    import torch
    S, seqs = K.bkpt_set(k, het)
    rng = np.random.default_rng(k)
    pal = None
    if k % 2 == 0:
        half = "".join("ACGT"[c] for c in rng.integers(0, 4, k // 2))
        pal = half + half[::-1].translate(str.maketrans("ACGT", "TGCA"))
        rand = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))
        seqs = seqs + [rand(100) + pal + rand(100)]
    o = oracle_lib.Index.from_sequences(seqs, k, 3, 40)
    words, off, lens = K.pack_sequences(seqs)
    words = np.concatenate([words, np.zeros(2, dtype=np.uint64)])
    w = torch.from_numpy(words.view(np.int64)).cuda()
    wo = torch.from_numpy(off.view(np.int64)).cuda()
    ln = torch.from_numpy(lens.view(np.int32)).cuda()
    ub = int(np.maximum(lens.astype(np.int64) - (k - 1), 0).sum())
    g = mtg.Index.from_packed_device(w.data_ptr(), wo.data_ptr(), ln.data_ptr(), len(seqs), ub, k, 3, 40)
    info = g.info()
    assert info["k"] == k and (info["nb_solid_kmers"], info["nb_branching"]) == o.stats()
    km, _ = o.export()
    M = np.uint64((1 << (2 * k)) - 1)
    if pal is not None:
        code = 0
        for c in pal:
            code = (code << 2) | "ACTG".index(c)
        assert _revcomp(np.array([code], dtype=np.uint64), k)[0] == code and o.contains(np.array([code], dtype=np.uint64))[0] == 1

    def neighbours(x):
        succ = ((x[:, None] << np.uint64(2)) & M) | np.arange(4, dtype=np.uint64)[None, :]
        pred = (x[:, None] >> np.uint64(2)) | (np.arange(4, dtype=np.uint64)[None, :] << np.uint64(2 * (k - 1)))
        return succ, pred

    rc = _revcomp(km, k)
    succ, pred = neighbours(km)
    q = np.concatenate([km, rc, succ.reshape(-1), pred.reshape(-1), rng.integers(0, 1 << (2 * k), 5000, dtype=np.uint64)])
    assert (g.contains(q) == o.contains(q)).all()
    assert (g.abundance(q) == o.abundance(q)).all()
    assert o.contains(rc).all()
    for x in (km, rc):
        s, p = g.neighbors(x)
        xs, xp = neighbours(x)
        es = (o.contains(xs.reshape(-1)).reshape(-1, 4) * (1 << np.arange(4))).sum(1)
        ep = (o.contains(xp.reshape(-1)).reshape(-1, 4) * (1 << np.arange(4))).sum(1)
        assert (s == es).all() and (p == ep).all()
    idxf = str(tmp_path / "packed.mtgidx")
    g.save(idxf)
    g.close()
    del w, wo, ln
    K.bkpt_sweep(mtg, tmp_path, k, het, index_file=idxf, oracle=o)
    o.close()
