"""bench.py's plain run and --dump-outputs: the sites are decoded as SynthSet.site gives them, the dump holds what a caller of the fill
receives (records, and a fixed sample of the sequences) in float64 / float32 within its size limit, the same for the same result sets;
on the GPU, two plain runs with the same arguments dump the same arrays and time exactly one block of --steps steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (numpy only at import time)
from tests import emu_lib  # noqa: E402

NAMES = ("gap_records", "filled_records", "seq_sample", "seq_sample_index")


@pytest.mark.parametrize("kw", [dict(), dict(het_snps=4), dict(het_snps=4, het_indels=2), dict(tips=1.0 / 3.0)], ids=["haploid", "het", "indel", "tips"])
def test_site_triples_equal_synthset_sites(kw):
    from mindthegap_amd.synth import SynthSet
    S = SynthSet(nseq=2000, n_sites=900, seed=1, k=31, **kw)
    assert bench.site_triples(S, 0, 900, chunk=97) == [S.site(i) for i in range(900)]
    assert bench.site_triples(S, 300, 700) == [S.site(i) for i in range(300, 700)]


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.detail is None and a.dump_outputs is None and a.steps == 7
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.detail == os.path.join(ROOT, "bench_detail.json") and a.dump_outputs == "d"


@pytest.fixture(scope="module")
def emu_product():
    from mindthegap_amd import lib as L
    saved = L._lib
    yield emu_lib.product_on_emulator()
    L._lib = saved


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


def test_dump_outputs_on_the_emulator(emu_product, tmp_path):
    from mindthegap_amd import lib as L
    from mindthegap_amd.synth import SynthSet
    from tests import oracle_lib
    S = SynthSet(nseq=300, n_sites=200, seed=3, k=31)
    o = oracle_lib.Index.from_sequences([S.ascii(j) for j in range(S.nseq)], 31, 3, 0)
    km, ct = o.export()
    o.close()
    idx = emu_product.Index.from_kmers(km, ct, 31)
    sites = bench.site_triples(S, 0, 200)
    gaps = [emu_product.Gap(l, r, [(r, S.site_name(i), False)]) for i, (l, r, _ins) in enumerate(sites)]

    class B:
        gidx, n = 5, len(gaps)

    h, nf, seqs = idx.fill_prepared(emu_product.Index.prepare_gaps(gaps), want_seqs=True)
    try:
        for d in ("a", "b"):
            bench.dump_outputs(L._lib, [(B, h, None, np.zeros(0, dtype=np.int64))], str(tmp_path / d))
    finally:
        idx.free_results(h)
        idx.close()
    x, y = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(v.nbytes for v in x.values()) <= bench.DUMP_LIMIT
    for n in NAMES:
        assert x[n].dtype == (np.float32 if n == "seq_sample" else np.float64)
        assert np.array_equal(x[n], y[n])
    g, f = x["gap_records"], x["filled_records"]
    assert g.shape == (200, 12) and (g[:, 0] == 5).all() and (g[:, 1] == np.arange(200)).all() and (g[:, 2] == 0).all()
    assert (g[:, 9] == nf).all() and (nf == 1).all() and len(f) == 200 and (f[:, 0] == np.arange(200)).all()
    want = [s.encode() for s in seqs.tobytes().decode().split("\n")[:-1]]
    assert want == [ins.encode() for (_l, _r, ins) in sites]  # every site filled with its inserted sequence
    assert [int(v) for v in f[:, 9]] == [len(s) for s in want]
    assert [v for v in f[:, 10]] == [bench._hash48(s) for s in want]
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for row, off, ln in x["seq_sample_index"].astype(np.int64):
        assert acgt[x["seq_sample"][off:off + ln].astype(np.int64)].tobytes() == want[row]


@pytest.mark.gpu
def test_plain_runs_dump_the_same_outputs(tmp_path):
    lines = []
    for d in ("one", "two"):
        cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", "5", "--warmup", "2",
                             "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert cp.returncode == 0, cp.stderr[-2000:]
        lines.append(json.loads(cp.stdout.strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "breakpoints/s"
        assert line["value"] == pytest.approx(256 / (line["ms_per_step"] * 1e-3), rel=1e-3)
        assert line["cpu_baseline"] is None and line["detail"] is None
    x, y = _load(str(tmp_path / "one")), _load(str(tmp_path / "two"))
    for n in NAMES:
        assert np.array_equal(x[n], y[n]), n
    assert x["gap_records"].shape == (256, 12) and (x["gap_records"][:, 9] >= 1).all()
