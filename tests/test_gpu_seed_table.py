"""Contig mode with ONE shared target table on the device (mtg_targets_create / mtg_fill_seeds) instead of a dictionary per seed: the same
results as the per-seed dictionaries of the reference (src/Filler.cpp:522-533), through the C ABI and through the tool."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mtg():
    import torch
    torch.cuda.init()  # torch bundles its own HIP runtime: initialise it before libmtgfill.so touches the device
    import mindthegap_amd
    mindthegap_amd.load_library()
    if mindthegap_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return mindthegap_amd


def _read(p):
    with open(p) as f:
        return f.read()


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def _table_of_contigs(path, k=31, trim=0):
    """run_contig's dictionary of all targets (src/Filler.cpp:755-829) in table order -- the order of its insertions here; the tool's own order
    is that of a std::unordered_map, which fill_seeds does not need -- and its seeds with the entries of their own contig"""
    recs, name = [], None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:].split()[0]
            recs.append([name, ""])
        elif line:
            recs[-1][1] += line
    entries, seeds, seen = [], [], set()
    for name, c in recs:
        if len(c) <= 2 * trim + k:
            continue
        rc = _revcomp(c)
        for key, is_rc in ((c[trim:trim + k], False), (rc[trim:trim + k], True)):
            if key not in seen:
                seen.add(key)
                entries.append((key, name, is_rc))
        seeds.append((name, c[len(c) - (trim + k):len(c) - trim]))
        seeds.append((name + "_Rc", rc[len(rc) - (trim + k):len(rc) - trim]))
    own = {}
    for i, (key, name, is_rc) in enumerate(entries):
        own.setdefault(name + "_Rc" if is_rc else name, []).append(i)
    return entries, seeds, own


def _compare_with_fill_batch(mtg, idx, entries, seeds, own):
    from mindthegap_amd import Gap, Seed
    t = idx.targets(entries)
    try:
        got = idx.fill_seeds(t, [Seed(src, own.get(nm, ())) for nm, src in seeds])
    finally:
        t.close()
    gaps, maps = [], []
    for nm, src in seeds:
        ex = set(own.get(nm, ()))
        keep = [i for i in range(len(entries)) if i not in ex]
        gaps.append(Gap(src, "".join(entries[i][0] for i in keep), [entries[i] for i in keep]))
        maps.append(keep)
    want = idx.fill_batch(gaps)
    nsol = 0
    for s, (a, b, m) in enumerate(zip(got, want, maps)):
        for f in b["filled"]:
            f["target_index"] = m[f["target_index"]]
        assert a == b, "seed %d (%s)" % (s, seeds[s][0])
        nsol += len(a["filled"])
    return nsol


def test_bundled_contig_case_fill_seeds_and_tool(mtg, tmp_path):
    """the reference's own contig case: every seed through fill_seeds equals fill_batch with its explicit dictionary (target numbers mapped to the
    table's); the tool, which now hands the dictionary over once, still writes gold.gfa"""
    reads = os.path.join(G, "data", "contig-reads.fasta.gz")
    contigs = os.path.join(G, "data", "contigs.fasta")
    idx = mtg.Index.from_reads([reads], 31, 3)
    try:
        entries, seeds, own = _table_of_contigs(contigs)
        assert len(entries) >= 16  # the table path (a piece index needs sixteen entries)
        assert _compare_with_fill_batch(mtg, idx, entries, seeds, own) > 0
        assert idx.fill_main(["-contig", contigs, "-out", str(tmp_path / "b")]) == 0
    finally:
        idx.close()
    assert _read(str(tmp_path / "b.gfa")) == _read(os.path.join(G, "contig_test", "gold.gfa"))


@pytest.mark.parametrize("mutate", [False, True])
def test_two_hundred_contigs_tool_and_fill_seeds_equal_oracle(mtg, tmp_path, mutate):
    """the _contig_gap_case shape (every donor sequence cut into two contigs around a hole) at 200 contigs, with and without mutated targets:
    the tool's files equal the oracle's, and fill_seeds equals fill_batch seed by seed"""
    from tests.test_emu_parity import _contig_gap_case
    _contig_gap_case(mtg, tmp_path, 100, mutate=mutate)
    from mindthegap_amd.synth import SynthSet
    S = SynthSet(nseq=100, n_sites=100, seed=31)
    o = oracle_lib.Index.from_sequences([S.ascii(j) for j in range(S.nseq)], 31, 3, 40)
    km, ct = o.export()
    o.close()
    idx = mtg.Index.from_kmers(km, ct, 31)
    try:
        entries, seeds, own = _table_of_contigs(str(tmp_path / "contigs.fa"))
        assert _compare_with_fill_batch(mtg, idx, entries, seeds, own) >= 100
    finally:
        idx.close()


def test_constructed_ties_equal_oracle(mtg, tmp_path, capfd):
    """ties: for every hole, two right contigs whose target k-mers differ from the donor in ONE place each, at different places -- the fill matches
    both with one difference at the same position, and the reference keeps the first of them in the seed's own dictionary order.  The device
    decides by table rank and flags those seeds; the host re-decides them.  Files must equal the oracle's with the full dictionary."""
    from mindthegap_amd.synth import SynthSet
    S = SynthSet(nseq=24, n_sites=24, seed=5)
    seqs = [S.ascii(j) for j in range(S.nseq)]
    o = oracle_lib.Index.from_sequences(seqs, 31, 3, 40)
    km, ct = o.export()
    contigs = str(tmp_path / "contigs.fa")

    def sub(t, i):
        return t[:i] + ("A" if t[i] != "A" else "C") + t[i + 1:]
    rng = np.random.default_rng(3)
    with open(contigs, "w") as f:
        for j, s in enumerate(seqs):
            p, L = int(S.pos[j]), int(S.ins_len[j])
            right = s[p + L:]
            # (the tool's targets are contig[31:62]: the trim of -overlap 31 comes first)
            a, b = sorted(rng.choice(31, 2, replace=False))
            tail = "".join("ACGT"[x] for x in rng.integers(0, 4, 200))
            f.write(">c%dL\n%s\n>c%dR\n%s\n>c%dT\n%s\n" % (j, s[:p], j, sub(right, 31 + int(a)), j, sub(right[:62], 31 + int(b)) + tail))
    idx = mtg.Index.from_kmers(km, ct, 31)
    try:
        o.fill_files("contig", contigs, str(tmp_path / "cpu"), params=oracle_lib.default_params(nb_cores=4))
        capfd.readouterr()
        mtg.tuning_set("DEBUG_TIMERS", "1")
        try:
            assert idx.fill_main(["-contig", contigs, "-out", str(tmp_path / "hip")]) == 0
        finally:
            mtg.tuning_set("DEBUG_TIMERS", "")
    finally:
        idx.close()
        o.close()
    err = capfd.readouterr().err
    line = [l for l in err.splitlines() if "[fill_seeds]" in l]
    assert line, err[-2000:]
    sys.stderr.write(line[0] + "\n")
    assert int(line[0].split(" of them with a tie")[0].split()[-1]) >= 12  # the device flagged the ties (both orientations of a hole can meet one)
    for ext in (".info.txt", ".gfa", ".insertions.fasta"):
        assert sorted(_read(str(tmp_path / ("hip" + ext))).splitlines()) == sorted(_read(str(tmp_path / ("cpu" + ext))).splitlines()), ext
    nfill = sum(1 for l in _read(str(tmp_path / "hip.gfa")).splitlines() if l.startswith("S") and ";" in l)
    assert nfill >= 24


def _synthetic_contigs(path, n, seed=11):
    """scripts/r6_contig_workload.py's donor: 5 kb sequences, three contigs each with gaps of 200-800 nt between them"""
    from mindthegap_amd.synth import SynthSet
    nseq = (n + 2) // 3
    S = SynthSet(nseq=nseq, n_sites=0, seed=seed, k=31)
    rng = np.random.default_rng(12)
    nc = 0
    with open(path, "w") as f:
        for j in range(nseq):
            s = S.ascii(j)
            g1, g2 = int(rng.integers(200, 801)), int(rng.integers(200, 801))
            L = (len(s) - g1 - g2) // 3
            for (b, e) in [(0, L), (L + g1, 2 * L + g1), (2 * L + g1 + g2, len(s))]:
                if nc < n:
                    f.write(">c%d\n%s\n" % (nc, s[b:e]))
                    nc += 1
    return S


def test_two_thousand_contigs_shared_table_equals_per_seed_path(mtg, tmp_path):
    """2 000 synthetic contigs: every file of the tool is byte-identical between the shared table and CONTIG_PER_SEED=1 (a dictionary per seed)"""
    cf = str(tmp_path / "contigs.fa")
    S = _synthetic_contigs(cf, 2000)
    o = oracle_lib.Index.from_sequences([S.ascii(j) for j in range(S.nseq)], 31, 3, 0)
    km, ct = o.export()
    o.close()
    idx = mtg.Index.from_kmers(km, ct, 31)
    try:
        t0 = time.perf_counter()
        assert idx.fill_main(["-contig", cf, "-out", str(tmp_path / "table")]) == 0
        t_table = time.perf_counter() - t0
        mtg.tuning_set("CONTIG_PER_SEED", "1")
        try:
            t0 = time.perf_counter()
            assert idx.fill_main(["-contig", cf, "-out", str(tmp_path / "perseed")]) == 0
            t_per_seed = time.perf_counter() - t0
        finally:
            mtg.tuning_set("CONTIG_PER_SEED", "")
    finally:
        idx.close()
    for ext in (".insertions.fasta", ".info.txt", ".gfa", "_seed_dictionary.fasta"):
        a, b = _read(str(tmp_path / ("table" + ext))), _read(str(tmp_path / ("perseed" + ext)))
        assert a == b, ext
    assert sum(1 for l in _read(str(tmp_path / "table.gfa")).splitlines() if l.startswith("L\t")) > 1000
    sys.stderr.write("[2 000 contigs] shared table %.3f s, per-seed dictionaries %.3f s\n" % (t_table, t_per_seed))


def test_table_device_memory_is_linear(mtg):
    """the table's device memory is O(T): 16 bytes of encoded key, the packed key text and one piece index (4 (cap + 4 T) bytes) per entry"""
    from mindthegap_amd import Seed
    rng = np.random.default_rng(1)
    S_n = 199998
    keys = ["".join("ACGT"[x] for x in row) for row in rng.integers(0, 4, (S_n, 31))]
    idx = mtg.Index.from_kmers(np.arange(1, 1000, dtype=np.uint64), np.full(999, 5, dtype=np.uint32), 31)
    try:
        t = idx.targets([(k, "c%d" % (i // 2), bool(i & 1)) for i, k in enumerate(keys)])
        try:
            res = idx.fill_seeds(t, [Seed(keys[0], [0, 1])])  # the piece index is made by the first fill
            assert len(res) == 1
            b = t.device_bytes()
        finally:
            t.close()
    finally:
        idx.close()
    sys.stderr.write("[table] %d entries: %.1f MB of device memory\n" % (S_n, b / 1e6))
    assert b < 64 * S_n + (1 << 22)


def test_contigs_100k(mtg, tmp_path):
    """100 000 contigs (200 000 seeds x 199 998 targets) on a resident index: the tool completes, and the info rows, FASTA records and GFA links of a
    sample of the seeds (the oracle with the FULL dictionary) equal the oracle's.  Records wall time and seeds/s."""
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "r6_contig_workload.py"), "--contigs", "100000", "--oracle-stride", "20000", "--repeats", "1",
                         "--label", "100k"], capture_output=True, text=True, timeout=900)
    assert cp.returncode == 0, cp.stderr[-3000:]
    out = json.loads(cp.stdout.strip().splitlines()[-1])
    sys.stderr.write("[100 000 contigs] %s\n" % json.dumps({k: out.get(k) for k in ("seeds", "seconds", "value", "oracle_sample")}))
    assert out["contigs"] == 100000 and out["seeds"] == 200000
    assert out["oracle_sample"]["seeds"] >= 5 and out["identical_to_oracle"], out["oracle_sample"]


def test_two_devices_same_files(mtg, tmp_path):
    """-nb-gpus 2 (one table per replica) writes the same files as one device"""
    if mtg.device_count() < 2:
        pytest.skip("one device")
    cf = str(tmp_path / "contigs.fa")
    S = _synthetic_contigs(cf, 600, seed=7)
    o = oracle_lib.Index.from_sequences([S.ascii(j) for j in range(S.nseq)], 31, 3, 0)
    km, ct = o.export()
    o.close()
    idx = mtg.Index.from_kmers(km, ct, 31)
    try:
        assert idx.fill_main(["-contig", cf, "-out", str(tmp_path / "one"), "-nb-gpus", "1"]) == 0
        assert idx.fill_main(["-contig", cf, "-out", str(tmp_path / "two"), "-nb-gpus", "2"]) == 0
    finally:
        idx.close()
    for ext in (".insertions.fasta", ".info.txt", ".gfa"):
        assert _read(str(tmp_path / ("one" + ext))) == _read(str(tmp_path / ("two" + ext))), ext
