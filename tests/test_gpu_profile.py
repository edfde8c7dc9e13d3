"""The sequence profile on the device (k_profile, k_profile_count / _seq_scan / _write / _finish in csrc/mtg_gpu_misc.hip behind
mtg_index_profile_sequences / _packed_device) against a plain model (tests/profile_cases.py) and against the index's own point queries
(Index.contains / abundance / neighbors): words and runs, all compared exactly.

tests/golden/full_test/reference.fasta is a data fixture: the reference genome of the reference's full test (its data/reference.fasta), the one
its `find` ran on to produce gold.breakpoints."""
import os
import subprocess

import numpy as np
import pytest

from tests import profile_cases as pc
from tests import reads_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FASTQ_PAIR = [os.path.join(GOLDEN, "data", "reads_r1.fastq"), os.path.join(GOLDEN, "data", "reads_r2.fastq")]
REFERENCE = os.path.join(GOLDEN, "full_test", "reference.fasta")
BKPT = os.path.join(GOLDEN, "full_test", "gold.breakpoints")
K, CUTOFF = 31, 7


@pytest.fixture(scope="module")
def mtg():
    import torch
    torch.cuda.init()  # torch bundles its own HIP runtime: initialise it before libmtgfill.so touches the device
    import mindthegap_amd
    mindthegap_amd.load_library()
    assert mindthegap_amd.device_count() >= 1, "these tests need a HIP device"
    return mindthegap_amd


@pytest.fixture(scope="module")
def reads_solid():
    solid = pc.solid_of_files(FASTQ_PAIR, K, CUTOFF)
    assert len(solid) == 7419  # the golden's solid k-mers (tests/golden/full_test/gold_fill.output)
    return solid


@pytest.fixture(scope="module")
def reads_index(mtg):
    idx = mtg.Index.from_reads(FASTQ_PAIR, K, CUTOFF)
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def reference():
    return pc.read_fasta(REFERENCE)


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


class Planted:
    """an index from explicit k-mers: about 2 000 random ones plus the k-mers of a few chains (random strings every k-mer of which is solid),
    abundances 1 .. 255"""

    def __init__(self, mtg, k, seed):
        rng = np.random.default_rng(seed)
        self.k = k
        self.chains = [rand_seq(rng, n) for n in (1500, 400, 90)]
        kms = set(rc.canon(int(x), k) for x in rng.integers(0, 1 << (2 * k), 2000, dtype=np.uint64))
        for c in self.chains:
            for p in range(len(c) - k + 1):
                kms.add(rc.canon(rc.encode(c[p:p + k]), k))
        kms = sorted(kms)
        ab = rng.integers(1, 256, len(kms))
        ab[::7] = 255
        self.solid = {x: int(a) for x, a in zip(kms, ab)}
        self.idx = None if mtg is None else mtg.Index.from_kmers(np.array(kms, dtype=np.uint64), ab.astype(np.uint32), k)
        self.rng = rng


@pytest.fixture(scope="module")
def planted31(mtg):
    p = Planted(mtg, 31, 31)
    yield p
    p.idx.close()


def check_profile(idx, solid, k, seqs, against_queries=False):
    """profile seqs and compare words, runs and statistics with the model; returns (words, runs, stats)"""
    words, runs, st = idx.profile_sequences(seqs)
    want_words, want_runs = pc.profile(solid, k, seqs)
    assert len(words) == len(seqs)
    for s, (got, want) in enumerate(zip(words, want_words)):
        assert got.dtype == np.uint32 and len(got) == len(want), (s, len(got), len(want))
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, "sequence %d (length %d): position %d: word %#x, expected %#x (%d positions differ)" % (s, len(seqs[s]), bad[0], got[bad[0]], want[bad[0]], len(bad))
    assert runs.dtype == pc.RUN_DTYPE and runs.tolist() == want_runs.tolist()
    allw = np.concatenate(want_words) if want_words else np.zeros(0, np.uint32)
    assert st["n_positions"] == len(allw) and st["n_valid"] == int(((allw >> 16) & 1).sum()) and st["n_present"] == int(((allw >> 17) & 1).sum())
    assert st["n_runs"] == len(want_runs) and st["longest_run"] == (int(want_runs["length"].max()) if len(want_runs) else 0)
    if against_queries:  # the same forward k-mers through the point queries, masked to 0 where absent
        import mindthegap_amd as m
        for s, seq in enumerate(seqs):
            up = seq.upper()
            pos = [p for p in range(len(seq) - k + 1) if "N" not in up[p:p + k]]
            if not pos:
                continue
            q = np.array([rc.encode(up[p:p + k]) for p in pos], dtype=np.uint64)
            has, ab = idx.contains(q), idx.abundance(q)
            su, pr = idx.neighbors(q)
            w = words[s][pos]
            assert (m.profile_valid(w) == 1).all()
            assert (m.profile_present(w) == has).all() and (m.profile_abundance(w) == np.minimum(ab, 255)).all()
            assert (m.profile_succ(w) == np.where(has == 1, su, 0)).all() and (m.profile_pred(w) == np.where(has == 1, pr, 0)).all()
            inv = np.setdiff1d(np.arange(len(words[s])), pos)
            assert (words[s][inv] == 0).all()
    return words, runs, st


def synthetic(rng, sources, k, n):
    """n strings cut from the sources (mostly present), some mutated, some with an N or lower case, some random"""
    out = []
    for i in range(n):
        src = sources[int(rng.integers(len(sources)))]
        ln = int(rng.integers(k - 2, min(len(src), 260)))
        a = int(rng.integers(0, len(src) - ln + 1))
        s = list(src[a:a + ln])
        if i % 3 == 0 and ln:
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(ln))] = "ACGT"[int(rng.integers(4))]
        if i % 5 == 0 and ln:
            s[int(rng.integers(ln))] = "Nn"[i % 2]
        if i % 4 == 0:
            s = [c.lower() if rng.integers(3) == 0 else c for c in s]
        if i % 17 == 0:
            s = list(rand_seq(rng, ln))
        out.append("".join(s))
    return out


# ------------------------------------------------------------------------------------------------ 1. words
def test_words_of_the_reference_and_synthetic_strings(mtg, reads_index, reads_solid, reference):
    rng = np.random.default_rng(1)
    reads = [r.decode() for r in rc.read_records(FASTQ_PAIR[0])[:400]]
    seqs = [s for _, s in reference] + synthetic(rng, reads + [s for _, s in reference], K, 200)
    words, runs, st = check_profile(reads_index, reads_solid, K, seqs, against_queries=True)
    assert st["n_present"] > 3000 and len(runs) > 40  # the reference is mostly in the graph, with the variant sites absent


@pytest.mark.parametrize("k", [11, 21, 31])
def test_words_for_other_k(mtg, k):
    p = Planted(mtg, k, 100 + k)
    try:
        seqs = p.chains[1:] + synthetic(p.rng, p.chains, k, 150)
        words, runs, st = check_profile(p.idx, p.solid, k, seqs, against_queries=True)
        assert st["n_present"] > 500 and st["n_valid"] > st["n_present"]
    finally:
        p.idx.close()


# ------------------------------------------------------------------------------------------------ 2. shapes
def test_lengths_around_the_seams(mtg, reads_index, reads_solid, reference):
    ref = "".join(s for _, s in reference)
    lens = [K - 1, K, K + 1, K + 62, K + 63, K + 64, K + 254, K + 255, K + 256, K + 257, 3 * 256 + K + 5]
    seqs = [ref[100 + 7 * i:100 + 7 * i + n] for i, n in enumerate(lens)] + ["", "A", ref[:K - 1]]
    words, runs, st = check_profile(reads_index, reads_solid, K, seqs)
    assert [len(w) for w in words[:len(lens)]] == [0, 1, 2, 63, 64, 65, 255, 256, 257, 258, 3 * 256 + 6]


def test_invalid_and_lower_case_characters_at_the_seams(mtg, reads_index, reads_solid, reference):
    base = reference[2][1][:600]
    offs = sorted(set([0, K - 1] + [s + d for s in (64, 128, 256, 512) for d in (-1, 0, 1)] + [s - K + d for s in (64, 256) for d in (0, 1)]))
    seqs = []
    for o in offs:
        seqs.append(base[:o] + "N" + base[o + 1:])
        seqs.append(base[:o] + base[o].lower() + base[o + 1:])
    seqs.append(base[:300] + "n" + base[301:305] + "N" + base[306:])
    seqs.append("N" * 40 + base[:40])
    words, runs, st = check_profile(reads_index, reads_solid, K, seqs)
    for i in range(len(offs)):  # lower case changes nothing; an N blanks exactly the k-mers that cover it
        assert (words[2 * i + 1] == words[1]).all()
        o = offs[i]
        lo, hi = max(o - K + 1, 0), min(o, len(words[2 * i]) - 1)
        assert (words[2 * i][lo:hi + 1] == 0).all() and (words[2 * i][:lo] == words[1][:lo]).all() and (words[2 * i][hi + 1:] == words[1][hi + 1:]).all()


def test_no_sequences(mtg, reads_index):
    words, runs, st = reads_index.profile_sequences([])
    assert words == [] and len(runs) == 0 and st["n_positions"] == 0 and st["n_runs"] == 0
    words, runs, st = reads_index.profile_sequences(["", "ACGT"], want_positions=False)
    assert words is None and len(runs) == 0 and st["n_positions"] == 0


def test_more_sequences_than_workgroups(mtg, planted31):
    """4 500 sequences of k characters (a launch has at most 4 096 workgroups, each striding over the sequences), half of them solid"""
    p = planted31
    rng = np.random.default_rng(5)
    c = p.chains[0]
    seqs = [c[a:a + K] if i % 2 else rand_seq(rng, K) for i, a in enumerate(rng.integers(0, len(c) - K + 1, 4500))]
    words, runs, st = check_profile(p.idx, p.solid, K, seqs)
    assert st["n_present"] == 2250 and st["n_runs"] == 2250 and (runs["seq"] == np.arange(0, 4500, 2)).all() and (runs["flags"] == 0).all()


def test_all_absent_and_all_present(mtg, planted31):
    p = planted31
    rng = np.random.default_rng(6)
    seqs = [rand_seq(rng, 900), p.chains[0], rand_seq(rng, K), p.chains[2]]
    words, runs, st = check_profile(p.idx, p.solid, K, seqs)
    assert runs.tolist() == [(0, 0, 900 - K + 1, 0), (2, 0, 1, 0)]
    assert (mtg.profile_present(words[1]) == 1).all() and (mtg.profile_present(words[3]) == 1).all()
    # inside a chain every k-mer has its one successor and its one predecessor (the random k-mers of the index may add a second one)
    assert (mtg.profile_succ(words[1][:-1]) != 0).all() and (mtg.profile_pred(words[1][1:]) != 0).all()


# ------------------------------------------------------------------------------------------------ 3. runs
def flank(rng, n, first_not=None, last_not=None):
    """n random nucleotides that do not continue a chain: the first is not first_not, the last is not last_not"""
    s = list(rand_seq(rng, n))
    if first_not is not None:
        s[0] = [x for x in "ACGT" if x != first_not][int(rng.integers(3))]
    if last_not is not None:
        s[-1] = [x for x in "ACGT" if x != last_not][int(rng.integers(3))]
    return "".join(s)


def run_cases(p, rng):
    c = p.chains[0]
    return {
        "at_start": flank(rng, 40) + c[0:100],
        "at_end": c[0:100] + flank(rng, 40, first_not=c[100]),
        "split_by_n": c[0:80] + flank(rng, 45, first_not=c[80]) + "N" + flank(rng, 45, last_not=c[99]) + c[100:180],
        "one_present": flank(rng, 50, last_not=c[199]) + c[200:200 + K] + flank(rng, 50, first_not=c[200 + K]),
        "long": c[0:60] + flank(rng, 700, first_not=c[60], last_not=c[299]) + c[300:360],
    }


def test_run_bounds_and_flags(mtg, planted31):
    p = planted31
    cases = run_cases(p, np.random.default_rng(7))
    names = list(cases)
    words, runs, st = check_profile(p.idx, p.solid, K, [cases[n] for n in names])
    by = {n: [tuple(int(x) for x in r)[1:] for r in runs if r["seq"] == i] for i, n in enumerate(names)}
    assert by["at_start"] == [(0, 40, 2)]                           # no position before it: no L flag
    assert by["at_end"] == [(100 - K + 1, 40, 1)]                   # reaches the last position: no R flag
    # around the N the 31 k-mers that cover it are invalid: two runs, neither bounded on that side
    assert by["split_by_n"] == [(80 - K + 1, 45, 1), (80 + 45 + 1, 45, 2)]
    assert by["one_present"] == [(0, 50, 2), (51, 50, 1)]           # both flagged towards the one solid k-mer at position 50
    assert by["long"] == [(60 - K + 1, 700 + K - 1, 3)] and st["longest_run"] == 700 + K - 1


def test_run_order_capacity_and_runs_only(mtg, planted31):
    p = planted31
    rng = np.random.default_rng(8)
    c = p.chains[0]
    seqs = list(run_cases(p, rng).values())
    for i in range(300):  # present and absent stretches in turn, now and then an N, a sequence without runs, one too short
        parts = []
        for j in range(int(rng.integers(1, 7))):
            a = int(rng.integers(0, len(c) - 200))
            parts.append(c[a:a + int(rng.integers(K, 200))] if (i + j) % 2 else rand_seq(rng, int(rng.integers(1, 120))))
            if rng.integers(6) == 0:
                parts.append("N")
        seqs.append("".join(parts))
    seqs += [c[:300], "ACG"]
    words, runs, st = check_profile(p.idx, p.solid, K, seqs)
    n = len(runs)
    assert n > 400
    key = runs["seq"].astype(np.int64) * (1 << 32) + runs["start"]
    assert (np.diff(key) > 0).all()
    for cap in (0, 1, n - 1, n, n + 5):
        w2, r2, st2 = p.idx.profile_sequences(seqs, runs_cap=cap)
        assert st2["n_runs"] == n and len(r2) == min(cap, n) and r2.tolist() == runs[:cap].tolist() and st2["longest_run"] == st["longest_run"]
        assert all((a == b).all() for a, b in zip(w2, words))
    w3, r3, st3 = p.idx.profile_sequences(seqs, want_positions=False)
    assert w3 is None and r3.tolist() == runs.tolist() and {x: st3[x] for x in st3 if x != "kernel_ms"} == {x: st[x] for x in st if x != "kernel_ms"}


# ------------------------------------------------------------------------------------------------ 4. packed sequences in device memory
def test_packed_device_entry_equals_the_host_entry(mtg, planted31):
    import torch
    p = planted31
    rng = np.random.default_rng(9)
    c = p.chains[0]
    seqs = [s for s in run_cases(p, rng).values() if "N" not in s] + [c, rand_seq(rng, 30), rand_seq(rng, 31), c[5:5 + 64 + K], c[9:9 + 256 + K - 1] + rand_seq(rng, 300)]
    words, runs, st = check_profile(p.idx, p.solid, K, seqs)
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    word_off = np.zeros(len(seqs), dtype=np.uint64)
    pos_off = np.zeros(len(seqs), dtype=np.uint64)
    nw = npos = 0
    for i, n in enumerate(lens):
        word_off[i], pos_off[i] = nw, npos
        nw += (int(n) + 31) // 32 + 1
        npos += max(int(n) - K + 1, 0)
    packed = np.zeros(nw + 1, dtype=np.uint64)
    for i, s in enumerate(seqs):
        for j, ch in enumerate(s):
            packed[int(word_off[i]) + (j >> 5)] |= np.uint64(((ord(ch) >> 1) & 3) << (2 * (j & 31)))
    dev = torch.device("cuda", 0)
    d_w = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_wo = torch.from_numpy(word_off.view(np.int64)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_po = torch.from_numpy(pos_off.view(np.int64)).to(dev)
    for cap in (len(runs) + 3, len(runs), 2, 0):
        d_out = torch.full((npos + 1,), -1, dtype=torch.int32, device=dev)
        d_runs = torch.full((max(cap, 1) * 4 + 4,), -1, dtype=torch.int32, device=dev)
        total, st2 = p.idx.profile_packed_device(d_w.data_ptr(), d_wo.data_ptr(), d_ln.data_ptr(), len(seqs), d_po.data_ptr(), d_out.data_ptr(), d_runs.data_ptr() if cap else None, cap)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(np.uint32)
        assert (got[:npos] == np.concatenate(words)).all() and got[npos] == 0xFFFFFFFF
        r = d_runs.cpu().numpy().view(np.uint32)
        n = min(cap, len(runs))
        assert total == len(runs) and r[:4 * n].view(pc.RUN_DTYPE).tolist() == runs[:n].tolist()
        assert (r[4 * n:] == 0xFFFFFFFF).all()  # nothing behind the runs that were asked for
        assert {x: st2[x] for x in st2 if x != "kernel_ms"} == {x: st[x] for x in st if x != "kernel_ms"}
    total, st2 = p.idx.profile_packed_device(d_w.data_ptr(), d_wo.data_ptr(), d_ln.data_ptr(), len(seqs), None, None, None, 0)  # runs-only, counted
    assert total == len(runs) and st2["n_present"] == st["n_present"]


# ------------------------------------------------------------------------------------------------ 5. the reference's goldens
def test_homozygous_sites_of_the_golden_are_bounded_runs(mtg, reads_index, reads_solid, reference):
    """Each HOM record of gold.breakpoints (the reference's `find` on this reference and these reads) names a run bounded on both sides: with
    fuzzy = the size of the repeat at the site, the run has k - 1 - fuzzy positions, ends fuzzy positions before pos, and the k-mer before it
    is the record's left k-mer.  Checked with the model at cut-off 7 before it was asserted: Seq2/535, Seq2/835 and Seq4/603 hold on all three
    conditions.  Seq3/781 has its run end at pos but the run is 46 positions long (a second variant 16 nt upstream merges into it), and no run
    ends at Seq4/821 (the run there spans 791 .. 840): those two are not clean insertion sites of the plain profile, and classifying them is
    `find`'s work, not the profile's.  They are asserted as the model gives them."""
    names = [n for n, _ in reference]
    words, runs, st = check_profile(reads_index, reads_solid, K, [s for _, s in reference])
    recs = pc.gold_hom_records(BKPT)
    assert [(n, p) for n, p, _, _ in recs] == [("Seq2", 535), ("Seq2", 835), ("Seq3", 781), ("Seq4", 603), ("Seq4", 821)]
    clean = 0
    for name, pos, fuzzy, left in recs:
        s = names.index(name)
        seq = reference[s][1]
        hit = [r for r in runs if r["seq"] == s and r["flags"] == 3 and int(r["start"]) + int(r["length"]) + fuzzy == pos]
        if (name, pos) == ("Seq4", 821):
            assert hit == [] and [(int(r["start"]), int(r["length"]), int(r["flags"])) for r in runs if r["seq"] == s and r["start"] <= 821 < r["start"] + r["length"]] == [(791, 50, 3)]
            continue
        assert len(hit) == 1
        start, length = int(hit[0]["start"]), int(hit[0]["length"])
        if (name, pos) == ("Seq3", 781):
            assert (start, length) == (735, 46)
            continue
        assert length == K - 1 - fuzzy and seq[start - 1:start - 1 + K].upper() == left
        clean += 1
    assert clean == 3


# ------------------------------------------------------------------------------------------------ 6. the tool
def test_profile_tool_writes_the_runs_as_bed(mtg, reads_solid, reference, tmp_path):
    exe = os.path.join(os.path.dirname(mtg.build_library()), "MindTheGap")
    out = str(tmp_path / "prof")
    r = subprocess.run([exe, "profile", "-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-abundance-min", str(CUTOFF), "-out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want_words, want_runs = pc.profile(reads_solid, K, [s for _, s in reference])
    flag = {0: ".", 1: "L", 2: "R", 3: "LR"}
    want = ["%s\t%d\t%d\t%d\t%s" % (reference[r["seq"]][0], r["start"], int(r["start"]) + int(r["length"]), r["length"], flag[int(r["flags"])]) for r in want_runs]
    assert open(out + ".absent.bed").read().splitlines() == want
    stats = dict(l.split(" : ") for l in open(out + ".profile.txt").read().splitlines())
    allw = np.concatenate(want_words)
    assert int(stats["kmer_size"]) == K and int(stats["nb_solid_kmers"]) == 7419 and int(stats["nb_sequences"]) == len(reference)
    assert int(stats["nb_positions"]) == len(allw) and int(stats["nb_present"]) == int(((allw >> 17) & 1).sum()) and int(stats["nb_runs"]) == len(want_runs)
    assert int(stats["longest_run"]) == int(want_runs["length"].max())
    assert sorted(os.listdir(str(tmp_path))) == ["prof.absent.bed", "prof.profile.txt"]
    # the module through the library's entry: same bytes
    assert mtg.profile_main(["-in", ",".join(FASTQ_PAIR), "-ref", REFERENCE, "-abundance-min", str(CUTOFF), "-out", out + "2"]) == 0
    assert open(out + "2.absent.bed").read() == open(out + ".absent.bed").read()


def test_fill_module_of_the_tool_is_unchanged(mtg, tmp_path):
    exe = os.path.join(os.path.dirname(mtg.build_library()), "MindTheGap")
    out = str(tmp_path / "fill")
    r = subprocess.run([exe, "fill", "-in", ",".join(FASTQ_PAIR), "-bkpt", BKPT, "-abundance-min", str(CUTOFF), "-out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out + ".insertions.fasta").read() == open(os.path.join(GOLDEN, "full_test", "gold.insertions.fasta")).read()
