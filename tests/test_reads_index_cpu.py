"""The index built from read files (`-in`) against a plain k-mer count, on the CPU: the plain reference itself is pinned to the
reference project's numbers, then judges the oracle and the product on the emulator (tests/reads_cases.py has the cases).

On the emulator FileReadStream, kmer_from_ascii, count_insert and index_from_reads' option handling are the product's own code; the
construction around them is the emulator's one-pass stand-in, so the pass loop, the pieces of a large block and the device kernels are
left to tests/test_gpu_reads_index.py.  Every comparison is exact."""
import gzip
import os

import numpy as np
import pytest

from tests import reads_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FASTQ_PAIR = [os.path.join(GOLDEN, "data", "reads_r1.fastq"), os.path.join(GOLDEN, "data", "reads_r2.fastq")]
CONTIG_READS = [os.path.join(GOLDEN, "data", "contig-reads.fasta.gz")]
MASTER = [os.path.join(GOLDEN, "micro", "master.fasta")]


@pytest.fixture(scope="module")
def mtg():
    from tests import emu_lib
    return emu_lib.product_on_emulator()


def _same(counts, pair):
    km, ct = rc.as_arrays(counts)
    return len(km) == len(pair[0]) and (km == pair[0]).all() and (ct == pair[1]).all()


@pytest.mark.parametrize("files,cutoff,solid,branching", [(FASTQ_PAIR, 7, 7419, 36), (CONTIG_READS, 3, 10194, 46)])
def test_plain_count_gives_the_reference_projects_numbers(files, cutoff, solid, branching):
    """the reference before it judges anything: the golden runs of the reference project report these numbers of solid and branching
    nodes (test/full_test/gold_fill.output; the contig test's) -- with the per-window loop, and the numpy variant equal to it"""
    counts = rc.plain_count(files, 31)
    g = rc.expected_graph(counts, 31, cutoff, 0)
    assert len(g.solid) == solid
    assert g.nb_branching() == branching
    assert _same(counts, rc.plain_count_np(files, 31))


def _small_cases(tmp_path):
    """(name, paths, k) of groups A, B and C"""
    out = []
    for k in (31, 21):
        for group in rc.FORMAT_GROUPS:
            d = tmp_path / ("%s_%d" % (group, k))
            d.mkdir()
            out += [("%s/%s/k%d" % (group, name, k), paths, k) for name, paths in rc.format_cases(d, k, group)]
    kp = rc.k_case(tmp_path)
    out += [("k/%d" % k, kp, k) for k in rc.K_VALUES]
    for k in (31, 21):
        d = tmp_path / ("window_%d" % k)
        d.mkdir()
        out.append(("window/k%d" % k, rc.window_case(d, k)[0], k))
    return out


def test_loop_and_numpy_variants_agree_and_oracle_agrees_with_them(tmp_path):
    """groups A, B, C: plain_count's loop == its numpy variant, and the oracle's -in (mtgo_index_from_files, which the rest of the suite
    trusts) exports exactly the k-mers and counts of the plain count at abundance_min 1 and at 2"""
    from tests import oracle_lib
    for name, paths, k in _small_cases(tmp_path):
        counts = rc.plain_count(paths, k)
        assert counts, name
        assert _same(counts, rc.plain_count_np(paths, k)), name
        for lo in (1, 2):
            g = rc.expected_graph(counts, k, lo, 0)
            o = oracle_lib.Index.from_files(paths, k, lo)
            km, ct = o.export()
            o.close()
            assert len(km) == len(g.solid) and (km == g.solid).all(), (name, lo, len(km), len(g.solid))
            assert (np.minimum(ct, 255) == g.abund).all(), (name, lo)


def test_generators_make_what_they_promise(tmp_path):
    """palindromes occur the known number of times (B); every k-mer of word i counts c_i (C); an N every k-th character leaves no window
    and every (k+1)-th exactly one per stretch (A)"""
    for k in rc.K_VALUES + (12, 30):
        x = np.random.default_rng(k).integers(0, 1 << (2 * k), 200, dtype=np.uint64)
        assert [int(v) for v in rc.revcomp_np(x, k)] == [rc.revcomp(int(v), k) for v in x]
        assert rc.encode(rc.rc_str(rc.decode(x[0], k))) == rc.revcomp(int(x[0]), k)
    paths = rc.k_case(tmp_path)
    for k, times in rc.PALINDROME_TIMES.items():
        p = rc.encode(rc.palindrome(k))
        assert rc.revcomp(p, k) == p
        assert rc.plain_count(paths, k)[p] == times
    for k in (31, 21):
        d = tmp_path / ("w%d" % k)
        d.mkdir()
        wp, by_count = rc.window_case(d, k)
        counts = rc.plain_count(wp, k)
        assert len(counts) == 6 * len(rc.WINDOW_COUNTS)
        for c, kms in by_count.items():
            assert [counts[x] for x in kms] == [c] * 6
        base_only = rc.plain_count(dict(rc.format_cases(d, k, "wrap"))["width0"], k)
        n = dict(rc.format_cases(d, k, "N"))
        assert rc.plain_count(n["every_kth"], k) == base_only
        extra = rc.plain_count(n["every_k_plus_1th"], k)
        assert sum(extra.values()) - sum(base_only.values()) == 2 * 3 * 6  # 3 reads twice, 6 stretches of k nucleotides each


@pytest.mark.parametrize("k", [31, 21])
@pytest.mark.parametrize("group", rc.FORMAT_GROUPS)
def test_emulator_file_formats(mtg, tmp_path, group, k):
    """group A on the emulator: FileReadStream::getl (CRLF, a last line without newline, lines longer than its buffer's reads),
    next_block's FASTA branch (joined lines, blank lines, a header without sequence), its FASTQ branch (four lines whatever they start with),
    the file list of index_from_reads, and kmer_from_ascii / ascii_invalid (lowercase, N and n, the '\\n' between records)"""
    for name, paths in rc.format_cases(tmp_path, k, group):
        counts = rc.plain_count(paths, k)
        idx = mtg.Index.from_reads(paths, k, 2)
        try:
            rc.check_index(idx, counts, k, 2, 0)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        finally:
            idx.close()


def test_emulator_same_file_twice_doubles_every_count(mtg, tmp_path):
    """index_from_reads sums solidity over the list: the same file named twice makes a k-mer seen once solid at abundance_min 2"""
    (name, paths), = [c for c in rc.format_cases(tmp_path, 31, "several_files") if c[0] == "same_file_twice"]
    once, twice = rc.plain_count(paths[:1], 31), rc.plain_count(paths, 31)
    assert twice == {x: 2 * c for x, c in once.items()}
    idx = mtg.Index.from_reads(paths, 31, 2)
    assert idx.info()["nb_solid_kmers"] == len(once)
    idx.close()


@pytest.mark.parametrize("k", rc.K_VALUES)
def test_emulator_k(mtg, tmp_path, k):
    """group B on the emulator: kmer_from_ascii's canonical form and the tables' key widths at every k, self-complementary k-mers at even k"""
    paths = rc.k_case(tmp_path)
    counts = rc.plain_count(paths, k)
    must = [rc.encode(rc.palindrome(k))] if k in rc.PALINDROME_TIMES else []
    for lo in (1, 2):
        idx = mtg.Index.from_reads(paths, k, lo)
        rc.check_index(idx, counts, k, lo, 0, must_check=must)
        if must:
            assert idx.abundance(must)[0] == rc.PALINDROME_TIMES[k]
        idx.close()


@pytest.mark.parametrize("k", [10, 32])
def test_emulator_k_out_of_range(mtg, tmp_path, k):
    """index_from_reads' argument check: 11 <= k <= 31"""
    paths = rc.k_case(tmp_path)
    with pytest.raises(mtg.lib.MtgError) as e:
        mtg.Index.from_reads(paths, k, 2)
    assert e.value.code == 2  # MTG_ERR_ARG


def _build_window(mtg, paths, k, lo, hi):
    """an index, or None where the window leaves nothing solid and the build says so (see test_emulator_nothing_to_index)"""
    return mtg.Index.from_reads(paths, k, lo, hi)


@pytest.mark.parametrize("k", [31, 21])
def test_emulator_solidity_window(mtg, tmp_path, k):
    """group C on the emulator: both ends of [abundance_min, abundance_max] (the stand-in's own comparison, index_from_reads' passing of
    the options), the 255 ceiling of the stored abundance and nb_saturated"""
    paths, by_count = rc.window_case(tmp_path, k)
    counts = rc.plain_count(paths, k)
    edges = [x for c in (1, 2, 3, 5, 6, 12, 254, 255, 256, 300, 1000) for x in by_count[c]]
    for lo in rc.WINDOW_MINS:
        for hi in rc.window_maxs(lo):
            idx = mtg.Index.from_reads(paths, k, lo, hi)
            try:
                g = rc.check_index(idx, counts, k, lo, hi, must_check=edges)
            except AssertionError as e:
                raise AssertionError("window [%d, %d]: %s" % (lo, hi, e))
            if hi == 0 or hi >= 256:
                want = 3 if hi == 0 else 1  # 256, 300, 1000 / 256 alone
                assert g.nb_saturated == 6 * want and (idx.abundance(by_count[256]) == 255).all()
            idx.close()


@pytest.mark.parametrize("files,lo,auto,solid,branching", [(FASTQ_PAIR, -1, 7, 7419, 36), (CONTIG_READS, 3, -1, 10194, 46), (MASTER, -1, 3, None, None)])
def test_emulator_automatic_cutoff(mtg, files, lo, auto, solid, branching):
    """group F on the emulator: auto_cutoff on the histogram of the count table, and the graph at that cut-off against the plain count
    and the oracle"""
    from tests import oracle_lib
    counts = rc.plain_count_np(files, 31)
    idx = mtg.Index.from_reads(files, 31, lo)
    o = oracle_lib.Index.from_files(files, 31, lo)
    info = idx.info()
    assert info["abundance_auto"] == auto
    assert info["abundance_min"] == (auto if lo < 0 else lo)
    rc.check_index(idx, counts, 31, info["abundance_min"], 0, oracle_index=o)
    if solid is not None:
        assert (info["nb_solid_kmers"], info["nb_branching"]) == (solid, branching)
    o.close()
    idx.close()


def test_emulator_count_table_retry_is_reported(mtg, tmp_path):
    """the observable the GPU test of the too-small count table relies on: the build profile's phase "count_attempts" has the number of
    count tables tried in `units` -- more than one for single-coverage input (size hint / 4 slots for about size hint distinct k-mers),
    one for the deep window case"""
    paths = [rc.write_fasta(str(tmp_path / "low.fa"), [rc.rand_seq(np.random.default_rng(1), 60000)])]
    idx = mtg.Index.from_reads(paths, 31, 1)
    attempts = [p["units"] for p in idx.build_profile()["phases"] if p["name"] == "count_attempts"]
    assert len(attempts) == 1 and attempts[0] >= 2, attempts
    rc.check_index(idx, rc.plain_count_np(paths, 31), 31, 1, 0)
    idx.close()
    paths, _ = rc.window_case(tmp_path, 31)
    idx = mtg.Index.from_reads(paths, 31, 1)
    assert [p["units"] for p in idx.build_profile()["phases"] if p["name"] == "count_attempts"] == [1]
    idx.close()


def test_emulator_unreadable_input(mtg, tmp_path):
    """group G: a missing file among good ones, and a .gz cut off in the middle, give MTG_ERR_IO and mtg_last_error names the path
    (FileReadStream::next_block's gzopen, getl's gzerror / gzeof test, index_from_reads' rs.failed())"""
    good = rc.k_case(tmp_path)
    missing = str(tmp_path / "not_there.fa")
    with pytest.raises(mtg.lib.MtgError) as e:
        mtg.Index.from_reads(good + [missing] + good, 31, 2)
    assert e.value.code == 3 and missing in str(e.value)
    whole = rc.write_fasta(str(tmp_path / "whole.fa.gz"), [rc.rand_seq(np.random.default_rng(2), 200000)], width=70)
    cut = str(tmp_path / "cut.fa.gz")
    data = open(whole, "rb").read()
    open(cut, "wb").write(data[:len(data) // 2])
    with pytest.raises(mtg.lib.MtgError) as e:
        mtg.Index.from_reads(good + [cut], 31, 2)
    assert e.value.code == 3 and cut in str(e.value)


@pytest.mark.parametrize("content", ["", ">a\n>b words\n", ">a\nACGTNNACGT\n>b\nacgt\n"])
@pytest.mark.parametrize("lo", [-1, 1, 3])
def test_emulator_nothing_to_index(mtg, tmp_path, content, lo):
    """group G: an empty file, headers only, reads shorter than k.  Observed, and the same for the oracle and the emulator: MTG_OK and an
    empty index that answers "absent" to everything; with the automatic cut-off, abundance_min = abundance_auto = 10001 (auto_cutoff
    runs to the end of an all-zero histogram)"""
    from tests import oracle_lib
    path = str(tmp_path / "nothing.fa")
    open(path, "w").write(content)
    assert rc.plain_count([path], 31) == {}
    idx = mtg.Index.from_reads([path], 31, lo)
    o = oracle_lib.Index.from_files([path], 31, lo)
    assert len(o) == 0
    rc.check_index(idx, {}, 31, lo, 0, oracle_index=o)
    assert idx.info()["abundance_min"] == (10001 if lo < 0 else lo)
    o.close()
    idx.close()


def test_emulator_block_seam(mtg, tmp_path):
    """group E(ii) on the emulator: FileReadStream::next_block ends a block at the first record end past 64 MB and starts the next one
    with the record that follows (about 20 s here: two readings of 80 MB, the second after the count table doubled); every count is 200
    times the chunk's"""
    paths, chunk = rc.block_seam_case(tmp_path)
    assert os.path.getsize(paths[0]) > (64 << 20) + (8 << 20)
    km, ct = rc.plain_count_np([chunk], 31)
    idx = mtg.Index.from_reads(paths, 31, 1, 0)
    rc.check_index(idx, (km, ct * rc.BLOCK_COPIES), 31, 1, 0)
    assert idx.info()["nb_solid_kmers"] == len(km)
    idx.close()
