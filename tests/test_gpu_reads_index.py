"""The index the device builds from read files (index_from_stream in csrc/mtg_gpu_build.hip: k_count, k_count_stats,
k_jt_insert_from_counts and the host logic around them) against a plain k-mer count (tests/reads_cases.py): which k-mers are solid, with
which abundance, which edges, and the statistics -- all compared exactly.  Every case builds with Index.from_reads and ends in check_index."""
import os

import numpy as np
import pytest

from tests import reads_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FASTQ_PAIR = [os.path.join(GOLDEN, "data", "reads_r1.fastq"), os.path.join(GOLDEN, "data", "reads_r2.fastq")]
CONTIG_READS = [os.path.join(GOLDEN, "data", "contig-reads.fasta.gz")]
MASTER = [os.path.join(GOLDEN, "micro", "master.fasta")]
PASSES = (None, 2, 3, 5, 8)


@pytest.fixture(scope="module")
def mtg():
    import torch
    torch.cuda.init()  # torch bundles its own HIP runtime: initialise it before libmtgfill.so touches the device
    import mindthegap_amd
    mindthegap_amd.load_library()
    assert mindthegap_amd.device_count() >= 1, "these tests need a HIP device"
    return mindthegap_amd


def _passes(monkeypatch, n):
    if n is None:
        monkeypatch.delenv("MTG_COUNT_PASSES", raising=False)
    else:
        monkeypatch.setenv("MTG_COUNT_PASSES", str(n))


def _attempts(idx):
    a = [p["units"] for p in idx.build_profile()["phases"] if p["name"] == "count_attempts"]
    assert len(a) == 1, a
    return a[0]


# ------------------------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("k", [31, 21])
@pytest.mark.parametrize("group", rc.FORMAT_GROUPS)
def test_file_formats(mtg, monkeypatch, tmp_path, group, k):
    """A. What files look like: the text FileReadStream::next_block hands to count_pass (joined FASTA lines, CRLF, blank lines, headers
    without sequence, a last line without newline, four-line FASTQ records whatever their lines start with, .gz, several files as one
    stream) and what k_count / kmer_from_ascii make of it (lowercase, N and n at every place, reads of 0 .. 2k-1 nucleotides, the '\\n'
    between records), at abundance_min 2 so that a window counted once too often or too seldom changes the solid set"""
    _passes(monkeypatch, None)
    for name, paths in rc.format_cases(tmp_path, k, group):
        counts = rc.plain_count(paths, k)
        idx = mtg.Index.from_reads(paths, k, 2)
        try:
            rc.check_index(idx, counts, k, 2, 0)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        finally:
            idx.close()


# ------------------------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("k", rc.K_VALUES)
def test_k(mtg, monkeypatch, tmp_path, k):
    """B. k: kmer_from_ascii's canonical form, the key widths of the junction table (2(k-1) bits) and of the abundance source (2k bits),
    k_count's window end `i + k <= n`; at even k a self-complementary k-mer with a known count.  One pass and three (AbFromCounts /
    AbFromTable)."""
    paths = rc.k_case(tmp_path)
    counts = rc.plain_count(paths, k)
    must = [rc.encode(rc.palindrome(k))] if k in rc.PALINDROME_TIMES else []
    for npass in (None, 3):
        _passes(monkeypatch, npass)
        for lo in (1, 2):
            idx = mtg.Index.from_reads(paths, k, lo)
            rc.check_index(idx, counts, k, lo, 0, must_check=must)
            if must:
                assert counts[must[0]] == rc.PALINDROME_TIMES[k] and idx.abundance(must)[0] == rc.PALINDROME_TIMES[k]
            idx.close()


@pytest.mark.parametrize("k", [10, 32])
def test_k_out_of_range(mtg, tmp_path, k):
    """B. the argument check of index_from_reads / index_from_stream: 11 <= k <= 31, anything else is MTG_ERR_ARG"""
    paths = rc.k_case(tmp_path)
    with pytest.raises(mtg.lib.MtgError) as e:
        mtg.Index.from_reads(paths, k, 2)
    assert e.value.code == 2


# ------------------------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("lo", rc.WINDOW_MINS)
def test_solidity_window_and_ceiling_under_every_pass_count(mtg, monkeypatch, tmp_path, lo):
    """C. The solidity window and the ceiling: `lo = max(abundance_min, 1)`, `hi`, the test `c < lo || c > hi` of k_jt_insert_from_counts,
    the stored abundance min(c, 255) and nb_saturated, which one pass counts in k_us_ab / k_jt_scan / k_jt_unstored (AbFromCounts) and
    several passes count in k_jt_insert_from_counts (AbFromTable, cnt[3]); k_count's `% npass` with npass no power of two.  The five
    builds of a window answer every query alike, have the same statistics, and equal the plain count.  A window that leaves nothing
    solid (abundance_max below abundance_min) is an empty index, as test_nothing_to_index."""
    k = 31
    paths, by_count = rc.window_case(tmp_path, k)
    counts = rc.plain_count(paths, k)
    edges = [x for c in (1, 2, 3, 5, 6, 12, 254, 255, 256, 300, 1000) for x in by_count[c]]
    km, _ = rc.as_arrays(counts)
    q = np.concatenate([km, rc.revcomp_np(km, k), rc.expected_graph(counts, k, 1, 0).neighbor_kmers(km)])
    for hi in rc.window_maxs(lo):
        first = None
        for npass in PASSES:
            _passes(monkeypatch, npass)
            idx = mtg.Index.from_reads(paths, k, lo, hi)
            try:
                g = rc.check_index(idx, counts, k, lo, hi, must_check=edges)
            except AssertionError as e:
                raise AssertionError("window [%d, %d], passes %s: %s" % (lo, hi, npass, e))
            info = idx.info()
            got = ({s: info[s] for s in rc.STATS}, rc.answers(idx, q))
            if first is None:
                first = got
            assert got[0] == first[0], ("window [%d, %d], passes %s" % (lo, hi, npass), got[0], first[0])
            assert got[1] == first[1], "window [%d, %d], passes %s: answers differ from the one-pass build's" % (lo, hi, npass)
            if hi == 0 or hi >= 256:
                assert info["nb_saturated"] == g.nb_saturated == (18 if hi == 0 else 6)  # 256, 300 and 1000 / 256 alone
                assert (idx.abundance(by_count[256]) == 255).all() and (idx.abundance(by_count[255]) == 255).all()
                assert (idx.abundance(by_count[254]) == 254).all()
            idx.close()


# ------------------------------------------------------------------------------------------------------------------------------ D
@pytest.fixture(scope="module")
def low_coverage(tmp_path_factory):
    d = tmp_path_factory.mktemp("lowcov")
    plain = rc.low_coverage_case(d)
    counts = rc.plain_count_np(plain, 31)
    return plain, rc.low_coverage_case(d, gz=True), counts


@pytest.mark.parametrize("variant", ["plain", "gz", "passes3"])
def test_count_table_too_small(mtg, monkeypatch, low_coverage, variant):
    """D. The count table that is too small: single-coverage input has about as many distinct k-mers as bytes, four times the
    `size_hint / 4` slots of the first attempt (for .gz the hint is four times the file, about the same text).  count_insert's probe
    limit sets flags[0], count_pass reports it, round 1 breaks out, `continue` doubles total_slots and the histogram starts again from
    zero (d_histo is cleared per attempt).  The retry is observed: the build profile's phase "count_attempts" counts the tables tried.
    With MTG_COUNT_PASSES=3 the overflow shows in a pass after histogram bins were already accumulated."""
    plain, gz, counts = low_coverage
    assert len(counts[0]) > 0.9 * os.path.getsize(plain[0])
    _passes(monkeypatch, 3 if variant == "passes3" else None)
    idx = mtg.Index.from_reads(gz if variant == "gz" else plain, 31, 1)
    attempts = _attempts(idx)
    print("count tables tried (%s): %d" % (variant, attempts))
    assert attempts >= 2, attempts
    rc.check_index(idx, counts, 31, 1, 0)
    idx.close()


def test_count_table_large_enough_is_one_attempt(mtg, monkeypatch, tmp_path):
    """D. the observable the other way round: deep input fits the first table"""
    _passes(monkeypatch, None)
    paths, _ = rc.window_case(tmp_path, 31)
    idx = mtg.Index.from_reads(paths, 31, 1)
    assert _attempts(idx) == 1
    idx.close()


# ------------------------------------------------------------------------------------------------------------------------------ E
@pytest.fixture(scope="module")
def piece_seam(tmp_path_factory):
    return rc.piece_seam_case(tmp_path_factory.mktemp("piece"), 31)


@pytest.mark.parametrize("npass", [None, 2])
def test_piece_seam(mtg, monkeypatch, piece_seam, npass):
    """E(i). Piece seam: one record of 100 000 300 nucleotides is one block of FileReadStream, larger than the 80 MB device buffer, so
    count_pass sends it in two pieces: `len = min(text_cap - 64, n - off)` and `off += len - (k - 1)`.  Every k-mer of the repeated unit
    counts 100 (99 for the k-1 that wrap); one lost or doubled at the seam reads 99 or 101 on an interior k-mer.  With [100, 100] as the
    window those would leave the solid set; the k-mers around the seam are checked by name."""
    paths, counts, must = piece_seam
    assert os.path.getsize(paths[0]) > rc.TEXT_CAP and len(must) == 2 * 31 + 1
    _passes(monkeypatch, npass)
    idx = mtg.Index.from_reads(paths, 31, 100, 100)
    g = rc.check_index(idx, counts, 31, 100, 100, must_check=must)
    assert len(g.solid) == rc.PIECE_UNIT - 30
    assert (idx.abundance(must) == 100).all()
    idx.close()
    idx = mtg.Index.from_reads(paths, 31, 99, 99)
    assert idx.info()["nb_solid_kmers"] == 30
    rc.check_index(idx, counts, 31, 99, 99, must_check=must)
    idx.close()


@pytest.fixture(scope="module")
def block_seam(tmp_path_factory):
    paths, chunk = rc.block_seam_case(tmp_path_factory.mktemp("blocks"))
    km, ct = rc.plain_count_np([chunk], 31)
    return paths, (km, ct * rc.BLOCK_COPIES)


@pytest.mark.parametrize("npass", [None, 2])
def test_block_seam(mtg, monkeypatch, block_seam, npass):
    """E(ii). Block seam: about 80 MB of wrapped records cross FileReadStream's 64 MB BLOCK: next_block ends the block after the record
    that passes the mark and the following call starts with the line read ahead (have_line); the device sees two blocks per pass.  Every
    count is 200 times the chunk's."""
    paths, counts = block_seam
    assert os.path.getsize(paths[0]) > (64 << 20) + (8 << 20)
    _passes(monkeypatch, npass)
    idx = mtg.Index.from_reads(paths, 31, 1)
    rc.check_index(idx, counts, 31, 1, 0)
    assert idx.info()["nb_solid_kmers"] == len(counts[0])
    idx.close()
    idx = mtg.Index.from_reads(paths, 31, rc.BLOCK_COPIES, rc.BLOCK_COPIES)
    rc.check_index(idx, counts, 31, rc.BLOCK_COPIES, rc.BLOCK_COPIES)
    idx.close()


# ------------------------------------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("npass", [None, 3])
@pytest.mark.parametrize("files,lo,auto,solid,branching", [(FASTQ_PAIR, -1, 7, 7419, 36), (CONTIG_READS, 3, -1, 10194, 46), (MASTER, -1, 3, None, None)])
def test_automatic_cutoff(mtg, monkeypatch, files, lo, auto, solid, branching, npass):
    """F. The automatic cut-off from the device's histogram: k_count_stats (the LDS bins below 256 and the global ones), accumulated over
    the passes, read back into `histo` and given to auto_cutoff; then the graph at that cut-off.  The numbers are the reference
    project's golden ones."""
    from tests import oracle_lib
    _passes(monkeypatch, npass)
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


# ------------------------------------------------------------------------------------------------------------------------------ G
def test_unreadable_input(mtg, monkeypatch, tmp_path):
    """G. Input that cannot be read: count_pass returns MTG_ERR_IO on rs.failed() (a missing file: next_block's gzopen; a .gz cut off in
    the middle: getl's gzerror / gzeof test) and index_from_reads names the path in mtg_last_error"""
    _passes(monkeypatch, None)
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


@pytest.mark.parametrize("npass", [None, 3])
@pytest.mark.parametrize("content", ["", ">a\n>b words\n"])
def test_nothing_to_index(mtg, monkeypatch, tmp_path, content, npass):
    """G. An empty file and a file of headers only.  Observed on the emulator build and the oracle, and required here: MTG_OK and an
    empty index that answers "absent" everywhere; under the automatic cut-off abundance_min = abundance_auto = 10001 (auto_cutoff runs
    to the end of an all-zero histogram).  On the device: n_solid = 0, alloc_slot_table's 64-bucket floor, a scan that finds no chain
    start, sparsify with no record and no left-over k-mer."""
    from tests import oracle_lib
    _passes(monkeypatch, npass)
    path = str(tmp_path / "nothing.fa")
    open(path, "w").write(content)
    for lo in (-1, 3):
        idx = mtg.Index.from_reads([path], 31, lo)
        o = oracle_lib.Index.from_files([path], 31, lo)
        rc.check_index(idx, {}, 31, lo, 0, oracle_index=o)
        assert idx.info()["abundance_min"] == (10001 if lo < 0 else lo)
        o.close()
        idx.close()
