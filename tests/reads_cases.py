"""Read files as users write them, and a plain k-mer count to judge the index built from them (`-in`, mtg_index_create_from_reads).

The reference here is independent of the product, the oracle, the emulator and synth.py: it parses FASTA / FASTQ (.gz) itself, slides a
window over every record and counts canonical k-mers in the ABI's encoding (2 bits per nucleotide, A=0 C=1 T=2 G=3, first nucleotide in the
most significant bits).  A window that holds any character other than ACGTacgt is skipped; the generators below emit only ACGTNacgtn and
line ends, so "other" is unambiguous.  Every comparison made with it is exact."""
import gzip
import os

import numpy as np

NT = "ACTG"  # code -> nucleotide
CODE = {"A": 0, "C": 1, "T": 2, "G": 3}
QUERY_LIMIT = 2_000_000  # counted k-mers queried in full; above, a fixed-seed sample of this size (plus the case's must_check)
U64 = np.uint64


# ---------------------------------------------------------------------------------------------------------------- k-mers as integers
def kmask(k):
    return (1 << (2 * k)) - 1


def encode(s):
    x = 0
    for ch in s.upper():
        x = (x << 2) | CODE[ch]
    return x


def decode(x, k):
    x = int(x)
    return "".join(NT[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


def revcomp(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | ((x & 3) ^ 2)  # A <-> T is 0 <-> 2, C <-> G is 1 <-> 3
        x >>= 2
    return r


def canon(x, k):
    return min(x, revcomp(x, k))


def rc_str(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def revcomp_np(x, k):
    """revcomp for an array: complement (xor 2 per nucleotide), then the 32 two-bit groups of the word reversed (pairs, nibbles, bytes)
    and shifted down to the low 2k bits"""
    x = (np.array(x, dtype=U64) & U64(kmask(k))) ^ U64(0xAAAAAAAAAAAAAAAA & kmask(k))
    x = ((x >> U64(2)) & U64(0x3333333333333333)) | ((x & U64(0x3333333333333333)) << U64(2))
    x = ((x >> U64(4)) & U64(0x0F0F0F0F0F0F0F0F)) | ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4))
    return x.byteswap() >> U64(64 - 2 * k)


def canon_np(x, k):
    x = np.asarray(x, dtype=U64)
    return np.minimum(x, revcomp_np(x, k))


# ---------------------------------------------------------------------------------------------------------------- the plain reference
def read_records(path):
    """the sequences of a FASTA / FASTQ (.gz) file as bytes, one per record: a FASTA record is every line up to the next '>' line, joined;
    a FASTQ record is four lines of which the second is the sequence; CRLF counts as a line end; the last line may lack its newline"""
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        data = f.read()
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    lines = [l[:-1] if l.endswith(b"\r") else l for l in lines]
    recs, i = [], 0
    while i < len(lines):
        if lines[i].startswith(b">"):
            i += 1
            parts = []
            while i < len(lines) and not lines[i].startswith(b">"):
                parts.append(lines[i])
                i += 1
            recs.append(b"".join(parts))
        elif lines[i].startswith(b"@"):
            if i + 1 < len(lines):
                recs.append(lines[i + 1])
            i += 4
        else:
            i += 1
    return recs


_DIGITS = {i: "x" for i in range(256)}
_DIGITS.update({ord(c): str(v) for c, v in CODE.items()})
_DIGITS.update({ord(c.lower()): str(v) for c, v in CODE.items()})
_COMP_DIGITS = str.maketrans("0123", "2301")


def plain_count(files, k):
    """{canonical k-mer: number of windows of the files' records that spell it or its reverse complement}; the simple per-window loop"""
    counts = {}
    for path in files:
        for rec in read_records(path):
            t = rec.decode("latin-1").translate(_DIGITS)  # base-4 digits, 'x' for everything that is not a nucleotide
            n = len(t)
            u = t[::-1].translate(_COMP_DIGITS)           # the reverse complement, digit by digit
            for i in range(n - k + 1):
                w = t[i:i + k]
                if "x" in w:
                    continue
                f, r = int(w, 4), int(u[n - i - k:n - i], 4)
                c = f if f < r else r
                counts[c] = counts.get(c, 0) + 1
    return counts


_LUT = np.full(256, 255, np.uint8)
for _c, _v in CODE.items():
    _LUT[ord(_c)] = _v
    _LUT[ord(_c.lower())] = _v


def count_text_np(text, k):
    """the same count over one text (uint8 array, records separated by any non-nucleotide): rolling 2-bit codes, then np.unique.
    Returns (sorted canonical k-mers, their counts)."""
    n = len(text) - k + 1
    if n <= 0:
        return np.zeros(0, U64), np.zeros(0, np.int64)
    codes = _LUT[text]
    cs = np.concatenate([[0], np.cumsum(codes == 255)])
    ok = (cs[k:] - cs[:-k]) == 0
    c64 = (codes & 3).astype(U64)
    f, r = np.zeros(n, U64), np.zeros(n, U64)
    for j in range(k):
        w = c64[j:j + n]
        f = (f << U64(2)) | w
        r |= (w ^ U64(2)) << U64(2 * j)
    km, ct = np.unique(np.minimum(f, r)[ok], return_counts=True)
    return km.astype(U64), ct.astype(np.int64)


def plain_count_np(files, k):
    """plain_count, vectorised, for the cases with millions of k-mers; returns (sorted canonical k-mers, counts)"""
    parts = []
    for path in files:
        for rec in read_records(path):
            parts.append(rec)
            parts.append(b"\n")
    return count_text_np(np.frombuffer(b"".join(parts), np.uint8), k)


def as_arrays(counts):
    """a dict of plain_count or a pair of plain_count_np as (sorted k-mers uint64, counts int64)"""
    if isinstance(counts, dict):
        km = np.array(sorted(counts), dtype=U64)
        ct = np.array([counts[int(x)] for x in km], dtype=np.int64)
        return km, ct
    km, ct = counts
    return np.asarray(km, dtype=U64), np.asarray(ct, dtype=np.int64)


class ExpectedGraph:
    """what Graph::create makes of a count: the solid set, the stored abundance, nb_saturated, and the neighbours of any k-mer"""

    def __init__(self, counts, k, lo, hi):
        self.k = k
        self.kmers, self.counts = as_arrays(counts)
        solid = self.counts >= max(lo, 1)
        if hi > 0:
            solid &= self.counts <= hi
        self.is_solid = solid
        self.solid = self.kmers[solid]
        self.solid_counts = self.counts[solid]
        self.abund = np.minimum(self.solid_counts, 255).astype(np.uint32)
        self.nb_saturated = int((self.solid_counts > 255).sum())

    def _find(self, q):
        c = canon_np(q, self.k)
        if len(self.solid) == 0:
            return np.zeros(len(c), bool), np.zeros(len(c), np.int64)
        i = np.minimum(np.searchsorted(self.solid, c), len(self.solid) - 1)
        return self.solid[i] == c, i

    def contains(self, q):
        return self._find(q)[0]

    def abundance(self, q):
        hit, i = self._find(q)
        if len(self.solid) == 0:
            return np.zeros(len(hit), np.uint32)
        return np.where(hit, self.abund[i], 0).astype(np.uint32)

    def neighbors(self, q):
        """(successor mask, predecessor mask) of the k-mers q as given (either orientation, solid or not), by eight set look-ups; bit nt
        in the order A, C, T, G"""
        q = np.asarray(q, dtype=U64) & U64(kmask(self.k))
        succ, pred = np.zeros(len(q), np.uint8), np.zeros(len(q), np.uint8)
        for nt in range(4):
            s = ((q << U64(2)) & U64(kmask(self.k))) | U64(nt)
            p = (q >> U64(2)) | U64(nt << (2 * (self.k - 1)))
            succ |= self.contains(s).astype(np.uint8) << nt
            pred |= self.contains(p).astype(np.uint8) << nt
        return succ, pred

    def neighbor_kmers(self, q):
        q = np.asarray(q, dtype=U64)
        out = []
        for nt in range(4):
            out.append(((q << U64(2)) & U64(kmask(self.k))) | U64(nt))
            out.append((q >> U64(2)) | U64(nt << (2 * (self.k - 1))))
        return np.concatenate(out) if out else np.zeros(0, U64)

    def nb_branching(self):
        """solid k-mers that do not have exactly one successor and one predecessor"""
        s, p = self.neighbors(self.solid)
        pc = np.array([bin(i).count("1") for i in range(16)])
        return int((~((pc[s] == 1) & (pc[p] == 1))).sum())


def expected_graph(counts, k, lo, hi):
    return ExpectedGraph(counts, k, lo, hi)


def _first_differences(name, q, got, want, k, n=5):
    bad = np.nonzero(got != want)[0]
    return "%s differs for %d of %d k-mers, e.g. %s" % (name, len(bad), len(q), ", ".join(
        "%s: got %d, expected %d" % (decode(q[i], k), int(got[i]), int(want[i])) for i in bad[:n]))


def check_index(idx, counts, k, lo, hi, oracle_index=None, must_check=()):
    """The one comparison every case goes through: idx (an mtg.Index) against the expected graph of `counts`, exactly.  Returns the
    ExpectedGraph."""
    g = expected_graph(counts, k, lo, hi)
    info = idx.info()
    assert info["k"] == k
    assert info["nb_solid_kmers"] == len(g.solid), ("nb_solid_kmers", info["nb_solid_kmers"], len(g.solid))
    assert info["nb_saturated"] == g.nb_saturated, ("nb_saturated", info["nb_saturated"], g.nb_saturated)
    rng = np.random.default_rng(20240611)
    km, sampled = g.kmers, False
    if len(km) > QUERY_LIMIT:
        km, sampled = km[np.sort(rng.choice(len(km), QUERY_LIMIT, replace=False))], True
    must = np.array([int(x) for x in must_check], dtype=U64)
    if len(must):
        km = np.union1d(km, canon_np(must, k))
    hit = g.contains(km)
    solid_q, other_q = km[hit], km[~hit]
    assert len(g.kmers) == 0 or len(solid_q) + len(other_q) > 0
    rnd = rng.integers(0, 1 << (2 * k), 10000, dtype=np.uint64)
    q = np.concatenate([solid_q, revcomp_np(solid_q, k), other_q, revcomp_np(other_q, k), g.neighbor_kmers(solid_q), rnd, must])
    step = 1 << 22
    for a in range(0, len(q), step):
        qq = q[a:a + step]
        want_c, want_a = g.contains(qq).astype(np.uint8), g.abundance(qq)
        got_c, got_a = idx.contains(qq), idx.abundance(qq)
        assert (got_c == want_c).all(), _first_differences("contains", qq, got_c, want_c, k)
        assert (got_a == want_a).all(), _first_differences("abundance", qq, got_a, want_a, k)
        want_s, want_p = g.neighbors(qq)
        got_s, got_p = idx.neighbors(qq)
        assert (got_s == want_s).all(), _first_differences("successors", qq, got_s, want_s, k)
        assert (got_p == want_p).all(), _first_differences("predecessors", qq, got_p, want_p, k)
    if not sampled:
        assert info["nb_branching"] == g.nb_branching(), ("nb_branching", info["nb_branching"], g.nb_branching())
    if oracle_index is not None:
        o_solid, o_branching = oracle_index.stats()
        assert (info["nb_solid_kmers"], info["nb_branching"]) == (o_solid, o_branching)
        assert info["abundance_min"] == oracle_index.lib.mtgo_index_abundance_min(oracle_index.h)
        assert info["abundance_auto"] == oracle_index.lib.mtgo_index_auto_cutoff(oracle_index.h)
    return g


STATS = ("nb_solid_kmers", "nb_branching", "nb_saturated", "nb_unitigs", "nb_kmers_outside_unitigs")


def answers(idx, q):
    """everything an index says about the k-mers q, for comparing two builds of the same reads"""
    s, p = idx.neighbors(q)
    return idx.contains(q).tobytes(), idx.abundance(q).tobytes(), s.tobytes(), p.tobytes()


# ---------------------------------------------------------------------------------------------------------------- writers
def _open_w(path):
    return gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")


def write_fasta(path, reads, width=0, eol="\n", final_newline=True, blank_every=0, blank_inside=False):
    """reads as FASTA records; width > 0 wraps the sequence lines; blank_every = n: an empty line after every n-th record;
    blank_inside: an empty line in the middle of every wrapped record"""
    out = []
    for i, r in enumerate(reads):
        out.append(">r%d some words" % i)
        lines = [r[j:j + width] for j in range(0, len(r), width)] if width > 0 else ([r] if r else [])
        if blank_inside and len(lines) > 1:
            lines.insert(len(lines) // 2, "")
        out.extend(lines)
        if blank_every and i % blank_every == blank_every - 1:
            out.append("")
    text = eol.join(out) + (eol if final_newline else "")
    with _open_w(path) as f:
        f.write(text.encode())
    return path


def write_fastq(path, reads, qual="I", eol="\n", final_newline=True):
    """reads as four-line FASTQ records; qual: "I" (a plain quality line), "@" / ">" (the quality line starts with that character),
    "ACGT" (the quality line is made of these letters only, a sequence of its own that must not be counted)"""
    out = []
    for i, r in enumerate(reads):
        if qual == "I":
            q = "I" * len(r)
        elif qual in ("@", ">"):
            q = (qual + "I" * len(r))[:len(r)]
        else:
            q = ("GATTACACCGT" * (len(r) // 11 + 1))[:len(r)]
        out += ["@r%d/1" % i, r, "+", q]
    text = eol.join(out) + (eol if final_newline else "")
    with _open_w(path) as f:
        f.write(text.encode())
    return path


# ---------------------------------------------------------------------------------------------------------------- generators
def rand_seq(rng, n):
    return "".join(NT[i] for i in rng.integers(0, 4, n))


def tiled_reads(rng, genome_len=1500, read_len=100, step=37):
    """reads tiled over a random genome, every third one as its reverse complement: k-mer counts run from 1 to 3"""
    g = rand_seq(rng, genome_len)
    reads = [g[i:i + read_len] for i in range(0, genome_len - read_len + 1, step)]
    return [rc_str(r) if i % 3 == 2 else r for i, r in enumerate(reads)]


def format_cases(tmp, k, group):
    """group A, "what files look like": [(name, [paths])] written under tmp.  Every case holds the tiled base reads, so no index is empty,
    and is meant to be built with abundance_min 2 so that the solidity window decides something."""
    rng = np.random.default_rng(1000 + k)
    base = tiled_reads(rng)
    p = lambda name: os.path.join(str(tmp), name)
    cases = []
    if group == "wrap":
        for w in (1, 7, k - 1, k, 60, 70, 0):
            cases.append(("width%d" % w, [write_fasta(p("w%d.fa" % w), base, width=w)]))
    elif group == "line_ends":
        cases.append(("crlf", [write_fasta(p("crlf.fa"), base, width=60, eol="\r\n")]))
        cases.append(("crlf_fastq", [write_fastq(p("crlf.fq"), base, eol="\r\n")]))
        cases.append(("blank_between", [write_fasta(p("bb.fa"), base, width=60, blank_every=2)]))
        cases.append(("blank_inside", [write_fasta(p("bi.fa"), base, width=k, blank_inside=True)]))
        cases.append(("header_only", [write_fasta(p("ho.fa"), base[:5] + [""] + base[5:] + [""], width=60)]))
        cases.append(("no_final_newline", [write_fasta(p("nn.fa"), base, width=60, final_newline=False)]))
        cases.append(("no_final_newline_fastq", [write_fastq(p("nn.fq"), base, final_newline=False)]))
        cases.append(("no_final_newline_crlf", [write_fasta(p("nnc.fa"), base, width=0, eol="\r\n", final_newline=False)]))
    elif group == "case":
        cases.append(("lower", [write_fasta(p("lo.fa"), [r.lower() for r in base], width=60)]))
        mixed = ["".join(c.lower() if (i * 7 + j) % 3 == 0 else c for j, c in enumerate(r)) for i, r in enumerate(base)]
        cases.append(("mixed", [write_fasta(p("mx.fa"), mixed, width=60)]))
        cases.append(("mixed_fastq", [write_fastq(p("mx.fq"), mixed)]))
    elif group == "N":
        def put(r, pos, ch="N"):
            r = list(r)
            for q in pos:
                r[q] = ch
            return "".join(r)
        L = len(base[0])
        cases.append(("alone", [write_fasta(p("n1.fa"), [put(r, [L // 2]) for r in base], width=60)]))
        cases.append(("alone_lower", [write_fasta(p("n1l.fa"), [put(r, [L // 2], "n") for r in base], width=60)]))
        cases.append(("run", [write_fasta(p("nr.fa"), [put(r, range(40, 40 + k + 3)) for r in base], width=60)]))
        cases.append(("first_last", [write_fasta(p("nfl.fa"), [put(r, [0, L - 1]) for r in base]),
                                     write_fastq(p("nfl.fq"), [put(r, [0]) for r in base[:4]] + [put(r, [L - 1], "n") for r in base[4:8]])]))
        long_reads = [rand_seq(rng, 6 * (k + 1)) for _ in range(3)] * 2
        cases.append(("every_kth", [write_fasta(p("nk.fa"), base + [put(r, range(k - 1, len(r), k)) for r in long_reads], width=70)]))
        cases.append(("every_k_plus_1th", [write_fasta(p("nk1.fa"), base + [put(r, range(k, len(r), k + 1)) for r in long_reads], width=70)]))
        cases.append(("every_k_plus_1th_lower", [write_fastq(p("nk1.fq"), base + [put(r.lower(), range(k, len(r), k + 1), "n") for r in long_reads])]))
    elif group == "lengths":
        short = []
        for n in (0, 1, k - 1, k, k + 1, 2 * k - 1):
            s = rand_seq(rng, n)
            short += [s, s, rc_str(s)]  # three times: solid at abundance_min 2 when it holds a k-mer at all
        cases.append(("fasta", [write_fasta(p("len.fa"), short + base)]))
        cases.append(("fasta_short_last", [write_fasta(p("len2.fa"), base + short[::-1], final_newline=False)]))
        cases.append(("fastq", [write_fastq(p("len.fq"), short + base)]))
        cases.append(("fasta_wrapped", [write_fasta(p("len3.fa"), short + base, width=k - 1)]))
    elif group == "fastq":
        for name, qual in (("at", "@"), ("gt", ">"), ("acgt", "ACGT"), ("plain", "I")):
            cases.append(("qual_" + name, [write_fastq(p("q_%s.fq" % name), base, qual=qual)]))
    elif group == "gz":
        cases.append(("fasta_gz", [write_fasta(p("z.fa.gz"), base, width=60)]))
        cases.append(("fastq_gz", [write_fastq(p("z.fq.gz"), base, qual="@")]))
        cases.append(("crlf_no_newline_gz", [write_fasta(p("z2.fa.gz"), base, width=7, eol="\r\n", final_newline=False)]))
    elif group == "several_files":
        a, b, c = base[0::3], base[1::3], base[2::3]
        cases.append(("two", [write_fasta(p("a.fa"), a, width=60), write_fasta(p("b.fa"), b + c)]))
        cases.append(("three_mixed", [write_fasta(p("a3.fa"), a, final_newline=False), write_fastq(p("b3.fq"), b, qual="@"), write_fasta(p("c3.fa.gz"), c, width=k)]))
        one = write_fasta(p("twice.fa"), base, width=70)
        cases.append(("same_file_twice", [one, one]))
        cases.append(("fastq_then_fasta", [write_fastq(p("m.fq"), a + b, final_newline=False), write_fasta(p("m.fa"), c + a)]))
    else:
        raise ValueError(group)
    return cases


FORMAT_GROUPS = ("wrap", "line_ends", "case", "N", "lengths", "fastq", "gz", "several_files")

K_VALUES = (11, 16, 21, 22, 31)
PALINDROME_TIMES = {16: 3, 22: 5}


def palindrome(k):
    """a self-complementary k-mer (even k): a fixed half followed by its reverse complement"""
    h = rand_seq(np.random.default_rng(500 + k), k // 2)
    return h + rc_str(h)


def k_case(tmp):
    """group B: one read set for every k; the self-complementary 16-mer occurs 3 times and the 22-mer 5 times, each between random flanks
    (a window on a palindrome counts once: the k-mer is its own reverse complement)"""
    rng = np.random.default_rng(77)
    reads = tiled_reads(rng, genome_len=2500)
    for k, times in PALINDROME_TIMES.items():
        for _ in range(times):
            reads.append(rand_seq(rng, 40) + palindrome(k) + rand_seq(rng, 40))
    return [write_fasta(os.path.join(str(tmp), "k.fa"), reads, width=60)]


WINDOW_COUNTS = tuple(range(1, 13)) + (254, 255, 256, 300, 1000)
WINDOW_MINS = (0, 1, 2, 3, 12)


def window_maxs(lo):
    return (0, 1, 5, 255, 256, lo)


def window_case(tmp, k):
    """group C: distinct random words of k + 5 nucleotides, word i written c_i times as separate reads (every other copy as its reverse
    complement), so that each of its six k-mers counts c_i exactly.  Returns (paths, {count: [canonical k-mers]})."""
    for seed in range(100):
        rng = np.random.default_rng(9000 + seed)
        words = [rand_seq(rng, k + 5) for _ in WINDOW_COUNTS]
        kms = [[canon(encode(w[i:i + k]), k) for i in range(6)] for w in words]
        flat = [x for l in kms for x in l]
        if len(set(flat)) == len(flat):
            break
    else:
        raise RuntimeError("no word set without a shared k-mer")
    reads = []
    for w, c in zip(words, WINDOW_COUNTS):
        reads += [w if j % 2 == 0 else rc_str(w) for j in range(c)]
    order = np.random.default_rng(5).permutation(len(reads))
    reads = [reads[i] for i in order]
    return [write_fasta(os.path.join(str(tmp), "window.fa"), reads)], dict(zip(WINDOW_COUNTS, kms))


def low_coverage_case(tmp, gz=False, mbp=6):
    """group D: single-coverage random FASTA in long records: about as many distinct k-mers as the file has bytes, four times the slots of
    the first count table (size hint / 4)"""
    rng = np.random.default_rng(4242)
    path = os.path.join(str(tmp), "lowcov.fa" + (".gz" if gz else ""))
    lut = np.frombuffer(NT.encode(), np.uint8)
    with (gzip.open(path, "wb", compresslevel=1) if gz else open(path, "wb")) as f:
        for i in range(mbp * 4):
            f.write(b">long%d\n" % i)
            f.write(lut[rng.integers(0, 4, 250_000)].tobytes())
            f.write(b"\n")
    return [path]


PIECE_UNIT = 1_000_003
PIECE_COPIES = 100
TEXT_CAP = 80 << 20  # the device text buffer of index_from_stream


def piece_seam_case(tmp, k):
    """group E(i): ONE record of a random unit U (1 000 003 nt, its circular canonical k-mers all distinct) written 100 times back to
    back: longer than the device buffer, so it is counted in pieces.  Returns (paths, (kmers, counts), must_check): the circular k-mers
    starting at 0 .. L-k count 100, the k-1 that wrap count 99."""
    L = PIECE_UNIT
    for seed in range(20):
        rng = np.random.default_rng(31337 + seed)
        codes = rng.integers(0, 4, L).astype(np.uint8)
        u = np.frombuffer(NT.encode(), np.uint8)[codes]
        circ = np.concatenate([u, u[:k - 1]])
        km, ct = count_text_np(circ, k)
        if len(km) == L and (ct == 1).all():
            break
    else:
        raise RuntimeError("no unit with distinct circular k-mers")
    # per circular start offset: the canonical k-mer (count_text_np sorted them; redo the rolling code in text order for the offsets)
    first, _ = count_text_np(circ[:L], k)           # the L-k+1 k-mers that do not wrap
    counts = np.where(np.isin(km, first), PIECE_COPIES, PIECE_COPIES - 1).astype(np.int64)
    path = os.path.join(str(tmp), "piece.fa")
    with open(path, "wb") as f:
        f.write(b">one\n")
        for _ in range(PIECE_COPIES):
            f.write(u.tobytes())
        f.write(b"\n")
    # the k-mers around the first seam: a piece holds TEXT_CAP - 64 characters and the next one starts k-1 before its end
    must = []
    for seam in (TEXT_CAP - 64 - (k - 1), 2 * (TEXT_CAP - 64 - (k - 1))):
        if seam + 2 * k >= L * PIECE_COPIES:
            continue
        for off in range(seam - k, seam + k + 1):
            o = off % L
            must.append(canon(encode(circ[o:o + k].tobytes().decode()), k) if o + k <= len(circ) else 0)
    return [path], (km, counts), must


BLOCK_COPIES = 200


def block_seam_case(tmp, copies=BLOCK_COPIES):
    """group E(ii): a wrapped multi-record FASTA of about 80 MB, 200 copies of one chunk of records of about 400 kb: it crosses
    FileReadStream's 64 MB block end at a record boundary.  Returns (paths, chunk path): every count is `copies` times the chunk's."""
    rng = np.random.default_rng(6464)
    reads = [rand_seq(rng, int(n)) for n in rng.integers(150, 2500, 300)]
    chunk = write_fasta(os.path.join(str(tmp), "chunk.fa"), reads, width=70)
    body = open(chunk, "rb").read()
    path = os.path.join(str(tmp), "blocks.fa")
    with open(path, "wb") as f:
        for _ in range(copies):
            f.write(body)
    return [path], chunk
