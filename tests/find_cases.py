"""A plain model of `find` for homozygous insertions (include/mtg_fill.h: mtg_index_find_homo_sequences), to judge the device's calls.

It is the reference's scan written out as it stands: the sequential loop of FindBreakpoints::notify with its four members (solid stretch, gap
stretch, kmer_begin, kmer_end; src/FindBreakpoints.hpp:390-455,560-622) and the four gap observers in the order the reference registers them
(src/Finder.cpp:562-571): FindSmallCleanInsertion, FindSmallFuzzyInsertion (src/FindSmallInsertion.hpp), FindCleanInsertion,
FindFuzzyInsertion (src/FindInsertion.hpp), statement by statement.  It knows nothing of the product: the graph is a Python dict of solid
canonical k-mers (tests/reads_cases.plain_count), a k-mer is looked up by its string.  Strings hold ACGTNacgtn only (N / n is the invalid
character, lower case counts as upper case).

A call is the tuple (seq, pos, kind, repeat, left, right, ins) of mtg_find_call: pos 0-based as the observers pass it to writeBreakpoint /
writeIndel, kind 0 = insertion site, 1 = insertion of 1-2 nt, left / right = sequence positions of the two k-mers as written, ins = index of
the inserted string in INSERTIONS (0 for sites)."""
import numpy as np

from tests.reads_cases import plain_count

CALL_DTYPE = np.dtype([("seq", np.uint32), ("pos", np.uint32), ("kind", np.uint32), ("repeat", np.uint32), ("left", np.uint32), ("right", np.uint32), ("ins", np.uint32)])
INSERTIONS = ["A", "C", "G", "T", "AA", "AC", "AG", "AT", "CA", "CC", "CG", "CT", "GA", "GC", "GG", "GT", "TA", "TC", "TG", "TT"]  # char nucleo[20][6]


_DIGITS = str.maketrans("ACTG", "0123")       # the ABI's codes as base-4 digits
_COMP_DIGITS = str.maketrans("ACTG", "2301")  # those of the complement


def canon_of(w):
    """the canonical k-mer of a string over ACGT as an integer (first nucleotide most significant): the smaller of it and its reverse complement"""
    return min(int(w.translate(_DIGITS), 4), int(w[::-1].translate(_COMP_DIGITS), 4))


def solid_of_files(files, k, lo):
    """the set of canonical k-mers seen at least lo times in the files"""
    return {c for c, n in plain_count(files, k).items() if n >= lo}


class Graph:
    def __init__(self, solid, k):
        self.solid, self.k = solid, k

    def contains(self, s):
        """IFindObserver::contains: the canonical form of the k-mer is a node"""
        return canon_of(s) in self.solid

    def outdegree(self, s):
        return sum(self.contains(s[1:] + nt) for nt in "ACGT")

    def indegree(self, s):
        return sum(self.contains(nt + s[:-1]) for nt in "ACGT")


def is_valid(w):
    return len(w) > 0 and w.strip("ACGT") == ""  # (nothing is left once the nucleotides are stripped from both ends: there is no other character)


class Scan:
    """the members of FindBreakpoints that the gap observers in scope read, and the observers themselves"""

    def __init__(self, graph, max_repeat):
        self.g, self.k, self.max_repeat = graph, graph.k, max_repeat
        self.calls = []
        self.gaps = 0        # times the gap observers were called
        self.candidates = 0  # of those, with both k-mers valid and the gap's length in range
        self.counts = {"homo_clean": 0, "homo_fuzzy": 0, "small_clean": 0, "small_fuzzy": 0}

    # ---- FindSmallInsertion.hpp:57-125 / 147-212: the loop over the 20 strings, shared by the two observers
    def micro_assembly(self, kmer_begin_str, kmer_end_str):
        k = self.k
        for i, ins in enumerate(INSERTIONS):
            seq = kmer_begin_str + ins + kmer_end_str
            sum_valid, found = 0, False
            for j in range(len(seq) - k + 1):
                if self.g.contains(seq[j:j + k]):
                    sum_valid += 1
                else:
                    break
                if sum_valid == k:
                    found = True      # the windows behind the k-th are still looked at, but nothing depends on them any more
            if found:
                return i
        return None

    def small_clean(self):
        if self.kmer_begin is None or self.kmer_end is None:
            return False
        if self.gap_stretch == self.k - 1:
            b, e = self.kmer_str(self.kmer_begin), self.kmer_str(self.kmer_end)
            i = self.micro_assembly(b, e)    # no degree test in this observer
            if i is None:
                return False
            self.calls.append((self.s, self.position - 2, 1, 0, self.kmer_begin, self.kmer_end, i))
            self.counts["small_clean"] += 1
            return True
        return False

    def fuzzy_right(self, repeat):
        """kmer_end_str of the fuzzy observers: k characters at position() - 1 + repeat_size, None when codeSeed finds them invalid"""
        a = self.position - 1 + repeat
        w = self.seq[a:a + self.k]
        return (a, w) if len(w) == self.k and is_valid(w) else (a, None)

    def small_fuzzy(self):
        if self.kmer_begin is None or self.kmer_end is None:
            return False
        k = self.k
        if self.gap_stretch < k - 1 and self.gap_stretch >= k - 1 - self.max_repeat:
            repeat = k - 1 - self.gap_stretch
            b = self.kmer_str(self.kmer_begin)
            a, w = self.fuzzy_right(repeat)
            if self.g.outdegree(b) == 0 or self.g.indegree(self.kmer_str(self.kmer_end)) == 0 or w is None:
                return False
            i = self.micro_assembly(b, w)
            if i is None:
                return False
            self.calls.append((self.s, self.position - 2, 1, repeat, self.kmer_begin, a, i))
            self.counts["small_fuzzy"] += 1
            return True
        return False

    def clean(self):
        if self.kmer_begin is None or self.kmer_end is None:
            return False
        if self.gap_stretch == self.k - 1:
            if self.g.outdegree(self.kmer_str(self.kmer_begin)) == 0 or self.g.indegree(self.kmer_str(self.kmer_end)) == 0:
                return False
            self.calls.append((self.s, self.position - 2, 0, 0, self.kmer_begin, self.kmer_end, 0))
            self.counts["homo_clean"] += 1
            return True
        return False

    def fuzzy(self):
        if self.kmer_begin is None or self.kmer_end is None:
            return False
        k = self.k
        if self.gap_stretch < k - 1 and self.gap_stretch >= k - 1 - self.max_repeat:
            repeat = k - 1 - self.gap_stretch
            a, w = self.fuzzy_right(repeat)
            if self.g.outdegree(self.kmer_str(self.kmer_begin)) == 0 or self.g.indegree(self.kmer_str(self.kmer_end)) == 0 or w is None:
                return False
            self.calls.append((self.s, self.position - 2 + repeat, 0, repeat, self.kmer_begin, a, 0))
            self.counts["homo_fuzzy"] += 1
            return True
        return False

    def kmer_str(self, p):
        return self.seq[p:p + self.k]

    # ---- FindBreakpoints::operator() and notify
    def run_sequence(self, s, seq):
        k = self.k
        self.s, self.seq = s, seq.upper()
        self.kmer_begin = self.kmer_end = None    # KmerCanonical(): not valid
        self.solid_stretch = self.gap_stretch = 0
        previous_kmer = None                      # m_previous_kmer is not reset per sequence; it is read only behind a solid stretch of this one
        self.position = 0
        observers = (self.small_clean, self.small_fuzzy, self.clean, self.fuzzy)
        while self.position + k <= len(self.seq):
            w = self.seq[self.position:self.position + k]
            if not is_valid(w):
                self.solid_stretch = self.gap_stretch = 0
                self.kmer_begin = self.kmer_end = None
            else:
                in_graph = self.g.contains(w)
                if in_graph:
                    self.solid_stretch += 1
                    if self.solid_stretch > 1 and self.gap_stretch > 0:
                        self.gaps += 1
                        if self.kmer_begin is not None and self.kmer_end is not None and k - 1 - self.max_repeat <= self.gap_stretch <= k - 1:
                            self.candidates += 1
                        for ob in observers:
                            if ob():
                                break
                        self.gap_stretch = 0
                    if self.solid_stretch == 1:
                        self.kmer_end = self.position
                else:
                    if self.solid_stretch == 1:
                        self.gap_stretch += self.solid_stretch
                    if self.solid_stretch > 1 and previous_kmer is not None:
                        self.kmer_begin = previous_kmer
                    self.gap_stretch += 1
                    self.solid_stretch = 0
                previous_kmer = self.position
            self.position += 1


def find_homo(solid, k, seqs, max_repeat):
    """(calls as a list of tuples in detection order, statistics) of the literal scan"""
    if max_repeat > k - 2:
        max_repeat = k - 2   # the library's rule for larger values (a gap has at least one position)
    sc = Scan(Graph(solid, k), max_repeat)
    for s, seq in enumerate(seqs):
        sc.run_sequence(s, seq)
    st = {"n_gaps": sc.gaps, "n_candidates": sc.candidates, "n_homo_clean": sc.counts["homo_clean"], "n_homo_fuzzy": sc.counts["homo_fuzzy"],
          "n_small_clean": sc.counts["small_clean"], "n_small_fuzzy": sc.counts["small_fuzzy"]}
    return sc.calls, st


def gaps_by_anchors(solid, k, seqs):
    """the data-parallel statement of the gap rule: [(seq, first position, length, fresh kmer_begin)] of the reported gaps.  A position is an
    anchor when it is present and its left or right neighbour is; a gap is a maximal stretch of valid positions that are no anchors; it is
    reported when the position behind it is an anchor, and its kmer_begin is valid when the position before it is one."""
    g = Graph(solid, k)
    out = []
    for s, seq in enumerate(seqs):
        up = seq.upper()
        n = max(len(up) - k + 1, 0)
        valid = [is_valid(up[p:p + k]) for p in range(n)]
        present = [valid[p] and g.contains(up[p:p + k]) for p in range(n)]
        anchor = [present[p] and ((p > 0 and present[p - 1]) or (p + 1 < n and present[p + 1])) for p in range(n)]
        p = 0
        while p < n:
            if not valid[p] or anchor[p]:
                p += 1
                continue
            e = p
            while e < n and valid[e] and not anchor[e]:
                e += 1
            if e < n and anchor[e]:
                out.append((s, p, e - p, p > 0 and anchor[p - 1]))
            p = e
    return out


def literal_gaps(solid, k, seqs):
    """the same from the literal loop: one entry per call of the gap observers"""
    out = []

    class Rec(Scan):
        pass
    sc = Rec(Graph(solid, k), 0)
    probe = lambda: out.append((sc.s, sc.position - 1 - sc.gap_stretch, sc.gap_stretch, sc.kmer_begin is not None)) or True  # noqa: E731
    sc.small_clean = probe
    for s, seq in enumerate(seqs):
        sc.run_sequence(s, seq)
    return out


# ---------------------------------------------------------------------------------------------------------------- the tool's files
def breakpoint_lines(calls, names, seqs, k):
    """the lines of prefix.breakpoints (writeBreakpoint) and the record lines of prefix.othervariants.vcf (writeIndel) for calls in detection
    order; ids are numbered from 1 across both files; the REPEATED field is empty"""
    bk, vcf = [], []
    for n, (s, pos, kind, repeat, left, right, ins) in enumerate(calls, 1):
        up = seqs[s].upper()
        lk = up[left:left + k]                                           # model().toString: upper case
        rk = seqs[s][right:right + k] if repeat else up[right:right + k]   # the fuzzy right k-mer is the genome's text as it stands
        if kind == 0:
            head = ">bkpt%d_%s_pos_%d_fuzzy_%d_HOM" % (n, names[s], pos + 1, repeat)
            bk += [head + "  left_kmer", lk, head + "  right_kmer", rk]
        else:
            ref = lk[k - 1 - repeat]
            vcf.append("%s\t%d\tbkpt%d\t%s\t%s\t.\tPASS\tTYPE=INS;LEN=%d;FUZZY=%d\tGT\t1/1" % (names[s], pos + 1, n, ref, ref + INSERTIONS[ins], len(INSERTIONS[ins]), repeat))
    return bk, vcf


def parse_breakpoints(text):
    """[(name, 1-based pos, fuzzy, type, left k-mer, right k-mer)] of a .breakpoints file"""
    lines = text.splitlines()
    out = []
    for i in range(0, len(lines) - 3, 4):
        f = lines[i][1:].split()[0].split("_")
        assert lines[i].split()[-1] == "left_kmer" and lines[i + 2].split()[-1] == "right_kmer" and lines[i].split()[0] == lines[i + 2].split()[0]
        out.append(("_".join(f[1:-5]), int(f[-4]), int(f[-2]), f[-1], lines[i + 1], lines[i + 3]))
    return out


def parse_vcf(text):
    """[(name, POS, REF, ALT, TYPE, LEN, FUZZY, GT)] of the record lines of a VCF"""
    out = []
    for l in text.splitlines():
        if not l or l.startswith("#"):
            continue
        f = l.split("\t")
        info = dict(x.split("=") for x in f[7].split(";"))
        out.append((f[0], int(f[1]), f[3], f[4], info["TYPE"], int(info["LEN"]), int(info["FUZZY"]), f[9]))
    return out


# ---------------------------------------------------------------------------------------------------------------- synthetic cases
def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def solid_of_strings(strings, k):
    """every k-mer of the strings, canonical"""
    out = set()
    for s in strings:
        for p in range(len(s) - k + 1):
            out.add(canon_of(s[p:p + k]))
    return out


def planted(rng, donor, k, sites):
    """the donor with the stretches [a, a + n) cut out: what a reference looks like when the donor carries insertions of n nt behind position
    a - 1.  sites = [(a, n)] ascending and apart; a junction repeat arises where the donor's text makes one"""
    out, at = [], 0
    for a, n in sites:
        out.append(donor[at:a])
        at = a + n
    out.append(donor[at:])
    return "".join(out)


def with_repeat(rng, donor, a, n, r):
    """the donor changed around the stretch [a, a + n) so that cutting it out leaves a junction repeat of exactly r: the r characters behind
    the stretch equal its first r characters (wrapping around when r > n), the next one differs, and the character before the stretch
    differs from its last one (no repeat towards the left).  Returns the new donor."""
    d = list(donor)
    other = lambda ch: "ACGT"[("ACGT".index(ch) + 1 + int(rng.integers(3))) % 4]  # noqa: E731
    for i in range(r):
        d[a + n + i] = d[a + i]
    if d[a + n + r] == d[a + r]:
        d[a + n + r] = other(d[a + r])
    if d[a - 1] == d[a + n - 1]:
        d[a - 1] = other(d[a + n - 1])
    return "".join(d)
