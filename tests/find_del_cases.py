"""A plain model of `find` for homozygous deletions (include/mtg_fill.h: mtg_index_find_del_sequences), to judge the device's calls.

It is the reference's gap observer FindDeletion::update with its fuzzy_site (src/FindDeletion.hpp:58-188) written out as it stands, run
inside the loop of find_cases.Scan.run_sequence -- the scan of FindBreakpoints::notify, which asks its gap observers in the order they were
registered and leaves the gap at the first one that calls it (src/FindBreakpoints.hpp:582-590).  The order is that of src/Finder.cpp:549-582:
the deletion observer, the two observers of insertions of 1-2 nt, the two site observers; which of them run is the configuration's.  The
observer reads the two k-mers, the gap's length and the graph, nothing else, and changes nothing of the scan.

A call is the tuple (seq, pos, kind, repeat, left, right, ins) of mtg_find_call with kind 4: pos = 0-based position of the nucleotide before
the deleted text (position() - 2 - del_size, what the observer passes to writeVcfVariant), repeat = the final repeat_size, left / right =
positions of kmer_begin / kmer_end, ins = del_size."""
from tests import find_cases as fc
from tests import find_het_cases as fh

STAT_KEYS = ("n_gaps", "n_candidates", "n_del_clean", "n_del_fuzzy", "n_fallback", "n_calls")

# the observer lists of the reference's configurations (src/Finder.cpp:320-398, :549-582); the heterozygous k-mer observer is not in this loop
OBSERVERS = {
    "-deletion-only": ("deletion", "small_clean", "small_fuzzy"),
    "-homo-only -no-snp": ("deletion", "small_clean", "small_fuzzy", "clean", "fuzzy"),
    "-no-snp": ("deletion", "small_clean", "small_fuzzy", "clean", "fuzzy"),
    "deletion": ("deletion",),
    "insertions": ("small_clean", "small_fuzzy", "clean", "fuzzy"),
}


class DelScan(fc.Scan):
    def __init__(self, graph, max_repeat, observers):
        fc.Scan.__init__(self, graph, max_repeat)
        self.observer_names = observers
        self.del_candidates = 0
        self.dcounts = {"n_del_clean": 0, "n_del_fuzzy": 0, "n_fallback": 0}

    # ---- FindDeletion.hpp:179-188
    def fuzzy_site(self, begin, end):
        i = self.max_repeat
        while i != 0:
            j = 1
            while begin[len(begin) - i:len(begin) - i + j] == end[0:j]:
                if i == j:
                    return j
                j += 1
            i -= 1
        return 0

    def all_in_graph(self, seq):
        for j in range(len(seq) - self.k + 1):
            if not self.g.contains(seq[j:j + self.k]):
                return False
        return True

    # ---- FindDeletion.hpp:61-173
    def deletion(self):
        if self.kmer_begin is None or self.kmer_end is None:
            return False
        if self.gap_stretch < self.k - self.max_repeat:
            return False
        self.del_candidates += 1
        begin, end = self.kmer_str(self.kmer_begin), self.kmer_str(self.kmer_end)
        repeat_size = self.fuzzy_site(begin, end)
        if repeat_size > self.max_repeat:
            return False
        if repeat_size != 0:
            begin = begin[:len(begin) - repeat_size]
        del_size = self.gap_stretch - self.k + repeat_size + 1
        if not self.all_in_graph(begin + end):
            if repeat_size == 0:
                return False
            if not self.all_in_graph(self.kmer_str(self.kmer_begin) + end):
                return False
            del_size -= repeat_size
            repeat_size = 0
            self.dcounts["n_fallback"] += 1
        if del_size <= 0:
            return False
        del_start_pos = self.position - 2 - del_size
        self.calls.append((self.s, del_start_pos, 4, repeat_size, self.kmer_begin, self.kmer_end, del_size))
        self.dcounts["n_del_fuzzy" if repeat_size else "n_del_clean"] += 1
        return True

    # the four slots of the base class's observer tuple (find_cases.Scan.run_sequence): the deletion observer goes before the first, and an
    # observer that the configuration leaves out never calls
    def small_clean(self):
        if "deletion" in self.observer_names and self.deletion():
            return True
        return "small_clean" in self.observer_names and fc.Scan.small_clean(self)

    def small_fuzzy(self):
        return "small_fuzzy" in self.observer_names and fc.Scan.small_fuzzy(self)

    def clean(self):
        return "clean" in self.observer_names and fc.Scan.clean(self)

    def fuzzy(self):
        return "fuzzy" in self.observer_names and fc.Scan.fuzzy(self)


def scan(solid, k, seqs, max_repeat, observers):
    """the literal scan with a list of observers (a key of OBSERVERS or a tuple of names): the DelScan after all sequences"""
    if max_repeat > k - 2:
        max_repeat = k - 2   # the library's rule for larger values
    sc = DelScan(fc.Graph(solid, k), max_repeat, OBSERVERS.get(observers, observers))
    for s, seq in enumerate(seqs):
        sc.run_sequence(s, seq)
    return sc


def find_del(solid, k, seqs, max_repeat):
    """(calls as a list of tuples in detection order, statistics) of the deletion observer alone"""
    sc = scan(solid, k, seqs, max_repeat, "deletion")
    st = {"n_gaps": sc.gaps, "n_candidates": sc.del_candidates, "n_calls": len(sc.calls)}
    st.update(sc.dcounts)
    return sc.calls, st


def find_gap_family(solid, k, seqs, max_repeat, config):
    """the calls of all gap observers of a configuration in one literal scan, in detection order"""
    return scan(solid, k, seqs, max_repeat, config).calls


# ---------------------------------------------------------------------------------------------------------------- the tool's files
def detected_at(call):
    """where the scan stood when the call was made and the observer family: a deletion is made by the gap observers at right + 1"""
    s, pos, kind, repeat, left, right, ins = call
    return (s, right + 1, 1) if kind == 4 else fh.detected_at(call)


def merge(homo, dels, het=()):
    """what the tool does with the lists of its layers: every homozygous insertion call (kind 0 or 1) on a gap with a deletion call -- equal
    (seq, left) -- is dropped, the rest is put in detection order, a heterozygous call before a gap call at the same position"""
    taken = {(c[0], c[4]) for c in dels}
    kept = [c for c in homo if (c[0], c[4]) not in taken]
    return sorted(kept + list(dels) + list(het), key=detected_at)


def lines(calls, names, seqs, k):
    """(lines of prefix.breakpoints, record lines of prefix.othervariants.vcf) for calls of all five kinds in detection order; ids count from 1
    across both files.  A deletion is one VCF line (writeVcfVariant, src/FindBreakpoints.hpp:661-678): REF = the genome's text
    [pos, pos + del_size + 1) as it stands, ALT = its first character"""
    bk, vcf = [], []
    for n, c in enumerate(calls, 1):
        s, pos, kind, repeat, left, right, ins = c
        if kind != 4:
            b, v = fh.lines([c], names, seqs, k)
            bk += [x.replace(">bkpt1_", ">bkpt%d_" % n, 1) for x in b]
            vcf += [x.replace("\tbkpt1\t", "\tbkpt%d\t" % n, 1) for x in v]
            continue
        ref = seqs[s][pos:pos + ins + 1]
        vcf.append("%s\t%d\tbkpt%d\t%s\t%s\t.\tPASS\tTYPE=DEL;LEN=%d;FUZZY=%d\tGT\t1/1" % (names[s], pos + 1, n, ref, ref[0], ins, repeat))
    return bk, vcf


# ---------------------------------------------------------------------------------------------------------------- synthetic cases
def deleted(donor_side, a, n):
    """the text with the stretch [a, a + n) cut out: a donor that carries a deletion of n nt behind position a - 1 of the reference"""
    return donor_side[:a] + donor_side[a + n:]


def with_del_repeat(rng, ref, a, n, r):
    """the reference changed around the stretch [a, a + n) so that deleting it leaves a junction repeat of exactly r (fuzzy_site compares a suffix with
    a prefix and can see more where the texts agree by chance, e.g. in a homopolymer; the model says what the observer then does):
    the r characters behind the stretch equal its first r (wrapping when r > n), the next one differs, and the character before the stretch
    differs from the stretch's last.  find_cases.with_repeat states the same for insertions: a deletion in the donor is an insertion in the
    reference"""
    return fc.with_repeat(rng, ref, a, n, r)


def tandem_case(rng, d, copies, flank=80):
    """(reference, donor): a unit of d nt in `copies` copies in the reference, one copy fewer in the donor, between random flanks whose
    characters next to the repeat do not continue it"""
    u = fc.rand_seq(rng, d)
    while d > 1 and len(set(u)) == 1:
        u = fc.rand_seq(rng, d)
    other = lambda ch: "ACGT"[("ACGT".index(ch) + 1 + int(rng.integers(3))) % 4]  # noqa: E731
    left, right = fc.rand_seq(rng, flank), fc.rand_seq(rng, flank)
    if left[-1] == u[-1]:
        left = left[:-1] + other(u[-1])
    if right[0] == u[0]:
        right = other(u[0]) + right[1:]
    return left + u * copies + right, left + u * (copies - 1) + right
