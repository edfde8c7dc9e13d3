"""A plain model of `find` for close homozygous SNPs (include/mtg_fill.h: mtg_index_find_msnp_sequences), to judge the device's calls.

THE LITERAL MODEL (RingScan) is the reference's gap observer FindMultiSNP::update (src/FindSNP.hpp:459-545) with FindSNP::snp_at_end
(:139-208), mutate_kmer (:88-96) and correct_history (:548-564) written out as they stand, on a real ring: m_het_kmer_history is a list of
256 k-mers, every index is taken & 255 (the reference's unsigned char), the ring is filled with the all-A k-mer per sequence (memset 0,
src/FindBreakpoints.hpp:403), written at end_index for every valid position (store_kmer_info, :1037) and both indices advance at every
position (:423).  Stale slots stay where they are.  It runs in the loop of find_cases.Scan.run_sequence, copied here because the ring has to
be written at every position; the solo observer of find_snp_cases, which the reference registers first (src/Finder.cpp:551-553), reads the
same ring.  A gap taken in part changes gap_stretch, solid_stretch and kmer_begin as the reference does (:531-538).

THE CLOSED FORM (closed_form) is the rule as include/mtg_fill.h states it, a pure function of one gap on a private copy of the text, with
switches that make the wrong models of the mutation checks.

THE DEVIATION: the product does not judge gaps of 255 positions and more.  RingScan.judge_long = True is the reference as it stands (its
ring wraps); False is what the product is held to: such a gap is a candidate, counted in n_long, consumed 0, no call.

A call is the tuple (seq, pos, kind, repeat, left, right, ins) of mtg_find_call with kind 6: pos = 0-based position of the SNP (begin_pos,
what the observer passes to writeVcfVariant), repeat = 0, left / right = positions of kmer_begin / kmer_end as they were when the observer
was asked, ins = ord(ALT) | ord(REF) << 8.  A gap record is (seq, start, length, consumed, n_snps)."""
import numpy as np

from tests import find_cases as fc
from tests import find_snp_cases as fs

MAX_GAP = 254
STAT_KEYS = ("n_gaps", "n_candidates", "n_calls", "n_full", "n_partial", "n_long")

OBSERVERS = {"-multi-snps": ("multi",), "-solo-snps -multi-snps": ("solo", "multi"), "multi": ("multi",), "solo": ("solo",)}


class RingScan(fs.SnpScan):
    judge_long = False

    def __init__(self, graph, max_repeat, observers, snp_min_val):
        fs.SnpScan.__init__(self, graph, max_repeat, observers)
        self.snp_min_val = snp_min_val
        self.gap_records = []
        self.n_long = 0
        # what the steps looked like, for the coverage conditions of the tests
        self.seen = {"steps": 0, "calls": 0, "tie_below_k": 0, "two_reach_k": 0, "beyond_stop": 0, "reads_substitution": 0, "gaps_with_several": 0}

    # ---- FindBreakpoints: the ring
    def het_kmer_begin_index(self):
        return self.begin_index & 255

    def het_kmer_history(self, index):
        return self.ring[index & 255]

    # ---- FindSNP.hpp:139-208 with nb_kmer_val; returns (found, beginpos, ret_nuc, ref_nuc, nb_kmer_val).  `counts` keeps what every
    # alternative had when it left the map, for the statistics only
    def snp_at_end_count(self, beginpos, limit):
        k = self.k
        nuc = {0: 0, 1: 0, 2: 0, 3: 0}
        beginpos_init = beginpos
        ref_nuc = self.CODES.index(self.het_kmer_history(beginpos)[-1])
        del nuc[ref_nuc]
        counts = {}
        end = False
        j = 0
        while not end and j != k:
            for n in sorted(nuc):
                correct_kmer = self.mutate_kmer(self.het_kmer_history(beginpos), n, k - j)
                if self.g.contains(correct_kmer):
                    nuc[n] += 1
                else:
                    if len(nuc) == 1:
                        end = True
                        beginpos = (beginpos - 1) & 255
                        break
                    counts[n] = nuc[n]
                    del nuc[n]
            beginpos = (beginpos + 1) & 255
            j += 1
        counts.update(nuc)
        self.last_counts = counts
        best = sorted(nuc)[0]
        for n in sorted(nuc):
            if nuc[n] > nuc[best]:
                best = n
        if nuc[best] >= limit:
            return True, beginpos, best, ref_nuc, nuc[best]
        return False, beginpos_init, None, ref_nuc, 0

    # ---- FindSNP.hpp:548-564 (the degrees and the repeat flag of the slot are not modelled: nothing in scope reads them)
    def correct_history(self, pos, nuc):
        for i in range(self.k):
            index = (i + pos) & 255
            self.ring[index] = self.mutate_kmer(self.ring[index], nuc, self.k - i)

    # ---- FindSNP.hpp:459-545
    def multi(self):
        if self.kmer_begin is None or self.kmer_end is None:
            return False
        k, m = self.k, self.snp_min_val
        if self.gap_stretch > k + m:
            length, start = self.gap_stretch, self.position - 1 - self.gap_stretch
            if length > MAX_GAP and not self.judge_long:
                self.n_long += 1
                self.gap_records.append((self.s, start, length, 0, 0))
                return False
            nb_snp = 0
            begin_pos = self.position - 1 - self.gap_stretch + k - 1
            begin_pos_init = begin_pos
            index_end = (self.het_kmer_begin_index() + k - 1) & 255
            index_pos = (index_end - self.gap_stretch) & 255
            left, right = self.kmer_begin, self.kmer_end
            prev_nb = None
            while index_pos != index_end:
                save_index = index_pos
                found, index_pos, nuc, ref_nuc, nb_kmer_val = self.snp_at_end_count(index_pos, m)
                self.seen["steps"] += 1
                f = sorted(self.last_counts.values())
                if found and f[-1] == f[-2] and m <= f[-1] < k:
                    self.seen["tie_below_k"] += 1
                if f[-2] == k:
                    self.seen["two_reach_k"] += 1
                if found:
                    if begin_pos + nb_kmer_val - begin_pos_init > self.gap_stretch:
                        self.seen["beyond_stop"] += begin_pos > begin_pos_init
                        break
                    if prev_nb is not None and prev_nb < k:
                        self.seen["reads_substitution"] += 1
                    prev_nb = nb_kmer_val
                    self.correct_history(save_index, nuc)
                    nb_snp += 1
                    ins = ord(self.CODES[nuc]) | (ord(self.CODES[ref_nuc]) << 8)
                    self.calls.append((self.s, begin_pos, 6, 0, left, right, ins))
                    self.seen["calls"] += 1
                    begin_pos += nb_kmer_val
                else:
                    break
            self.seen["gaps_with_several"] += nb_snp > 1
            nb_kmer_correct = begin_pos - begin_pos_init
            self.gap_records.append((self.s, start, length, nb_kmer_correct, nb_snp))
            if nb_kmer_correct == 0:
                return False
            if nb_kmer_correct != self.gap_stretch:
                self.gap_stretch -= nb_kmer_correct
                self.solid_stretch += nb_kmer_correct
                self.kmer_begin = ("corrected", self.het_kmer_history(index_pos - 1))   # a k-mer that is no position of the sequence any more
                return False
            return True
        return False

    # the first slot of the base class's observer tuple: solo, then multi (src/Finder.cpp:551-553); nothing else is in scope with multi
    def small_clean(self):
        if "solo" in self.observer_names and self.solo():
            return True
        if "multi" in self.observer_names and self.multi():
            return True
        return False

    def small_fuzzy(self):
        return False

    def clean(self):
        return False

    def fuzzy(self):
        return False

    # ---- FindBreakpoints::operator() and notify (find_cases.Scan.run_sequence) with the ring
    def run_sequence(self, s, seq):
        k = self.k
        self.s, self.seq = s, seq.upper()
        self.kmer_begin = self.kmer_end = None
        self.solid_stretch = self.gap_stretch = 0
        self.ring = ["A" * k] * 256
        self.end_index, self.begin_index = k + 1, 1
        previous_kmer = None
        self.position = 0
        while self.position + k <= len(self.seq):
            w = self.seq[self.position:self.position + k]
            if not fc.is_valid(w):
                self.solid_stretch = self.gap_stretch = 0
                self.kmer_begin = self.kmer_end = None
            else:
                in_graph = self.g.contains(w)
                self.ring[self.end_index & 255] = w     # store_kmer_info, ahead of the observers
                if in_graph:
                    self.solid_stretch += 1
                    if self.solid_stretch > 1 and self.gap_stretch > 0:
                        self.gaps += 1
                        for ob in (self.small_clean, self.small_fuzzy, self.clean, self.fuzzy):
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
            self.begin_index += 1
            self.end_index += 1


class LiteralRingScan(RingScan):
    """the reference as it stands, gaps of 255 and more included"""
    judge_long = True


def scan(solid, k, seqs, snp_min_val=5, max_repeat=5, observers="multi", cls=RingScan):
    if max_repeat > k - 2:
        max_repeat = k - 2
    sc = cls(fc.Graph(solid, k), max_repeat, OBSERVERS.get(observers, observers), snp_min_val)
    for s, seq in enumerate(seqs):
        sc.run_sequence(s, seq)
    return sc


def stats_of(sc):
    recs = sc.gap_records
    return {"n_gaps": sc.gaps, "n_candidates": len(recs), "n_calls": sum(1 for c in sc.calls if c[2] == 6),
            "n_full": sum(1 for r in recs if r[3] == r[2]), "n_partial": sum(1 for r in recs if 0 < r[3] < r[2]), "n_long": sc.n_long}


def find_msnp(solid, k, seqs, snp_min_val=5, max_repeat=5, cls=RingScan):
    """(calls in detection order, gap records in scan order, statistics) of the multi observer alone"""
    sc = scan(solid, k, seqs, snp_min_val, max_repeat, "multi", cls)
    return sc.calls, sc.gap_records, stats_of(sc)


# ---------------------------------------------------------------------------------------------------------------- the closed form
def closed_form(graph, seq, start, length, k, m, first_at_tie=False, no_beyond_stop=False, uncapped=False, no_correction=False, order="ACTG", reads=None):
    """(calls [(pos, REF, ALT)], consumed) of one gap by the rule of include/mtg_fill.h.  The switches are the wrong models: the first
    alternative in order also where the best count is below k; no stop where a call would go beyond the gap; windows not capped at
    L - c + 1 (the text behind start + L + k is read as it stands); the text not corrected between steps; the alternatives in A, C, G, T order.
    The uncapped model cannot differ in its outcome -- a count that reaches L - c + 1 ends the chain whatever lies behind -- but in what it
    reads: reads, a list, receives the last text position of every window looked at"""
    t = list(seq.upper())
    base = "".join(t)
    c, calls = 0, []
    while c != length:
        g = start + c + k - 1
        ref = t[g]
        cap = k if uncapped else min(k, length - c + 1)
        src = list(base) if no_correction else t
        f = {}
        for a in order:
            if a == ref:
                continue
            j = 0
            while j < cap:
                w = src[start + c + j:start + c + j + k]
                if reads is not None:
                    reads.append(start + c + j + k - 1)
                if len(w) < k:
                    break
                w[k - 1 - j] = a
                if not graph.contains("".join(w)):
                    break
                j += 1
            f[a] = j
        best = max(f.values())
        tied = [a for a in order if a != ref and f[a] == best]
        win = tied[0] if (best == k or first_at_tie) else tied[-1]
        if best < m:
            break
        if c + best > length:
            if not no_beyond_stop:
                break
        calls.append((g, ref, win))
        t[g] = win
        c += best
        if c > length:   # (only the model without the stop gets here: it has to end)
            break
    return calls, c


def candidates(solid, k, seqs, m):
    """[(seq, start, length)] of the gaps the observer looks at, from the literal gaps of find_cases"""
    return [(s, p, n) for s, p, n, fresh in fc.literal_gaps(solid, k, seqs) if fresh and n > k + m]


def find_by_closed_form(solid, k, seqs, m, **wrong):
    """(calls, gap records) as find_msnp gives them, every candidate judged by the closed form; gaps of 255 and more are not judged"""
    graph = fc.Graph(solid, k)
    calls, recs = [], []
    for s, p, n in candidates(solid, k, seqs, m):
        if n > MAX_GAP:
            recs.append((s, p, n, 0, 0))
            continue
        got, consumed = closed_form(graph, seqs[s], p, n, k, m, **wrong)
        recs.append((s, p, n, consumed, len(got)))
        calls += [(s, g, 6, 0, p - 1, p + n, ord(alt) | ord(ref) << 8) for g, ref, alt in got]
    return calls, recs


# ---------------------------------------------------------------------------------------------------------------- the tool's files
def merge(solo, multi):
    """what the tool does with its two SNP lists: both observers are asked at right + 1 of their gap and no gap is a candidate of both, so
    the lists merge by (seq, right); the SNPs of one gap stay in ascending order"""
    return sorted(list(solo) + list(multi), key=lambda c: (c[0], c[5], c[1]))


def lines(calls, names):
    """record lines of prefix.othervariants.vcf for SNP calls of kind 5 and 6 in detection order, ids from 1; prefix.breakpoints stays empty"""
    return [fs.snp_line(c, n, names) for n, c in enumerate(calls, 1)]


# ---------------------------------------------------------------------------------------------------------------- synthetic cases
def competing_cases(k, seed, n_seqs, length=None):
    """[(sequence, solid set)]: the set holds the k-mers of two or three donors of the sequence.  The donors substitute at shared places
    (each with a nucleotide of its own choice, so that alternatives compete) and at places of their own; every sixth sequence has the
    shared places k apart and nothing else, so that more than one alternative holds all k windows.  At small k the k-mers of the donors
    also hold windows by chance"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_seqs):
        n = (4 * k + 60 + int(rng.integers(0, 60))) if length is None else length
        seq = fc.rand_seq(rng, n)
        lo, hi = 2 * k, n - 2 * k
        if i % 6 == 5:
            shared, own = list(range(lo, hi, k)), 0.0
        else:
            shared, own = [p for p in range(lo, hi) if rng.random() < 0.08], 0.04
        solid = set()
        for d in range(2 + i % 2):
            don = list(seq)
            for p in shared:
                if own == 0.0 or rng.random() < 0.8:
                    don[p] = fs.other(rng, seq[p])
            for p in range(lo, hi):
                if rng.random() < own:
                    don[p] = fs.other(rng, seq[p])
            solid |= fc.solid_of_strings(["".join(don)], k)
        out.append((seq, solid))
    return out


def long_gap_case(rng, k, start, length, step_lo=None):
    """(sequence, solid set of one donor): substitutions from g = start + k - 1 on, no more than k apart, the last at g + length - k, so
    that there is one gap of `length` positions from `start`; the sequence ends k + 1 nucleotides behind the gap.  Returns the number of
    substitutions as well; they are step_lo (default k - 6) .. k apart"""
    span, offs, lo = length - k, [0], step_lo or max(1, k - 6)
    while offs[-1] < span:
        rem, step = span - offs[-1], int(rng.integers(lo, k + 1))
        if rem <= k:
            step = rem                       # the last one
        elif rem - step < lo:
            step = max(rem - lo, lo)         # leave at least step_lo for the last one (k >= 2 step_lo - 1)
        offs.append(offs[-1] + step)
    seq = fc.rand_seq(rng, start + length + k + 1)
    don = list(seq)
    for o in offs:
        don[start + k - 1 + o] = fs.other(rng, seq[start + k - 1 + o])
    return seq, fc.solid_of_strings(["".join(don)], k), len(offs)
