"""A plain model of `find` for close homozygous SNPs with the reverse pass (include/mtg_fill.h: mtg_index_find_msnp_rev_sequences), to judge the
device's calls.

THE LITERAL MODEL (RevRingScan) extends find_msnp_cases.RingScan -- the real ring of 256 slots, the solo and the forward multi-SNP observer --
with FindSNP::snp_at_begin (src/FindSNP.hpp:219-293) and FindMultiSNPrev::update (:593-689) with its correct_history (:693-709) as they
stand: every index & 255, the entry test on the gap the forward observer left, the subtraction of the consumed length from m_position,
m_het_kmer_end_index and m_het_kmer_begin_index after a partial take (:672-674), the corrected kmer_end.  Registration order is solo, multi,
rev (src/Finder.cpp:551-554).  The scan restores m_position after the observers (src/FindBreakpoints.hpp:441-446); `restore_indices` says
whether the two ring indices are restored with it: False is the reference as it stands, True is what the product is held to (the deviation of
mtg_find_msnp.h: the ring indices count as restored after a gap).

THE CLOSED FORM (closed_form_rev, find_by_closed_form) is the rule as the header states it, forward then reverse on one private text, with
switches that make the wrong models.

A call is (seq, pos, kind, repeat, left, right, ins): kind 6 as in find_msnp_cases; kind 7, a reverse call, has pos = q, repeat = 0,
left = start + c - 1 (the k-mer before the residual gap), right = start + L.  A gap record is (seq, start, length, consumed, n_snps,
consumed_rev, n_snps_rev); the gap is full if consumed + consumed_rev = length."""
from tests import find_cases as fc
from tests import find_msnp_cases as fm

MAX_GAP = fm.MAX_GAP
STAT_KEYS = fm.STAT_KEYS

PASSES = {1: ("multi",), 2: ("rev",), 3: ("multi", "rev")}
OBSERVERS = {"-rev-snps": ("rev",), "-multi-snps -rev-snps": ("multi", "rev"), "-solo-snps -rev-snps": ("solo", "rev"), "-solo-snps -multi-snps -rev-snps": ("solo", "multi", "rev")}


class RevRingScan(fm.RingScan):
    restore_indices = True

    def __init__(self, graph, max_repeat, observers, snp_min_val):
        fm.RingScan.__init__(self, graph, max_repeat, observers, snp_min_val)
        self.rev_seen = {"steps": 0, "calls": 0, "tie_below_k": 0, "two_reach_k": 0, "beyond_stop": 0, "anchor_stop": 0, "full_take": 0, "partial_fwd_then_rev_call": 0,
                         "meet_exactly": 0, "rev_calls_left_partial": 0}

    # ---- FindBreakpoints
    def het_kmer_end_index(self):
        return self.end_index & 255

    # ---- FindSNP.hpp:219-293; returns (found, beginpos, ret_nuc, ref_nuc, nb_kmer_val)
    def snp_at_begin_count(self, beginpos, limit):
        k = self.k
        nuc = {0: 0, 1: 0, 2: 0, 3: 0}
        beginpos_init = beginpos
        ref_nuc = self.CODES.index(self.het_kmer_history(beginpos)[0])   # kmer >> 2(k - 1) & 3 on a gatb k-mer: its first nucleotide
        del nuc[ref_nuc]
        counts = {}
        end = False
        j = 0
        while not end and j != k:
            for n in sorted(nuc):
                correct_kmer = self.mutate_kmer(self.het_kmer_history(beginpos), n, j + 1)
                if self.g.contains(correct_kmer):
                    nuc[n] += 1
                else:
                    if len(nuc) == 1:
                        end = True
                        beginpos = (beginpos + 1) & 255
                        break
                    counts[n] = nuc[n]
                    del nuc[n]
            beginpos = (beginpos - 1) & 255
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

    # ---- FindSNP.hpp:593-689
    def rev(self):
        if self.kmer_begin is None or self.kmer_end is None:
            return False
        k, m = self.k, self.snp_min_val
        start, length = self.gap_orig
        if length > MAX_GAP and not self.judge_long:
            if "multi" not in self.observer_names and length > k + m:
                self.n_long += 1
                self.gap_records.append((self.s, start, length, 0, 0))
            return False
        if self.gap_stretch > k + m:
            consumed_fwd = length - self.gap_stretch
            if "multi" not in self.observer_names:
                self.gap_records.append((self.s, start, length, 0, 0))
            nb_snp = 0
            begin_pos = self.position - 2
            begin_pos_init = begin_pos
            index_limit = (self.het_kmer_end_index() - 2 - self.gap_stretch) & 255
            index_pos = (self.het_kmer_end_index() - 2) & 255
            left, right = start + consumed_fwd - 1, self.kmer_end
            seen = self.rev_seen
            while index_pos != index_limit:
                save_index = index_pos
                found, index_pos, nuc, ref_nuc, nb_kmer_val = self.snp_at_begin_count(index_pos, m)
                seen["steps"] += 1
                f = sorted(self.last_counts.values())
                if found and f[-1] == f[-2] and m <= f[-1] < k:
                    seen["tie_below_k"] += 1
                if f[-2] == k:
                    seen["two_reach_k"] += 1
                if found:
                    if begin_pos_init - (begin_pos - nb_kmer_val) > self.gap_stretch:
                        seen["beyond_stop"] += begin_pos < begin_pos_init
                        seen["anchor_stop"] += 1
                        break
                    self.correct_history((save_index - (k - 1)) & 255, nuc)
                    nb_snp += 1
                    ins = ord(self.CODES[nuc]) | (ord(self.CODES[ref_nuc]) << 8)
                    self.calls.append((self.s, begin_pos, 7, 0, left, right, ins))
                    seen["calls"] += 1
                    begin_pos -= nb_kmer_val
                else:
                    break
            nb_kmer_correct = begin_pos_init - begin_pos
            self.rev_result = (nb_kmer_correct, nb_snp)
            fwd_snps = self.gap_records[-1][4]
            seen["full_take"] += consumed_fwd == 0 and nb_kmer_correct == length
            seen["partial_fwd_then_rev_call"] += consumed_fwd > 0 and nb_snp > 0
            seen["meet_exactly"] += fwd_snps > 0 and nb_snp > 0 and consumed_fwd + nb_kmer_correct == length
            seen["rev_calls_left_partial"] += nb_snp > 0 and consumed_fwd + nb_kmer_correct < length
            if nb_kmer_correct == 0:
                return False
            if nb_kmer_correct != self.gap_stretch:
                self.position -= nb_kmer_correct
                self.end_index -= nb_kmer_correct
                self.begin_index -= nb_kmer_correct
                self.gap_stretch -= nb_kmer_correct
                self.kmer_end = ("corrected", self.het_kmer_history(index_pos + 1))
                return False
            return True
        return False

    # the first slot of the base class's observer tuple: solo, multi, rev (src/Finder.cpp:551-554); nothing else is in scope with rev.  The
    # record of a candidate gap -- by the gap as the scan reports it -- is completed here
    def small_clean(self):
        self.gap_orig = (self.position - 1 - self.gap_stretch, self.gap_stretch)
        self.rev_result = (0, 0)
        n0 = len(self.gap_records)
        saved = (self.position, self.end_index, self.begin_index)
        taken = False
        for name, ob in (("solo", self.solo), ("multi", self.multi), ("rev", self.rev)):
            if name in self.observer_names and ob():
                taken = True
                break
        self.position = saved[0]                     # src/FindBreakpoints.hpp:441-446
        if self.restore_indices:
            self.end_index, self.begin_index = saved[1], saved[2]
        if len(self.gap_records) > n0:
            self.gap_records[-1] = self.gap_records[-1][:5] + self.rev_result
        return taken


class AsIsRevRingScan(RevRingScan):
    """the reference as it stands: the ring indices stay shifted after a partial reverse take"""
    restore_indices = False


def scan(solid, k, seqs, snp_min_val=5, passes=3, max_repeat=5, solo=False, cls=RevRingScan):
    if max_repeat > k - 2:
        max_repeat = k - 2
    names = (("solo",) if solo else ()) + PASSES[passes]
    sc = cls(fc.Graph(solid, k), max_repeat, names, snp_min_val)
    for s, seq in enumerate(seqs):
        sc.run_sequence(s, seq)
    return sc


def stats_of(sc):
    recs = sc.gap_records
    return {"n_gaps": sc.gaps, "n_candidates": len(recs), "n_calls": sum(1 for c in sc.calls if c[2] in (6, 7)),
            "n_full": sum(1 for r in recs if r[3] + r[5] == r[2]), "n_partial": sum(1 for r in recs if 0 < r[3] + r[5] < r[2]), "n_long": sc.n_long}


def find_msnp_rev(solid, k, seqs, snp_min_val=5, passes=3, max_repeat=5, cls=RevRingScan):
    """(calls in detection order, gap records in scan order, statistics) of the passes alone"""
    sc = scan(solid, k, seqs, snp_min_val, passes, max_repeat, False, cls)
    return sc.calls, sc.gap_records, stats_of(sc)


# ---------------------------------------------------------------------------------------------------------------- the closed form
def closed_form_rev(graph, t, start, length, c, k, m, forward_text=False, ref_last=False, reads=None):
    """(calls [(pos, REF, ALT)] in the order made, consumed_rev) of the reverse pass on the text t (a list, CHANGED by the calls) of a gap
    of `length` from `start` of which the forward pass consumed c.  Wrong models: the text begins at `start`, so that the anchor window reads
    the k-mer at `start` in place of the one at start - 1; ref taken from the last nucleotide of the k-mer at q.  reads, a list, receives
    the first text position of every window looked at"""
    left = length - c
    d, calls = 0, []
    while d != left:
        q = start + length - 1 - d
        ref = t[q + k - 1] if ref_last else t[q]
        cap = min(k, left - d + 1)
        f = {}
        for a in "ACTG":
            if a == ref:
                continue
            j = 0
            while j < cap:
                p = q - j
                if forward_text and p < start:
                    p = start
                if reads is not None:
                    reads.append(p)
                w = t[p:p + k]
                w[j] = a
                if not graph.contains("".join(w)):
                    break
                j += 1
            f[a] = j
        best = max(f.values())
        tied = [a for a in "ACTG" if a != ref and f[a] == best]
        win = tied[0] if best == k else tied[-1]
        if best < m or d + best > left:
            break
        calls.append((q, ref, win))
        t[q] = win
        d += best
    return calls, d


def closed_form(graph, seq, start, length, k, m, passes=3, ascending=False, no_forward_subst=False, no_entry_test=False, **wrong):
    """(forward calls, consumed, reverse calls, consumed_rev) of one gap.  Wrong models beyond those of closed_form_rev: the reverse calls in
    ascending order; the reverse pass on the text without the forward substitutions; the entry test L - c > k + m dropped"""
    fwd, c = fm.closed_form(graph, seq, start, length, k, m) if passes & 1 else ([], 0)
    t = list(seq.upper())
    if not no_forward_subst:
        for g, ref, alt in fwd:
            t[g] = alt
    rev, d = [], 0
    if passes & 2 and c != length and (no_entry_test or length - c > k + m):
        rev, d = closed_form_rev(graph, t, start, length, c, k, m, **wrong)
    if ascending:
        rev = sorted(rev)
    return fwd, c, rev, d


def find_by_closed_form(solid, k, seqs, m, passes=3, **wrong):
    """(calls, gap records) as find_msnp_rev gives them, every candidate judged by the closed form; gaps of 255 and more are not judged"""
    graph = fc.Graph(solid, k)
    calls, recs = [], []
    for s, p, n in fm.candidates(solid, k, seqs, m):
        if n > MAX_GAP:
            recs.append((s, p, n, 0, 0, 0, 0))
            continue
        fwd, c, rev, d = closed_form(graph, seqs[s], p, n, k, m, passes, **wrong)
        recs.append((s, p, n, c, len(fwd), d, len(rev)))
        calls += [(s, g, 6, 0, p - 1, p + n, ord(alt) | ord(ref) << 8) for g, ref, alt in fwd]
        calls += [(s, q, 7, 0, p + c - 1, p + n, ord(alt) | ord(ref) << 8) for q, ref, alt in rev]
    return calls, recs


# ---------------------------------------------------------------------------------------------------------------- the tool's files
def merge(solo, multi):
    """what the tool does with its two SNP lists: they merge by (seq, right); the calls of one gap keep the order of their list (forward
    ascending, then reverse descending) and are not sorted by pos"""
    tagged = [((c[0], c[5]), 0, i, c) for i, c in enumerate(solo)] + [((c[0], c[5]), 1, i, c) for i, c in enumerate(multi)]
    return [c for _, _, _, c in sorted(tagged, key=lambda x: x[:3])]


def lines(calls, names):
    return fm.lines(calls, names)


def two_behind(recs):
    """a gap of the records starts exactly two positions behind the end of another of the same sequence"""
    ends = {(r[0], r[1] + r[2] + 2) for r in recs}
    return any((r[0], r[1]) in ends for r in recs)
