"""A plain model of `find` for heterozygous insertions (include/mtg_fill.h: mtg_index_find_het_sequences), to judge the device's calls.

It is the reference's k-mer observer FindHeteroInsertion::update (src/FindHeteroInsertion.hpp:46-174) written out as it stands, inside the
loop of FindBreakpoints::operator() (src/FindBreakpoints.hpp:390-455) with store_kmer_info (:1012-1046): a real ring of 256 history slots
indexed by two unsigned bytes, zeroed per sequence and written at valid positions only, and the counter m_recent_hetero.  No other observer
runs -- the configuration of -hete-only, and of -insert-only as far as this observer is concerned, since the gap observers write nothing it
reads.  The graph is find_cases.Graph, the micro-assembly find_cases.Scan.micro_assembly, the repeated (k-1)-mers an exact set counted in
plain Python (the reference asks a Bloom filter of that set).

A call is the tuple (seq, pos, kind, repeat, left, right, ins) of mtg_find_call: kind 2 = heterozygous site, 3 = heterozygous insertion of
1-2 nt, pos as the observer passes it to writeBreakpoint / writeIndel, left = position whose text the history slot holds, right = p + i."""
from collections import Counter

from tests import find_cases as fc

STAT_KEYS = ("n_candidates", "n_raw_sites", "n_filtered", "n_suppressed", "n_het_clean", "n_het_fuzzy", "n_het_small")


def repeated_set(seqs, k, het_max_occ=1):
    """the canonical (k-1)-mers that occur at least het_max_occ + 1 times in the sequences, over all of them and both strands"""
    n = Counter()
    for s in seqs:
        up = s.upper()
        for q in range(len(up) - (k - 1) + 1):
            w = up[q:q + k - 1]
            if fc.is_valid(w):
                n[fc.canon_of(w)] += 1
    return {c for c, v in n.items() if v >= het_max_occ + 1}


def repeat_flags(seqs, k, rep):
    """per sequence one flag per (k-1)-mer position (len - k + 2 of them): the (k-1)-mer there is valid and in the set"""
    out = []
    for s in seqs:
        up = s.upper()
        out.append(bytes(1 if fc.is_valid(up[q:q + k - 1]) and fc.canon_of(up[q:q + k - 1]) in rep else 0 for q in range(max(len(up) - k + 2, 0))))
    return out


class HetScan:
    def __init__(self, graph, max_repeat, branching_filter, flags):
        self.g, self.k, self.max_repeat, self.branching = graph, graph.k, max_repeat, branching_filter
        self.flags = flags   # None: nothing is repeated
        self.assembler = fc.Scan(graph, max_repeat)
        self.calls = []
        self.st = dict.fromkeys(STAT_KEYS, 0)

    def rep(self, s, q):
        return bool(self.flags is not None and self.flags[s][q])

    def judge(self, p):
        """the body of update() behind its first test, as if m_recent_hetero were 0: (outcome, i, left, ins); outcome None when no slot
        qualifies, "return" for the early return on an invalid right k-mer, else "ins", "site" or "filtered" """
        k = self.k
        for i in range(self.max_repeat + 1):
            left, nb_in, nb_out, is_repeated = self.hist[(self.begin_index + i) & 255]
            if nb_out == 2 and not is_repeated:
                kmer_begin_str = self.up[left:left + k]
                kmer_end_str = self.up[p + i:p + i + k]       # (the text as it stands; the assembly does not see the case)
                if len(kmer_end_str) < k or not fc.is_valid(kmer_end_str):
                    return "return", i, left, 0
                a = self.assembler.micro_assembly(kmer_begin_str, kmer_end_str)
                if a is not None:
                    return "ins", i, left, a
                filtering, max_branching = self.branching >= 0, self.branching if self.branching >= 0 else 100
                nb_branching = 0
                if filtering:
                    nb_prev, begin = 0, (self.begin_index - 1) & 255
                    while nb_branching <= max_branching and nb_prev < 100:
                        h = self.hist[(begin - nb_prev) & 255]
                        if h[2] > 1 or h[1] > 1:
                            nb_branching += 1
                        nb_prev += 1
                return ("site" if nb_branching <= max_branching else "filtered"), i, left, 0
        return None, 0, 0, 0

    def run_sequence(self, s, seq):
        k = self.k
        self.up = seq.upper()
        self.hist = [(0, 0, 0, False)] * 256         # memset(m_het_kmer_history, 0, ...)
        self.end_index, self.begin_index = (k + 1) & 255, 1
        recent = 0
        for p in range(len(self.up) - k + 1):
            w = self.up[p:p + k]
            if fc.is_valid(w):
                present = self.g.contains(w)
                nb_in = self.g.indegree(w) if present else 0
                nb_out = self.g.outdegree(w) if present else 0
                self.hist[self.end_index] = (p, nb_in, nb_out, self.rep(s, p + 1))   # store_kmer_info: the suffix's flag
                kmer_end_is_repeated = self.rep(s, p)                                  # the prefix's flag
                # FindHeteroInsertion::update
                fired = False
                if not kmer_end_is_repeated and nb_in == 2:
                    outcome, i, left, a = self.judge(p)
                    self.st["n_candidates"] += outcome is not None
                    self.st["n_raw_sites"] += outcome == "site"
                    if recent != 0:
                        self.st["n_suppressed"] += outcome in ("site", "ins")     # what the counter silences (the reference does not look)
                    elif outcome == "return":
                        fired = True
                    elif outcome == "ins":
                        self.calls.append((s, p - 1, 3, i, left, p + i, a))
                        self.st["n_het_small"] += 1
                        fired = True
                    elif outcome == "site":
                        self.calls.append((s, p - 1 + i, 2, i, left, p + i, 0))
                        self.st["n_het_clean" if i == 0 else "n_het_fuzzy"] += 1
                        recent = self.max_repeat
                        fired = True
                    elif outcome == "filtered":
                        self.st["n_filtered"] += 1
                        recent = max(0, recent - 1)
                        fired = True
                if not fired:
                    recent = max(0, recent - 1)
            self.begin_index = (self.begin_index + 1) & 255
            self.end_index = (self.end_index + 1) & 255


def find_het(solid, k, seqs, flags=None, max_repeat=5, branching_filter=15):
    """(calls as a list of tuples in detection order, statistics) of the literal scan; flags: repeat_flags(...) or None"""
    if max_repeat > k - 2:
        max_repeat = k - 2   # the library's rule for larger values
    sc = HetScan(fc.Graph(solid, k), max_repeat, branching_filter, flags)
    for s, seq in enumerate(seqs):
        sc.run_sequence(s, seq)
    return sc.calls, sc.st


# ---------------------------------------------------------------------------------------------------------------- the tool's files
def detected_at(call):
    """where the scan stood when the call was made, and which family of observers made it: k-mer observers (heterozygous) run before gap
    observers (homozygous) at the same position (src/FindBreakpoints.hpp:566-590)"""
    s, pos, kind, repeat, left, right, ins = call
    return (s, right - repeat, 0) if kind >= 2 else (s, right - repeat + 1, 1)


def merge(homo, het):
    """the calls of both layers in detection order (-insert-only)"""
    return sorted(list(homo) + list(het), key=detected_at)


def lines(calls, names, seqs, k):
    """(lines of prefix.breakpoints, record lines of prefix.othervariants.vcf) for calls of all four kinds in detection order; ids count from 1
    across both files; the REPEATED fields are empty"""
    bk, vcf = [], []
    for n, c in enumerate(calls, 1):
        s, pos, kind, repeat, left, right, ins = c
        if kind < 2:
            b, v = fc.breakpoint_lines([c], names, seqs, k)
            bk += [x.replace(">bkpt1_", ">bkpt%d_" % n, 1) for x in b]
            vcf += [x.replace("\tbkpt1\t", "\tbkpt%d\t" % n, 1) for x in v]
            continue
        lk = seqs[s].upper()[left:left + k]     # model().toString: upper case
        rk = seqs[s][right:right + k]           # string(&chrom_seq[position + i], k): the genome's text as it stands
        if kind == 2:
            head = ">bkpt%d_%s_pos_%d_fuzzy_%d_HET" % (n, names[s], pos + 1, repeat)
            bk += [head + "  left_kmer", lk, head + "  right_kmer", rk]
        else:
            ref = lk[k - 1 - repeat]
            vcf.append("%s\t%d\tbkpt%d\t%s\t%s\t.\tPASS\tTYPE=INS;LEN=%d;FUZZY=%d\tGT\t0/1" % (names[s], pos + 1, n, ref, ref + fc.INSERTIONS[ins], len(fc.INSERTIONS[ins]), repeat))
    return bk, vcf
