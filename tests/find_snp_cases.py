"""A plain model of `find` for isolated homozygous SNPs (include/mtg_fill.h: mtg_index_find_snp_sequences), to judge the device's calls.

It is the reference's gap observer FindSoloSNP::update (src/FindSNP.hpp:319-355) with FindSNP::snp_at_end (:139-208) and mutate_kmer (:88-96)
written out as they stand -- the map of the surviving nucleotides, its erasure, `limit` and the search for the best count -- run inside the
loop of find_cases.Scan.run_sequence ahead of the deletion observer, as the reference registers it first (src/Finder.cpp:551).  The k-mer
history that snp_at_end reads is the reference's ring m_het_kmer_history, written at slot k + 1 + p for position p
(src/FindBreakpoints.hpp:406-407,423,1037); here it is the sequence itself, read at the same index.  correct_history (:357), the call's
effect on what the heterozygous observer reads later, is not modelled: no configuration in scope runs both.

A call is the tuple (seq, pos, kind, repeat, left, right, ins) of mtg_find_call with kind 5: pos = 0-based position of the SNP
(position() - 2, what the observer passes to writeVcfVariant), repeat = 0, left / right = positions of kmer_begin / kmer_end,
ins = ord(ALT) | ord(REF) << 8, both upper case (nuc_to_char, :99-117)."""
from tests import find_cases as fc
from tests import find_del_cases as fd

STAT_KEYS = ("n_gaps", "n_candidates", "n_calls")

# "-solo-snps" and "-homo-only -solo-snps" are configurations of this project's tool, not of the reference: its registration order
# (src/Finder.cpp:549-582) without the two multi-SNP observers
OBSERVERS = dict(fd.OBSERVERS)
OBSERVERS.update({
    "-solo-snps": ("solo",),
    "-homo-only -solo-snps": ("solo", "deletion", "small_clean", "small_fuzzy", "clean", "fuzzy"),
    "solo": ("solo",),
})


class SnpScan(fd.DelScan):
    CODES = "ACTG"   # nuc_to_char: A = 0, C = 1, T = 2, G = 3, the order of the std::map's keys

    def __init__(self, graph, max_repeat, observers):
        fd.DelScan.__init__(self, graph, max_repeat, observers)
        self.snp_candidates = 0
        self.snp_calls = 0

    # ---- FindBreakpoints: the history, slot k + 1 + p for the k-mer at position p; begin index = 1 + position
    def het_kmer_begin_index(self):
        return self.position + 1

    def het_kmer_history(self, index):
        p = index - (self.k + 1)
        return self.seq[p:p + self.k]

    # ---- FindSNP.hpp:88-96: pos is 1-based from the start of the k-mer
    def mutate_kmer(self, kmer, nuc, pos):
        return kmer[:pos - 1] + self.CODES[nuc] + kmer[pos:]

    # ---- FindSNP.hpp:139-208; returns (found, beginpos, ret_nuc, ref_nuc)
    def snp_at_end(self, beginpos, limit):
        k = self.k
        nuc = {0: 0, 1: 0, 2: 0, 3: 0}
        beginpos_init = beginpos
        ref_nuc = self.CODES.index(self.het_kmer_history(beginpos)[-1])
        del nuc[ref_nuc]
        end = False
        j = 0
        while not end and j != k:
            for n in sorted(nuc):        # the map's iteration; an erased key is the one just visited
                correct_kmer = self.mutate_kmer(self.het_kmer_history(beginpos), n, k - j)
                if self.g.contains(correct_kmer):
                    nuc[n] += 1
                else:
                    if len(nuc) == 1:
                        end = True
                        beginpos -= 1
                        break
                    del nuc[n]
            beginpos += 1
            j += 1
        best = sorted(nuc)[0]
        for n in sorted(nuc):
            if nuc[n] > nuc[best]:
                best = n
        if nuc[best] >= limit:
            return True, beginpos, best, ref_nuc
        return False, beginpos_init, None, ref_nuc

    # ---- FindSNP.hpp:319-355
    def solo(self):
        if self.kmer_begin is None or self.kmer_end is None:
            return False
        if self.gap_stretch == self.k:
            self.snp_candidates += 1
            pos = self.het_kmer_begin_index() - 1
            found, pos, nuc, ref_nuc = self.snp_at_end(pos, self.k)
            if found:
                ins = ord(self.CODES[nuc]) | (ord(self.CODES[ref_nuc]) << 8)
                self.calls.append((self.s, self.position - 2, 5, 0, self.kmer_begin, self.kmer_end, ins))
                self.snp_calls += 1
                return True
        return False

    # the first slot of the base class's observer tuple: the solo observer goes before the deletion observer
    def small_clean(self):
        if "solo" in self.observer_names and self.solo():
            return True
        return fd.DelScan.small_clean(self)


def scan(solid, k, seqs, max_repeat, observers, cls=SnpScan):
    """the literal scan with a list of observers (a key of OBSERVERS or a tuple of names): the scan object after all sequences"""
    if max_repeat > k - 2:
        max_repeat = k - 2
    sc = cls(fc.Graph(solid, k), max_repeat, OBSERVERS.get(observers, observers))
    for s, seq in enumerate(seqs):
        sc.run_sequence(s, seq)
    return sc


def find_snp(solid, k, seqs, max_repeat=5, cls=SnpScan):
    """(calls as a list of tuples in detection order, statistics) of the solo observer alone"""
    sc = scan(solid, k, seqs, max_repeat, "solo", cls)
    return sc.calls, {"n_gaps": sc.gaps, "n_candidates": sc.snp_candidates, "n_calls": len(sc.calls)}


def find_gap_family(solid, k, seqs, max_repeat, config):
    """the calls of all gap observers of a configuration in one literal scan, in detection order"""
    return scan(solid, k, seqs, max_repeat, config).calls


def closed_form(graph, seq, start, k, order="ACTG"):
    """what the header states in place of the map: the first nucleotide in `order`, the sequence's own left out, for which the k k-mers at
    start .. start + k - 1 with position start + k - 1 replaced are all in the graph; None for none"""
    g = start + k - 1
    up = seq.upper()
    for a in order:
        if a == up[g]:
            continue
        changed = up[:g] + a + up[g + 1:]
        if all(graph.contains(changed[start + j:start + j + k]) for j in range(k)):
            return a
    return None


# ---------------------------------------------------------------------------------------------------------------- the tool's files
def detected_at(call):
    """where the scan stood when the call was made and the observer family: a solo call is made by the gap observers at right + 1"""
    return (call[0], call[5] + 1, 1) if call[2] == 5 else fd.detected_at(call)


def merge(homo, dels, snps):
    """what the tool does with the lists of its gap layers: every deletion call on a gap with a solo call -- equal (seq, left) -- is dropped,
    then every homozygous insertion call on a gap with a call of either, and the rest is put in detection order"""
    taken = {(c[0], c[4]) for c in snps}
    first = [c for c in dels if (c[0], c[4]) not in taken] + list(snps)
    taken = {(c[0], c[4]) for c in first}
    return sorted([c for c in homo if (c[0], c[4]) not in taken] + first, key=detected_at)


def snp_line(call, n, names):
    s, pos, kind, repeat, left, right, ins = call
    return "%s\t%d\tbkpt%d\t%s\t%s\t.\tPASS\tTYPE=SNP;LEN=1;FUZZY=0\tGT\t1/1" % (names[s], pos + 1, n, chr((ins >> 8) & 255), chr(ins & 255))


def lines(calls, names, seqs, k):
    """(lines of prefix.breakpoints, record lines of prefix.othervariants.vcf) for calls in detection order; ids count from 1 across both
    files.  A SNP is one VCF line (writeVcfVariant, src/FindBreakpoints.hpp:661-678) with REF and ALT from the 2-bit codes"""
    bk, vcf = [], []
    for n, c in enumerate(calls, 1):
        if c[2] == 5:
            vcf.append(snp_line(c, n, names))
            continue
        b, v = fd.lines([c], names, seqs, k)
        bk += [x.replace(">bkpt1_", ">bkpt%d_" % n, 1) for x in b]
        vcf += [x.replace("\tbkpt1\t", "\tbkpt%d\t" % n, 1) for x in v]
    return bk, vcf


# ---------------------------------------------------------------------------------------------------------------- synthetic cases
def other(rng, ch):
    return "ACGT"[("ACGT".index(ch) + 1 + int(rng.integers(3))) % 4]


def substituted(seq, g, a):
    return seq[:g] + a + seq[g + 1:]


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def overlap_case(rng, length, g):
    """(reference, donor with a SNP at g, donor with ref[g] deleted): ref[g - 1] != ref[g] != ref[g + 1], so that the deletion has no
    junction repeat and leaves a gap of exactly k, the SNP's gap"""
    ref = list(fc.rand_seq(rng, length))
    while ref[g - 1] == ref[g]:
        ref[g - 1] = other(rng, ref[g])
    while ref[g + 1] == ref[g]:
        ref[g + 1] = other(rng, ref[g])
    ref = "".join(ref)
    alt = other(rng, ref[g])
    return ref, substituted(ref, g, alt), ref[:g] + ref[g + 1:], alt
