"""The smallest inputs that take every exit of the five `find` runs (homozygous insertions, homozygous deletions, isolated SNPs, close SNPs,
heterozygous insertions), which share one skeleton on the device (FindStage in csrc/mtg_gpu_misc.hip): k = 13, at most four sequences of at most
200 nt, one graph for all.

STAGES[layer][stage] = the sequences.  The stages, in the order of the run's exits:
  none        no sequence at all
  short       only sequences shorter than k: no position, no gap, no candidate
  in_graph    a sequence that lies wholly in the graph
  unseen      something the layer's first pass looks at, nothing of it a candidate -- homo: a gap longer than k - 1; del: gaps shorter than
              k - max_repeat; snp: no gap of exactly k positions between two anchors; msnp: no gap longer than k + snp_min_val; het: a position
              of in-degree 2 without a k-mer of out-degree 2 k positions before it
  uncalled    candidates, none of them called
  calls       at least three calls
UNJUDGED: one stage more of the multi-SNP layer, a single sequence of at most 320 nt whose only candidate gap has 255 positions or more: it
is counted (n_long) and not judged, so the run has candidates and nothing to list.
ALL_LAYERS: sequences on which every layer makes a call.  tests/test_find_stages_cpu.py shows with the models alone that every input is what its
name says; tests/test_gpu_find_stages.py runs them on the device."""
import numpy as np

from tests import find_cases as fc
from tests import find_del_cases as fd
from tests import find_het_cases as fh
from tests import find_msnp_cases as fm
from tests import find_snp_cases as fs

K, MAX_REPEAT, BRANCHING, SNP_MIN_VAL = 13, 5, 15, 5
LAYERS = ("homo", "del", "snp", "msnp", "het")
STAGE_NAMES = ("none", "short", "in_graph", "unseen", "uncalled", "calls")


def model(layer, solid, seqs):
    """(calls, statistics) of the layer's plain model"""
    if layer == "homo":
        return fc.find_homo(solid, K, seqs, MAX_REPEAT)
    if layer == "del":
        return fd.find_del(solid, K, seqs, MAX_REPEAT)
    if layer == "snp":
        return fs.find_snp(solid, K, seqs, MAX_REPEAT)
    if layer == "msnp":
        calls, _, st = fm.find_msnp(solid, K, seqs, SNP_MIN_VAL, MAX_REPEAT)
        return calls, st
    return fh.find_het(solid, K, seqs, None, MAX_REPEAT, BRANCHING)


def msnp_gap_records(solid, seqs):
    """the multi-SNP model's records of its candidate gaps, (seq, start, length, consumed, n_snps) in scan order"""
    return fm.find_msnp(solid, K, seqs, SNP_MIN_VAL, MAX_REPEAT)[1]


def stat_keys(layer):
    return {"homo": ("n_gaps", "n_candidates", "n_homo_clean", "n_homo_fuzzy", "n_small_clean", "n_small_fuzzy"), "del": fd.STAT_KEYS, "snp": fs.STAT_KEYS, "msnp": fm.STAT_KEYS,
            "het": fh.STAT_KEYS}[layer]


def inputs(layer):
    """{stage: sequences} of a layer, UNJUDGED among them where the layer has it"""
    return dict(STAGES[layer], unjudged=UNJUDGED) if layer == "msnp" else STAGES[layer]


def in_degree_2_positions(solid, seqs):
    g = fc.Graph(solid, K)
    return sum(g.contains(s[p:p + K]) and g.indegree(s[p:p + K]) == 2 for s in seqs for p in range(len(s) - K + 1))


def _other(ch, step=1):
    return "ACGT"[("ACGT".index(ch) + step) % 4]


def _build():
    rng = np.random.default_rng(1300)
    solid, stages = set(), {layer: {"none": [], "short": ["ACGT", "", "ACGTTGCAACGT"]} for layer in LAYERS}
    know = lambda *strings: solid.update(fc.solid_of_strings(strings, K))  # noqa: E731

    plain = fc.rand_seq(rng, 150)
    know(plain)
    for layer in LAYERS:
        stages[layer]["in_graph"] = [plain, "ACG"]

    # a substitution: a gap of k positions -- too long for the insertion observers, a deletion candidate that nothing in the graph joins
    snp = fc.rand_seq(rng, 120)
    know(snp)
    snp = snp[:60] + _other(snp[60]) + snp[61:]
    stages["homo"]["unseen"] = stages["msnp"]["unseen"] = [snp]
    stages["del"]["uncalled"] = [snp, "ACGT"]
    # two texts of the graph one behind the other: a gap of k - 1 between a k-mer without a successor and one without a predecessor
    a, b = fc.rand_seq(rng, 70), fc.rand_seq(rng, 70)
    know(a, b)
    stages["homo"]["uncalled"] = [a + b, plain[:40]]
    stages["snp"]["unseen"] = [a + b]
    # an insertion in the graph with a junction repeat of 7: a gap of k - 1 - 7 positions
    donor = fc.with_repeat(rng, fc.rand_seq(rng, 170), 80, 20, 7)
    know(donor)
    stages["del"]["unseen"] = [fc.planted(rng, donor, K, [(80, 20)])]

    # homozygous insertions: a site, a fuzzy site and an insertion of 1 nt, one per sequence
    stages["homo"]["calls"] = []
    for n, r in ((20, 0), (9, 2), (1, 0)):
        donor = fc.with_repeat(rng, fc.rand_seq(rng, 150 + n), 66, n, r)
        know(donor)
        stages["homo"]["calls"].append(fc.planted(rng, donor, K, [(66, n)]))
    # homozygous deletions of 5, 20 and 40 nt
    stages["del"]["calls"] = []
    for n, r in ((5, 0), (20, 2), (40, 0)):
        seq = fd.with_del_repeat(rng, fc.rand_seq(rng, 150 + n), 70, n, r)
        know(fd.deleted(seq, 70, n))
        stages["del"]["calls"].append(seq)
    stages["del"]["calls"].append("ACGTACGTACGT")
    # heterozygous insertions: the graph knows the sequence and the donor
    stages["het"]["calls"] = []
    for n, r in ((20, 0), (9, 2), (1, 0)):
        donor = fc.with_repeat(rng, fc.rand_seq(rng, 150 + n), 66, n, r)
        ref = fc.planted(rng, donor, K, [(66, n)])
        know(donor, ref)
        stages["het"]["calls"].append(ref)
    # ... and one with a repeat of 2 whose sequence ends with the k-mer the observer fires at: the right k-mer, 2 further on, is not there
    donor = fc.with_repeat(rng, fc.rand_seq(rng, 159), 66, 9, 2)
    ref = fc.planted(rng, donor, K, [(66, 9)])
    know(donor, ref)
    stages["het"]["uncalled"] = [ref[:66 + K], plain[:50]]
    # two texts of the graph that end alike: the first k-mer of the common part has two predecessors, no k-mer has two successors
    x, y, tail = fc.rand_seq(rng, 60), fc.rand_seq(rng, 60), fc.rand_seq(rng, 60)
    y = y[:-1] + _other(x[-1])
    know(x + tail, y + tail)
    stages["het"]["unseen"] = [x + tail]

    # isolated SNPs: one substitution per sequence, a gap of k positions each
    stages["snp"]["calls"] = []
    for at in (40, 60, 75):
        text = fc.rand_seq(rng, 120)
        know(text)
        stages["snp"]["calls"].append(text[:at] + _other(text[at]) + text[at + 1:])
    # ... and a surplus nucleotide: a gap of k positions as well, which no substitution closes
    text = fc.rand_seq(rng, 120)
    know(text)
    stages["snp"]["uncalled"] = [text[:60] + _other(text[60]) + text[60:], plain[:40]]
    # close SNPs: two substitutions 7 and 9 apart, gaps of k + 7 and k + 9 positions with two calls each
    stages["msnp"]["calls"] = []
    for at, d in ((50, 7), (70, 9)):
        text = fc.rand_seq(rng, 130)
        know(text)
        stages["msnp"]["calls"].append(text[:at] + _other(text[at]) + text[at + 1:at + d] + _other(text[at + d]) + text[at + d + 1:])
    # ... and a stretch of 25 nt replaced: a gap of 25 + k - 1 positions whose first step finds no alternative that holds snp_min_val windows
    text = fc.rand_seq(rng, 130)
    know(text)
    stages["msnp"]["uncalled"] = [text[:50] + "".join(_other(ch, 2) for ch in text[50:75]) + text[75:], "ACGT"]
    # ... and one of 250 nt: the gap has more than 254 positions
    text = fc.rand_seq(rng, 310)
    know(text)
    unjudged = [text[:30] + "".join(_other(ch, 2) for ch in text[30:280]) + text[280:]]

    # the shared input: an insertion site, a deletion, a heterozygous site; an isolated substitution and two substitutions 7 apart
    text = fc.rand_seq(rng, 170)
    know(text)
    for at in (40, 120, 127):
        text = text[:at] + _other(text[at]) + text[at + 1:]
    every = [stages["homo"]["calls"][0], stages["del"]["calls"][0], stages["het"]["calls"][0], text]
    return solid, stages, unjudged, every


SOLID, STAGES, UNJUDGED, ALL_LAYERS = _build()
