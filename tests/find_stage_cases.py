"""The smallest inputs that take every exit of the three `find` runs (homozygous insertions, homozygous deletions, heterozygous insertions), which
share one skeleton on the device (FindStage in csrc/mtg_gpu_misc.hip): k = 13, at most four sequences of at most 200 nt, one graph for all.

STAGES[layer][stage] = the sequences.  The stages, in the order of the run's exits:
  none        no sequence at all
  short       only sequences shorter than k: no position, no gap, no candidate
  in_graph    a sequence that lies wholly in the graph
  unseen      something the layer's first pass looks at, nothing of it a candidate -- homo: a gap longer than k - 1; del: gaps shorter than
              k - max_repeat; het: a position of in-degree 2 without a k-mer of out-degree 2 k positions before it
  uncalled    candidates, none of them called
  calls       at least three calls
ALL_LAYERS: sequences on which every layer makes a call.  tests/test_find_stages_cpu.py shows with the models alone that every input is what its
name says; tests/test_gpu_find_stages.py runs them on the device."""
import numpy as np

from tests import find_cases as fc
from tests import find_del_cases as fd
from tests import find_het_cases as fh

K, MAX_REPEAT, BRANCHING = 13, 5, 15
LAYERS = ("homo", "del", "het")
STAGE_NAMES = ("none", "short", "in_graph", "unseen", "uncalled", "calls")


def model(layer, solid, seqs):
    """(calls, statistics) of the layer's plain model"""
    if layer == "homo":
        return fc.find_homo(solid, K, seqs, MAX_REPEAT)
    if layer == "del":
        return fd.find_del(solid, K, seqs, MAX_REPEAT)
    return fh.find_het(solid, K, seqs, None, MAX_REPEAT, BRANCHING)


def stat_keys(layer):
    return {"homo": ("n_gaps", "n_candidates", "n_homo_clean", "n_homo_fuzzy", "n_small_clean", "n_small_fuzzy"), "del": fd.STAT_KEYS, "het": fh.STAT_KEYS}[layer]


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
    stages["homo"]["unseen"] = [snp]
    stages["del"]["uncalled"] = [snp, "ACGT"]
    # two texts of the graph one behind the other: a gap of k - 1 between a k-mer without a successor and one without a predecessor
    a, b = fc.rand_seq(rng, 70), fc.rand_seq(rng, 70)
    know(a, b)
    stages["homo"]["uncalled"] = [a + b, plain[:40]]
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

    every = [stages["homo"]["calls"][0], stages["del"]["calls"][0], stages["het"]["calls"][0], snp]
    return solid, stages, every


SOLID, STAGES, ALL_LAYERS = _build()
