"""Rate of `find` for close homozygous SNPs (the planes and gaps of the gap observers, then the multi-SNP observer's k_gap_mark,
k_msnp_bound, k_msnp_judge, the listing of the slabs and k_msnp_emit) next to `find` for isolated homozygous SNPs, each on its own change of
bench_find.py's input: for find_snp nucleotide 16 of word 40 of every sequence is substituted (one gap of exactly k, bench_find_snp.py's
input), for find_msnp nucleotides 8 and 21 of that word, 13 apart: one gap of k + 13 positions with both anchors per sequence, a candidate
of the multi-SNP observer, which takes it whole with two calls (the chain's two steps: a best count of 13, then k).  Alternating rounds of
find_snp / find_msnp; every round's kernel_ms, the median and the spread (max - min) of each, positions per second, candidates per second,
the look-ups of the chain (per step 3 alternatives x cap windows go through the Bloom filter and, where it says yes, the table; cap = k at
both steps of this input) and the ratio.  Writes nothing: redirect the output."""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import mindthegap_amd as mtg
from mindthegap_amd.synth import SynthSet

nseq = int(sys.argv[1]) if len(sys.argv) > 1 else 600000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
K, MIN_VAL = 31, 5
mtg.load_library()
dev = torch.device("cuda", 0)
torch.cuda.init()
S = SynthSet(nseq=nseq, n_sites=min(100000, nseq), seed=1)
w = torch.from_numpy(S.words.view(np.int64)).to(dev)
wo = torch.from_numpy(S.word_off.view(np.int64)).to(dev)
ln = torch.from_numpy(S.lens.view(np.int32)).to(dev)
idx = mtg.Index.from_packed_device(w.data_ptr(), wo.data_ptr(), ln.data_ptr(), S.nseq, S.total_kmers_upper_bound, K, 3, 40)
one = S.words.copy()
one[:, 40] ^= np.uint64(1 << 32)                 # nucleotide 16 of the word becomes another one
two = S.words.copy()
two[:, 40] ^= np.uint64((1 << 16) | (1 << 42))   # nucleotides 8 and 21
w1 = torch.from_numpy(one.view(np.int64)).to(dev)
w2 = torch.from_numpy(two.view(np.int64)).to(dev)
del one, two
cap = 1 << 21
calls = torch.zeros(cap * 7, dtype=torch.int32, device=dev)
gap_cap = 1 << 20
gaps = torch.zeros(gap_cap * 5, dtype=torch.int32, device=dev)
extra = {"find_snp": {}, "find_msnp": {}}


def find_snp():
    n, st = idx.find_snp_packed_device(w1.data_ptr(), wo.data_ptr(), ln.data_ptr(), S.nseq, 5, calls.data_ptr(), cap)
    extra["find_snp"].update(gaps=st["n_gaps"], candidates=st["n_candidates"], calls=n)
    return st["n_positions"], st["kernel_ms"]


def find_msnp():
    n, ng, st = idx.find_msnp_packed_device(w2.data_ptr(), wo.data_ptr(), ln.data_ptr(), S.nseq, 5, MIN_VAL, calls.data_ptr(), cap, gaps.data_ptr(), gap_cap)
    extra["find_msnp"].update(gaps=st["n_gaps"], candidates=st["n_candidates"], calls=n, full=st["n_full"], partial=st["n_partial"], long=st["n_long"], gap_records=ng)
    return st["n_positions"], st["kernel_ms"]


legs = (("find_snp", find_snp), ("find_msnp", find_msnp))
for _, f in legs:
    f()  # warm-up
ms = {name: [] for name, _ in legs}
nk = {}
for r in range(rounds):
    for name, f in legs:
        n, t = f()
        nk[name] = n
        ms[name].append(t)
res = {"input": "SynthSet(nseq=%d, seed=1): every position of the donor, all members; find_snp: one nucleotide of word 40 of every sequence substituted, "
                "find_msnp: two, 13 apart" % nseq, "rounds": rounds, "snp_min_val": MIN_VAL}
for name, _ in legs:
    med = statistics.median(ms[name])
    res[name] = {"positions": int(nk[name]), "kernel_ms": [round(x, 3) for x in ms[name]], "median_ms": round(med, 3), "spread_ms": round(max(ms[name]) - min(ms[name]), 3),
                 "Gpositions_per_s": round(nk[name] / med / 1e6, 3)}
    res[name].update(extra[name])
    res[name]["Mcandidates_per_s"] = round(res[name]["candidates"] / med / 1e3, 3)
res["find_msnp"]["ratio_to_find_snp"] = round(res["find_msnp"]["Gpositions_per_s"] / res["find_snp"]["Gpositions_per_s"], 3)
res["find_msnp"]["median_minus_find_snp_ms"] = round(res["find_msnp"]["median_ms"] - res["find_snp"]["median_ms"], 3)
res["find_msnp"]["chain_lookups"] = int(res["find_msnp"]["calls"]) * 3 * K
print(json.dumps(res, indent=1))
