"""Rate of `find` for close homozygous SNPs with the reverse pass (mtg_index_find_msnp_rev_packed_device, passes 3: k_msnp_rev_judge in place of
k_msnp_judge, k_msnp_rev_emit, k_msnp_rev_gaps) next to the unchanged forward entry, by the method of bench_find_msnp.py, on two changes of
bench_find.py's input:
  idle  bench_find_msnp.py's own: nucleotides 8 and 21 of word 40 of every sequence substituted, one gap of k + 13 positions that the forward
        pass takes whole with two calls; the reverse pass has nothing to do;
  work  nucleotide 2 of word 40 and nucleotides 2 and 15 of word 41 substituted: substitutions at g0, g0 + k + 1 and g0 + k + 14, one gap of
        k + 45 = 76 positions.  The forward pass calls g0 with a count of k and stops one position before the second substitution
        (consumed 31); the reverse pass is asked (45 > k + 5), calls the third with a count of 13 and the second with k (consumed_rev 44); the
        k-mer in between holds no substitution and stays: the gap is partial, 75 of 76.  (Two substitutions k + 1 apart alone leave k + 1
        positions, which FindMultiSNPrev's own entry test, L - c > k + snp_min_val, refuses.)
Alternating rounds in one process of find_msnp and find_msnp_rev (passes 3) on each input; every round's kernel_ms, the median and the spread
(max - min) of each leg, and the difference of the medians to the find_msnp rounds on the same input.  Writes nothing: redirect the output."""
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
del w
idle = S.words.copy()
idle[:, 40] ^= np.uint64((1 << 16) | (1 << 42))   # nucleotides 8 and 21
work = S.words.copy()
work[:, 40] ^= np.uint64(1 << 4)                  # nucleotide 2
work[:, 41] ^= np.uint64((1 << 4) | (1 << 30))    # nucleotides 2 and 15
inputs = {"idle": torch.from_numpy(idle.view(np.int64)).to(dev), "work": torch.from_numpy(work.view(np.int64)).to(dev)}
del idle, work
cap = 1 << 21
calls = torch.zeros(cap * 7, dtype=torch.int32, device=dev)
gap_cap = 1 << 20
gaps = torch.zeros(gap_cap * 7, dtype=torch.int32, device=dev)
extra = {}


def leg(entry, which):
    name = "%s/%s" % (entry, which)
    d_w = inputs[which]

    def run():
        if entry == "find_msnp":
            n, ng, st = idx.find_msnp_packed_device(d_w.data_ptr(), wo.data_ptr(), ln.data_ptr(), S.nseq, 5, MIN_VAL, calls.data_ptr(), cap, gaps.data_ptr(), gap_cap)
        else:
            n, ng, st = idx.find_msnp_rev_packed_device(d_w.data_ptr(), wo.data_ptr(), ln.data_ptr(), S.nseq, 5, MIN_VAL, 3, calls.data_ptr(), cap, gaps.data_ptr(), gap_cap)
        extra[name] = dict(gaps=st["n_gaps"], candidates=st["n_candidates"], calls=n, full=st["n_full"], partial=st["n_partial"], long=st["n_long"], gap_records=ng)
        return st["n_positions"], st["kernel_ms"]
    return name, run


legs = [leg(e, i) for i in ("idle", "work") for e in ("find_msnp", "find_msnp_rev")]
for _, f in legs:
    f()  # warm-up
ms = {name: [] for name, _ in legs}
nk = {}
for r in range(rounds):
    for name, f in legs:
        n, t = f()
        nk[name] = n
        ms[name].append(t)
res = {"input": "SynthSet(nseq=%d, seed=1): every position of the donor, all members; idle: nucleotides 8 and 21 of word 40 substituted; work: nucleotide 2 of word 40 and "
                "nucleotides 2 and 15 of word 41" % nseq, "rounds": rounds, "snp_min_val": MIN_VAL, "passes": 3}
for name, _ in legs:
    med = statistics.median(ms[name])
    res[name] = {"positions": int(nk[name]), "kernel_ms": [round(x, 3) for x in ms[name]], "median_ms": round(med, 3), "spread_ms": round(max(ms[name]) - min(ms[name]), 3),
                 "Gpositions_per_s": round(nk[name] / med / 1e6, 3)}
    res[name].update(extra[name])
for which in ("idle", "work"):
    a, b = res["find_msnp/" + which], res["find_msnp_rev/" + which]
    b["ratio_to_find_msnp"] = round(b["Gpositions_per_s"] / a["Gpositions_per_s"], 3)
    b["median_minus_find_msnp_ms"] = round(b["median_ms"] - a["median_ms"], 3)
print(json.dumps(res, indent=1))
