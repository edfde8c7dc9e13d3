"""Rate of `find` for isolated homozygous SNPs (the planes and gaps of the gap observers, then the solo observer's k_gap_mark, k_snp_judge,
k_gap_emit) next to `find` for homozygous deletions, on bench_find.py's input with one change: in the scanned copy of every sequence
nucleotide 16 of word 40 is substituted, so that each sequence has one gap of exactly k positions with both anchors -- a candidate of the
solo observer, which calls it (every candidate is a call: the full judge is timed, the first alternative that holds is the graph's own
nucleotide) and of the deletion observer, which judges it and finds no deletion.  Alternating rounds of find_del / find_snp; every round's
kernel_ms, the median and the spread (max - min) of each, positions per second, candidates per second and the ratio.  Writes nothing:
redirect the output."""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import mindthegap_amd as mtg
from mindthegap_amd.synth import SynthSet

nseq = int(sys.argv[1]) if len(sys.argv) > 1 else 600000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
mtg.load_library()
dev = torch.device("cuda", 0)
torch.cuda.init()
S = SynthSet(nseq=nseq, n_sites=min(100000, nseq), seed=1)
w = torch.from_numpy(S.words.view(np.int64)).to(dev)
wo = torch.from_numpy(S.word_off.view(np.int64)).to(dev)
ln = torch.from_numpy(S.lens.view(np.int32)).to(dev)
idx = mtg.Index.from_packed_device(w.data_ptr(), wo.data_ptr(), ln.data_ptr(), S.nseq, S.total_kmers_upper_bound, 31, 3, 40)
changed = S.words.copy()
changed[:, 40] ^= np.uint64(1 << 32)  # nucleotide 16 of the word becomes another one
w2 = torch.from_numpy(changed.view(np.int64)).to(dev)
cap = 1 << 20
calls = torch.zeros(cap * 7, dtype=torch.int32, device=dev)
ptrs = (w2.data_ptr(), wo.data_ptr(), ln.data_ptr(), S.nseq)
extra = {"find_del": {}, "find_snp": {}}


def find_del():
    n, st = idx.find_del_packed_device(*ptrs, 5, calls.data_ptr(), cap)
    extra["find_del"].update(gaps=st["n_gaps"], candidates=st["n_candidates"], fallback=st["n_fallback"], calls=n)
    return st["n_positions"], st["kernel_ms"]


def find_snp():
    n, st = idx.find_snp_packed_device(*ptrs, 5, calls.data_ptr(), cap)
    extra["find_snp"].update(gaps=st["n_gaps"], candidates=st["n_candidates"], calls=n)
    return st["n_positions"], st["kernel_ms"]


legs = (("find_del", find_del), ("find_snp", find_snp))
for _, f in legs:
    f()  # warm-up
ms = {name: [] for name, _ in legs}
nk = {}
for r in range(rounds):
    for name, f in legs:
        n, t = f()
        nk[name] = n
        ms[name].append(t)
res = {"input": "SynthSet(nseq=%d, seed=1): every position of the donor, all members, one nucleotide of word 40 of every sequence substituted" % nseq, "rounds": rounds}
for name, _ in legs:
    med = statistics.median(ms[name])
    res[name] = {"positions": int(nk[name]), "kernel_ms": [round(x, 3) for x in ms[name]], "median_ms": round(med, 3), "spread_ms": round(max(ms[name]) - min(ms[name]), 3),
                 "Gpositions_per_s": round(nk[name] / med / 1e6, 3)}
    res[name].update(extra[name])
    res[name]["Mcandidates_per_s"] = round(res[name]["candidates"] / med / 1e3, 3)
res["find_snp"]["ratio_to_find_del"] = round(res["find_snp"]["Gpositions_per_s"] / res["find_del"]["Gpositions_per_s"], 3)
res["find_snp"]["median_minus_find_del_ms"] = round(res["find_snp"]["median_ms"] - res["find_del"]["median_ms"], 3)
print(json.dumps(res, indent=1))
