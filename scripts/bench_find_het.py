"""Rate of `find` for heterozygous insertions (k_profile<true>'s five planes, the candidate words, k_het_judge, the chains) next to `find` for
homozygous insertions, on bench_find.py's input: every position of the synthetic donor (all members), nothing repeated.  Alternating rounds
of find_homo / find_het; the median of each, positions per second and the ratio.  Writes nothing: redirect the output."""
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
cap = 1 << 20
calls = torch.zeros(cap * 7, dtype=torch.int32, device=dev)
ptrs = (w.data_ptr(), wo.data_ptr(), ln.data_ptr(), S.nseq)
extra = {"find_homo": {}, "find_het": {}}


def find_homo():
    n, st = idx.find_homo_packed_device(*ptrs, 5, calls.data_ptr(), cap)
    extra["find_homo"].update(gaps=st["n_gaps"], candidates=st["n_candidates"], calls=n)
    return st["n_positions"], st["kernel_ms"]


def find_het():
    n, st = idx.find_het_packed_device(*ptrs, None, 5, 15, calls.data_ptr(), cap)
    extra["find_het"].update(candidates=st["n_candidates"], raw_sites=st["n_raw_sites"], filtered=st["n_filtered"], suppressed=st["n_suppressed"], calls=n)
    return st["n_positions"], st["kernel_ms"]


legs = (("find_homo", find_homo), ("find_het", find_het))
for _, f in legs:
    f()  # warm-up
ms = {name: [] for name, _ in legs}
nk = {}
for r in range(rounds):
    for name, f in legs:
        n, t = f()
        nk[name] = n
        ms[name].append(t)
res = {"input": "SynthSet(nseq=%d, seed=1): every position of the donor, all members" % nseq, "rounds": rounds}
for name, _ in legs:
    med = statistics.median(ms[name])
    res[name] = {"positions": int(nk[name]), "kernel_ms": [round(x, 3) for x in ms[name]], "median_ms": round(med, 3), "Gpositions_per_s": round(nk[name] / med / 1e6, 3)}
    res[name].update(extra[name])
res["find_het"]["ratio_to_find_homo"] = round(res["find_het"]["Gpositions_per_s"] / res["find_homo"]["Gpositions_per_s"], 3)
print(json.dumps(res, indent=1))
