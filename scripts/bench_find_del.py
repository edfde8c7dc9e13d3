"""Rate of `find` for homozygous deletions (the planes and gaps of find_homo, then the deletion observer's k_gap_mark, k_del_judge, k_gap_emit) next to `find` for
homozygous insertions, on bench_find.py's input with one change: in the scanned copy of every sequence the 32 nucleotides of word 40 are
replaced, so that each sequence has one gap of 62 positions with both anchors -- a candidate of the deletion observer (judged: no deletion,
the joined text is not in the graph) and, being longer than k - 1, none of the insertion observers.  Alternating rounds of find_homo /
find_del; the median of each, positions per second, candidates per second and the ratio.  Writes nothing: redirect the output."""
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
changed[:, 40] ^= np.uint64(0x5555555555555555)  # every nucleotide of the word becomes another one
w2 = torch.from_numpy(changed.view(np.int64)).to(dev)
cap = 1 << 20
calls = torch.zeros(cap * 7, dtype=torch.int32, device=dev)
ptrs = (w2.data_ptr(), wo.data_ptr(), ln.data_ptr(), S.nseq)
extra = {"find_homo": {}, "find_del": {}}


def find_homo():
    n, st = idx.find_homo_packed_device(*ptrs, 5, calls.data_ptr(), cap)
    extra["find_homo"].update(gaps=st["n_gaps"], candidates=st["n_candidates"], calls=n)
    return st["n_positions"], st["kernel_ms"]


def find_del():
    n, st = idx.find_del_packed_device(*ptrs, 5, calls.data_ptr(), cap)
    extra["find_del"].update(gaps=st["n_gaps"], candidates=st["n_candidates"], fallback=st["n_fallback"], calls=n)
    return st["n_positions"], st["kernel_ms"]


legs = (("find_homo", find_homo), ("find_del", find_del))
for _, f in legs:
    f()  # warm-up
ms = {name: [] for name, _ in legs}
nk = {}
for r in range(rounds):
    for name, f in legs:
        n, t = f()
        nk[name] = n
        ms[name].append(t)
res = {"input": "SynthSet(nseq=%d, seed=1): every position of the donor, all members, word 40 of every sequence replaced" % nseq, "rounds": rounds}
for name, _ in legs:
    med = statistics.median(ms[name])
    res[name] = {"positions": int(nk[name]), "kernel_ms": [round(x, 3) for x in ms[name]], "median_ms": round(med, 3), "Gpositions_per_s": round(nk[name] / med / 1e6, 3)}
    res[name].update(extra[name])
res["find_del"]["Mcandidates_per_s"] = round(res["find_del"]["candidates"] / res["find_del"]["median_ms"] / 1e3, 3)
res["find_del"]["ratio_to_find_homo"] = round(res["find_del"]["Gpositions_per_s"] / res["find_homo"]["Gpositions_per_s"], 3)
print(json.dumps(res, indent=1))
