"""Rate of the sequence profile (k_profile + the run kernels) next to k_scan's exact mode, on bench_scan.py's input: every position of the
synthetic donor (all members).  Three alternating rounds of scan exact / profile with words / profile runs-only; the median of each, positions
per second, and the ratio to the scan.  Writes nothing: redirect the output."""
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
K = 31
npos = np.maximum(S.lens.astype(np.int64) - K + 1, 0)
pos_off = torch.from_numpy(np.concatenate([[0], np.cumsum(npos)[:-1]]).astype(np.int64)).to(dev)
bits = torch.zeros_like(w)
out = torch.zeros(int(npos.sum()) + 1, dtype=torch.int32, device=dev)
cap = 1 << 20
runs = torch.zeros(cap * 4, dtype=torch.int32, device=dev)
ptrs = (w.data_ptr(), wo.data_ptr(), ln.data_ptr(), S.nseq)


def scan():
    st = idx.scan_packed_device(*ptrs, bits.data_ptr(), exact=True)
    return st["n_kmers"], st["kernel_ms"]


def profile_words():
    n, st = idx.profile_packed_device(*ptrs, pos_off.data_ptr(), out.data_ptr(), runs.data_ptr(), cap)
    return st["n_positions"], st["kernel_ms"]


def profile_runs_only():
    n, st = idx.profile_packed_device(*ptrs, None, None, runs.data_ptr(), cap)
    return st["n_positions"], st["kernel_ms"]


legs = (("scan_exact", scan), ("profile_words", profile_words), ("profile_runs_only", profile_runs_only))
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
for name in ("profile_words", "profile_runs_only"):
    res[name]["ratio_to_scan_exact"] = round(res[name]["Gpositions_per_s"] / res["scan_exact"]["Gpositions_per_s"], 3)
print(json.dumps(res, indent=1))
