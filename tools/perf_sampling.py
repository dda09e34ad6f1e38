"""Sampling decode (include/icz.h: icz_*_sample_decode) against greedy, same process, bench.py's model size, random weights,
through the BUTD captioner: greedy, sample_decode with the defaults, top_k = 50, top_p = 0.9 and both filters at temperature 0.8
on 128 images x 20 steps, and n = 5 samples per image on 64 images.  Legs alternate over three rounds; per leg: ms per decode
(wall, synchronised), median of the rounds.  The new kernel's microseconds per step come from one kernel-trace run of --quick.
usage: perf_sampling.py [decodes per leg]   (1 with --quick: one round, for a kernel-trace run)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from simpleimagecaptionzoo_amd.captioner import BUTDDetection_Captioner  # noqa: E402
from simpleimagecaptionzoo_amd.synth import random_butd_params  # noqa: E402

quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else (1 if quick else 10)
dev = "cuda:0"
R, D, H, E, A, V = bench.R, bench.D, bench.H, bench.E, bench.A, bench.V

torch.manual_seed(0)
cap = BUTDDetection_Captioner(A, E, H, V, device=dev, enc_dim=D, num_regions=R, max_batch=128, max_beam=5)
cap.decoder.load_state_dict(random_butd_params(R, D, H, E, A, V, dev, seed=1234))
cap = cap.to(dev).eval()
vis = {B: {"bu_feats": torch.relu(torch.randn(B, R, D, device=dev)), "bu_masks": None} for B in (64, 128)}

# name -> (images, samples per image, temperature, top_k, top_p); None = greedy
LEGS = [("greedy B128", (128, None)), ("sample defaults B128", (128, 1, 1.0, 0, 1.0)), ("top_k=50 B128", (128, 1, 1.0, 50, 1.0)),
        ("top_p=0.9 B128", (128, 1, 1.0, 0, 0.9)), ("t=0.8 k=50 p=0.9 B128", (128, 1, 0.8, 50, 0.9)), ("greedy B64", (64, None)),
        ("n=5 defaults B64", (64, 5, 1.0, 0, 1.0)), ("n=5 t=0.8 k=50 p=0.9 B64", (64, 5, 0.8, 50, 0.9))]
seed = [0]


def run(spec):
    B = spec[0]
    if spec[1] is None:
        return cap.sampler(vis[B], 20)
    seed[0] += 1
    return cap.sample_decode(vis[B], spec[1], 20, spec[2], spec[3], spec[4], rng=seed[0])


def leg(spec):
    with torch.no_grad():
        run(spec)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            run(spec)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


res = {name: [] for name, _ in LEGS}
for r in range(1 if quick else 3):
    for name, spec in LEGS:
        ms = leg(spec)
        res[name].append(ms)
        print("round %d  %-28s %8.3f ms" % (r, name, ms), flush=True)
summary = {name: {"ms_median": round(sorted(v)[len(v) // 2], 3), "ms": [round(x, 3) for x in v]} for name, v in res.items()}
print(json.dumps({"device": torch.cuda.get_device_name(0), "decodes_per_leg": n, "legs": summary}))
