"""Beam search with options (include/icz.h: icz_beam_opts) against the plain search, same process: full-width BUTD (36 x 2048
features, H = E = A = 1024, V = 10102, sharpened random weights), beam 5 x 128 images, 20 steps, <end> suppressed so that every leg
runs all 20 steps.  Legs: off (icz_butd_beam_search), off through the options entry, block_ngram = 3, n_best = 5 + wu 0.9, and all
three together; they alternate over three rounds, median ms per search and per step.
usage: perf_beam_opts.py [searches per leg]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from simpleimagecaptionzoo_amd.butd import ButdHandle  # noqa: E402
from simpleimagecaptionzoo_amd.synth import random_butd_params  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
R, D, H, E, A, V = 36, 2048, 1024, 1024, 1024, 10102
B, K, STEPS = 128, 5, 20
params = random_butd_params(R, D, H, E, A, V, "cuda", seed=78)
params["predict.weight_g"].mul_(6.0)
params["predict.bias"][2] = -1e4
h = ButdHandle(R, D, H, E, A, V, B * K, 20)
h.bind(params)
torch.manual_seed(6)
feats = torch.relu(torch.randn(B, R, D, device="cuda"))

LEGS = [("off", None), ("off (opts entry)", dict()), ("block_ngram=3", dict(block_ngram=3)),
        ("n_best=5 + wu_0.9", dict(n_best=5, length_penalty="wu_0.9")),
        ("all", dict(n_best=5, length_penalty="wu_0.9", block_ngram=3))]


def run(opts):
    return h.beam_search(feats, K, STEPS) if opts is None else h.beam_search_opts(feats, K, STEPS, **opts)


def leg(opts):
    for _ in range(2):
        run(opts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = run(opts)
    torch.cuda.synchronize()
    assert int(out[1].max()) == STEPS + 1          # every leg ran all steps
    return (time.perf_counter() - t0) / n * 1e3


res = {name: [] for name, _ in LEGS}
for r in range(3):
    for name, opts in LEGS:
        ms = leg(opts)
        res[name].append(ms)
        print("round %d  %-20s %.3f ms / search  %.1f us / step" % (r, name, ms, ms / STEPS * 1e3), flush=True)
off = sorted(res["off"])[1]
summary = {name: {"ms_median": round(sorted(v)[1], 3), "ms": [round(x, 3) for x in v], "vs_off": round(sorted(v)[1] / off - 1, 4)}
           for name, v in res.items()}
print(json.dumps({"device": torch.cuda.get_device_name(0), "searches_per_leg": n, "images": B, "beam": K, "steps": STEPS,
                  "legs": summary}))
h.close()
