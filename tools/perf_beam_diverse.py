"""Diverse beam search (include/icz.h: icz_beam_diversity) against the plain options search, same process: full-width BUTD (36 x 2048
features, H = E = A = 1024, V = 10102, sharpened random weights), beam 6 x 128 images, 20 steps, <end> suppressed so that every leg
runs all 20 steps.  Legs: beam_search_opts at beam 6; diverse with G = 2, 3 and 6 at lambda = 0.5; G = 3 with n_best = 6, wu 0.9 and
block_ngram = 3.  They alternate over three rounds, median ms per search and per step.  Then one n_best = 6 search per leg gives the
mean number of distinct hypotheses per image and the mean number of distinct bigrams over an image's six hypotheses (near-duplicate
lists share most of theirs).
usage: perf_beam_diverse.py [searches per leg]"""
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
B, K, STEPS, LAM = 128, 6, 20, 0.5
params = random_butd_params(R, D, H, E, A, V, "cuda", seed=78)
params["predict.weight_g"].mul_(6.0)
params["predict.bias"][2] = -1e4
h = ButdHandle(R, D, H, E, A, V, B * K, 20)
h.bind(params)
torch.manual_seed(6)
feats = torch.relu(torch.randn(B, R, D, device="cuda"))

LEGS = [("beam 6 (opts)", dict()), ("G=2", dict(groups=2, diversity=LAM)), ("G=3", dict(groups=3, diversity=LAM)),
        ("G=6", dict(groups=6, diversity=LAM)),
        ("G=3 + n_best=6 wu_0.9 block3", dict(groups=3, diversity=LAM, n_best=6, length_penalty="wu_0.9", block_ngram=3))]


def run(opts):
    return h.beam_search_opts(feats, K, STEPS, **opts)


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


def distinct(opts):
    """(mean distinct hypotheses, mean distinct bigrams) per image over the full list of K"""
    seqs, lens, _ = run(dict(opts, n_best=K))
    seqs, lens = seqs.cpu(), lens.cpu()
    hyps = bigrams = 0
    for i in range(B):
        toks = [seqs[i, j, :int(lens[i, j])].long().tolist() for j in range(K)]
        hyps += len({tuple(t) for t in toks})
        bigrams += len({tuple(t[q:q + 2]) for t in toks for q in range(len(t) - 1)})
    return round(hyps / B, 3), round(bigrams / B, 2)


res = {name: [] for name, _ in LEGS}
for r in range(3):
    for name, opts in LEGS:
        ms = leg(opts)
        res[name].append(ms)
        print("round %d  %-30s %.3f ms / search  %.1f us / step" % (r, name, ms, ms / STEPS * 1e3), flush=True)
base = sorted(res["beam 6 (opts)"])[1]
summary = {}
for (name, opts), v in zip(LEGS, res.values()):
    hyps, bigrams = distinct(opts)
    summary[name] = {"ms_median": round(sorted(v)[1], 3), "ms": [round(x, 3) for x in v], "vs_beam6": round(sorted(v)[1] / base - 1, 4),
                     "distinct_hyps_per_image": hyps, "distinct_bigrams_per_image": bigrams}
    print("%-30s distinct hypotheses / image %.3f  distinct bigrams / image %.2f" % (name, hyps, bigrams))
print(json.dumps({"device": torch.cuda.get_device_name(0), "searches_per_leg": n, "images": B, "beam": K, "steps": STEPS,
                  "diversity": LAM, "legs": summary}))
h.close()
