"""Evaluation-report timing: coco_eval.Bleu + coco_eval.Rouge compute_score on N synthetic images x 5 references (Zipf words,
references of 8-12 tokens, candidates of 8-16), host encoding and float arithmetic included.  Median of R runs after one warm-up.
usage: perf_coco_metrics.py [N] [R]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from simpleimagecaptionzoo_amd.coco_eval import Bleu, Rouge

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rng = np.random.RandomState(0)
words = ["w%d" % i for i in range(2000)]


def sent(lo, hi):
    z = np.minimum(rng.zipf(1.3, size=rng.randint(lo, hi + 1)), len(words)) - 1
    return " ".join(words[j] for j in z)


gts = {i: [sent(8, 12) for _ in range(5)] for i in range(N)}
res = {i: [sent(8, 16)] for i in range(N)}
bleu, rouge = Bleu(), Rouge()


def run():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b, _ = bleu.compute_score(gts, res)
    t1 = time.perf_counter()
    r, _ = rouge.compute_score(gts, res)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, b[3], r


run()
times = [run() for _ in range(R)]
tb = float(np.median([t[0] for t in times]))
tr = float(np.median([t[1] for t in times]))
print("%d images x 5 refs: Bleu %.1f ms + Rouge %.1f ms = %.1f ms (median of %d; Bleu_4 %.4f, ROUGE_L %.4f)"
      % (N, 1e3 * tb, 1e3 * tr, 1e3 * (tb + tr), R, times[-1][2], times[-1][3]))
