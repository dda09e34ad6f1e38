"""The cost of sampling without replacement (stochastic beam search) at the benchmark width (R 36, D 2048, H = E = A 1024, V 10 102),
BUTD, 128 images, 20 steps, 5 decoder rows per image in every leg:
  (a) stochastic_beam.sample_distinct with n = 5;
  (b) beam_search_opts with beam 5: the same 640 decoder rows through beam_rowtopk_reg_kernel<10> and beam_merge_kernel;
  (c) sample_decode with n = 5: 640 independent rows with replacement.
(a) - (b) is what sbs_rowtopk_kernel + sbs_merge_kernel cost over the beam step's select kernels: the noise (two logs and a quarter
Philox call per token) and three sweeps over split-K slabs in place of one pass over finished rows.  Random weights keep every row
alive to the step limit: all legs run all 20 steps.  It also reports the number that motivates the feature: the mean number of
DISTINCT captions per image among the 5 that sample_decode draws at T = 1 and T = 0.7 (sample_distinct: 5 by construction), on
weights sharpened as the tests' (embedding x 30, predict gain x 15) so that the distribution has a mode.
Device events around synchronised work, two warm-up rounds, the legs alternated in one process, median of R rounds; the result also
goes to the file named by the second argument.
usage: perf_sample_distinct.py [R] [log file]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from simpleimagecaptionzoo_amd import stochastic_beam  # noqa: E402
from simpleimagecaptionzoo_amd.butd import ButdHandle  # noqa: E402
from simpleimagecaptionzoo_amd.synth import random_butd_params  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
N_IMG, N, STEPS = 128, 5, 20
DIMS = (36, 2048, 1024, 1024, 1024, 10102)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def distinct_per_image(ids):
    ids = ids.cpu().numpy().reshape(N_IMG, N, -1)
    return float(np.mean([len({tuple(r.tolist()) for r in img}) for img in ids]))


def main():
    torch.manual_seed(0)
    feats = torch.rand(N_IMG, 36, 2048, device="cuda")
    h = ButdHandle(*DIMS, N_IMG * N, STEPS)
    params = random_butd_params(*DIMS, "cuda:0", seed=3)
    h.bind(params)
    legs = [("(a) sample_distinct, n = 5", lambda: stochastic_beam.sample_distinct(h, feats, N, STEPS, 1.0, 1)),
            ("(b) beam_search_opts, beam 5", lambda: h.beam_search_opts(feats, N, STEPS)),
            ("(c) sample_decode, n = 5", lambda: h.sample_decode(feats, N, STEPS, 1.0, 0, 1.0, 1))]
    times = {name: [] for name, _ in legs}
    for rnd in range(R + 2):
        for name, fn in legs:
            ms, _ = timed(fn)
            if rnd >= 2:
                times[name].append(ms)
    lines = ["sampling without replacement vs beam search vs sampling with replacement, BUTD at the benchmark width, %d images x %d rows, "
             "%d steps, median of %d rounds" % (N_IMG, N, STEPS, R)]
    med = {}
    for name, _ in legs:
        med[name] = float(np.median(times[name]))
        lines.append("%-34s %8.3f ms per call  (min %.3f, max %.3f)" % (name, med[name], min(times[name]), max(times[name])))
    a, b, c = (med[name] for name, _ in legs)
    lines.append("(a) - (b): %.3f ms per call = %.1f us per step; (a) / (b) = %.3f; (a) / (c) = %.3f" % (a - b, 1000.0 * (a - b) / STEPS, a / b, a / c))
    # the motivating number, on a distribution with a mode
    params["embed.0.weight"] *= 30
    params["predict.weight_g"] *= 15
    h.refresh()
    for T in (1.0, 0.7):
        with_repl = np.mean([distinct_per_image(h.sample_decode(feats, N, STEPS, T, 0, 1.0, seed)[0]) for seed in (1, 2, 3)])
        ids, lens, _, _, _ = stochastic_beam.sample_distinct(h, feats, N, STEPS, T, 1)
        lines.append("T = %.1f: distinct captions per image among %d: sample_decode %.2f, sample_distinct %.2f" % (T, N, with_repl, distinct_per_image(ids)))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
