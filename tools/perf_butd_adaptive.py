"""BUTD over adaptive region sets at the benchmark width (D 2048, H = E = A 1024, V 10 102), 64 images: greedy decode (20 steps) and
one SCST step (rollouts + REINFORCE backward, Philox randomness, eager) for
  (a) a fixed 36-region batch -- the launches of the fixed-set kernels, the anchor;
  (b) regions = 64, counts drawn uniformly from 10..64, counts set (the counted kernels: loops bounded by each image's count);
  (c) the same padded tensor with no counts -- what a handle without icz_butd_set_regions does with such a batch (fixed-set kernels
      over all 64 rows, zero padding attended over);
  (d) regions = 100, counts 10..100, counts set.
One handle of capacity 100, one process, the legs alternated round by round, device events around synchronised work, two warm-up
rounds, median of R rounds with min and max.
usage: perf_butd_adaptive.py [R]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from simpleimagecaptionzoo_amd.butd import make_rng  # noqa: E402
from simpleimagecaptionzoo_amd.captioner import BUTDDetection_Captioner  # noqa: E402
from simpleimagecaptionzoo_amd.regions import RegionBatch  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
N_IMG, V, T, D = 64, 10102, 20, 2048


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def padded(regions, lo, rs):
    counts = [int(c) for c in rs.randint(lo, regions + 1, size=N_IMG)]
    f = torch.rand(N_IMG, regions, D)
    for i, c in enumerate(counts):
        f[i, c:] = 0
    return f.cuda(), counts


def main():
    torch.manual_seed(0)
    rs = np.random.RandomState(0)
    h = BUTDDetection_Captioner(1024, 1024, 1024, V, num_regions=100, max_batch=N_IMG, max_beam=1).cuda()._handle()
    fixed = torch.rand(N_IMG, 36, D, device="cuda")
    f64, c64 = padded(64, 10, rs)
    f100, c100 = padded(100, 10, rs)
    batches = (("(a) fixed 36", fixed), ("(b) regions 64, counts 10..64", RegionBatch(f64, c64)), ("(c) regions 64, no counts", f64),
               ("(d) regions 100, counts 10..100", RegionBatch(f100, c100)))
    reward = torch.randn(N_IMG, T, device="cuda")
    grads = h.new_grads()

    def scst(fb, seed):
        h.rollouts(fb, T, make_rng(seed))
        h.sample_backward(reward, grads)

    legs = []
    for name, fb in batches:
        legs.append(("greedy " + name, lambda fb=fb: h.greedy(fb, T)))
        legs.append(("SCST   " + name, lambda fb=fb: scst(fb, 11)))
    times = {name: [] for name, _ in legs}
    for rnd in range(R + 2):
        for name, fn in legs:
            ms = timed(fn)
            if rnd >= 2:
                times[name].append(ms)
    print("64 images, %d steps, benchmark width; mean count (b) %.1f of 64, (d) %.1f of 100; median of %d rounds after 2 warm-up rounds, "
          "legs alternated" % (T, float(np.mean(c64)), float(np.mean(c100)), R))
    med = {}
    for name, _ in legs:
        med[name] = float(np.median(times[name]))
        print("%-44s %8.3f ms   (min %.3f, max %.3f)" % (name, med[name], min(times[name]), max(times[name])))
    for kind in ("greedy", "SCST  "):
        b, c = med["%s (b) regions 64, counts 10..64" % kind], med["%s (c) regions 64, no counts" % kind]
        print("%s (b) / (c) = %.3f" % (kind, b / c))


if __name__ == "__main__":
    main()
