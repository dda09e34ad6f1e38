"""XE training on five captions per image, two routes in one process at the benchmark width: 128 images x 5 captions of 8 .. 16 words,
features device-resident, one training step = forward + backward (training mode, Philox dropout, label smoothing 0.1).
  (a) packed:  xe_forward + xe_backward on the 640 length-sorted rows, the features repeated five times (the route without
               icz_butd_xe_forward_n);
  (b) grouped: xe_forward_n + xe_backward on the same captions, image-major, with option group_att 0 (per-row attention kernels through
               the row -> image table) and 1 (the grouped attention kernels).
The legs alternate over five rounds after a warm-up of every leg; per leg and round: step ms (host clock around `steps` synchronised
steps) and the forward / backward split from device events.  Medians over the rounds, the spread (min .. max) beside them, the bytes
of features each route stages per batch, and the two routes' losses on the same batch.
usage: perf_xe_grouped.py [steps per leg] [images] [captions per image]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from simpleimagecaptionzoo_amd.butd import ButdHandle, make_rng  # noqa: E402
from simpleimagecaptionzoo_amd.grouped import xe_forward_n  # noqa: E402
from simpleimagecaptionzoo_amd.synth import random_butd_params  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B = int(sys.argv[2]) if len(sys.argv) > 2 else 128
K = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ROUNDS = 5
DEV = "cuda:0"
if not torch.cuda.is_available():
    sys.exit("perf_xe_grouped.py measures on the GPU: no device found")
R, D, H, E, A, V = bench.R, bench.D, bench.H, bench.E, bench.A, bench.V
rows = B * K
h = ButdHandle(R, D, H, E, A, V, rows, 20, DEV)
h.bind(random_butd_params(R, D, H, E, A, V, DEV, seed=1234))
gen = torch.Generator(device="cpu")
gen.manual_seed(4321)
feats = torch.relu(torch.randn(B, R, D, generator=gen)).to(DEV)
rs = np.random.RandomState(7)
words = rs.randint(8, 17, size=rows)                       # 8 .. 16 words; the row holds <sta> + words + <end>
lens = [int(w) + 1 for w in words]                         # len - 1, as the entries take it
caps = torch.zeros(rows, max(lens) + 1, dtype=torch.int64)
for r, w in enumerate(words):
    caps[r, 0] = 1
    caps[r, 1:w + 1] = torch.from_numpy(rs.randint(4, V, size=w))
    caps[r, w + 1] = 2
caps = caps.to(DEV)
order = sorted(range(rows), key=lambda r: -lens[r])
feats_rep = feats.repeat_interleave(K, 0)[order].contiguous()
caps_sorted, lens_sorted = caps[order].contiguous(), [lens[r] for r in order]
grads = h.new_grads()
rng = make_rng(99)


def packed():
    h.xe_forward(feats_rep, caps_sorted, lens_sorted, rng, train=True)


def grouped():
    xe_forward_n(h, feats, caps, lens, K, rng, train=True)


LEGS = [("packed", packed, None), ("grouped per-row attention", grouped, 0), ("grouped group_att", grouped, 1)]


def leg(forward, group, n):
    if group is not None:
        h.set_option("group_att", group)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for e in ev:
        e[0].record()
        forward()
        e[1].record()
        loss = h.xe_backward(grads, 0.1)
        e[2].record()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    fwd = sum(e[0].elapsed_time(e[1]) for e in ev) / n
    bwd = sum(e[1].elapsed_time(e[2]) for e in ev) / n
    return ms, fwd, bwd, float(loss.item())


for name, f, group in LEGS:                                # every shape of the timed window, once
    leg(f, group, 3)
res = {name: [] for name, *_ in LEGS}
for r in range(ROUNDS):
    for name, f, group in LEGS:
        out = leg(f, group, steps)
        res[name].append(out)
        print("round %d  %-28s step %.3f ms  forward %.3f ms  backward %.3f ms  loss %.6f" % ((r, name) + out), flush=True)
h.set_option("group_att", 0)
med = lambda xs: sorted(xs)[len(xs) // 2]
summary = {}
for name, rr in res.items():
    summary[name] = {"step_ms_median": round(med([x[0] for x in rr]), 3), "step_ms_min_max": [round(min(x[0] for x in rr), 3), round(max(x[0] for x in rr), 3)],
                     "forward_ms_median": round(med([x[1] for x in rr]), 3), "backward_ms_median": round(med([x[2] for x in rr]), 3),
                     "loss": rr[-1][3]}
print(json.dumps({"device": torch.cuda.get_device_name(0), "images": B, "captions_per_image": K, "steps_per_leg": steps, "rounds": ROUNDS,
                  "decoder_steps": max(lens), "tokens": sum(lens), "row_steps_run_grouped": rows * max(lens),
                  "feature_bytes_staged": {"packed": rows * R * D * 4, "grouped": B * R * D * 4}, "legs": summary}))
