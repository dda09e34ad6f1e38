"""Multi-sample SCST against the reference's step, same process: Engine.SCST_training_epoch at B = 64 images with samples_per_image
None (one sampled caption per image + greedy baseline) and 5 (five sampled captions per image, leave-one-out baseline), and at
B = 16 with 4; the multi-sample cases once on the grouped attention kernels (option group_att = 1) and once on the per-row kernels
(group_att = 0).  Legs alternate over three rounds; per leg: step ms (wall, synchronised) and sampled captions per second, plus the
GPU time of the phases (rollouts / reward / backward / adam) from the Engine's phase marks.
usage: perf_scst_n.py [steps per leg]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
eng, opt, vocab, words = bench.build_engine("cuda:0", 64)
eng.use_graphs = True
batches = {B: bench.make_batches(n + 3, B, words, "cuda:0", 0, id_base=100000 * B) for B in (64, 16)}
for bs in batches.values():
    for bt in bs:
        eng.scorer().preload(bt[2])
h = eng.model._handle()

LEGS = [("B64 greedy-baseline", 64, None, 1), ("B64 K5 grouped", 64, 5, 1), ("B64 K5 per-row", 64, 5, 0),
        ("B16 K4 grouped", 16, 4, 1), ("B16 K4 per-row", 16, 4, 0)]


def leg(B, K, group):
    h.set_option("group_att", group)
    bs = batches[B]
    eng.SCST_training_epoch(bs[:3], opt, None, tqdm_visible=False, samples_per_image=K)
    torch.cuda.synchronize()
    eng.phase_events = []
    t0 = time.perf_counter()
    eng.SCST_training_epoch(bs[3:], opt, None, tqdm_visible=False, samples_per_image=K)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    phases = eng.phase_times()
    eng.phase_events = None
    return ms, B * (K or 1) / ms * 1e3, phases


res = {name: [] for name, *_ in LEGS}
for r in range(3):
    for name, B, K, group in LEGS:
        ms, caps, ph = leg(B, K, group)
        res[name].append((ms, caps, ph))
        print("round %d  %-20s step %.3f ms  %8.0f sampled captions/s  %s" % (
            r, name, ms, caps, " ".join("%s %.3f" % kv for kv in ph.items())), flush=True)
h.set_option("group_att", 0)
summary = {}
for name, rows in res.items():
    ms = sorted(x[0] for x in rows)[1]
    summary[name] = {"step_ms_median": round(ms, 3), "step_ms": [round(x[0], 3) for x in rows],
                     "sampled_captions_per_s_median": round(sorted(x[1] for x in rows)[1], 1),
                     "phases_ms_last_round": {k: round(v, 3) for k, v in rows[-1][2].items()}}
print(json.dumps({"device": torch.cuda.get_device_name(0), "steps_per_leg": n, "legs": summary}))
