"""dev tool: AoA multi-sample rollout + backward against the route that exists without it, same process.  At bench.py's model size
(36 regions, D = 2048, Hd = E = 1024, 8 heads, bench.V words) and K = 5 samples per image at the largest image count the bench-sized
handle's rows allow (max_batch 64 x beam 5 = 320 rows: 64 images):
  leg "sample_n"  multisample.sample_n(h, feats [B, R, D], K) + sample_backward           (one refiner pass per image)
  leg "repeated"  h.sample(feats.repeat_interleave(K, 0)) + sample_backward               (one refiner pass per row)
each on a handle of its own over the same parameters, Philox randomness, graphs off and on (sample_n only: sample is not captured).
Legs alternate over three rounds; per leg the median wall time per step (synchronised), the GPU time of the two phases (events) and the
device memory the leg's first step allocates.  One JSON line at the end.

  python tools/perf_scst_n_aoa.py [--steps 10] [--warmup 3] [--train-refiner]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from simpleimagecaptionzoo_amd.aoa import AoADetection_Captioner, make_aoa_rng  # noqa: E402
from simpleimagecaptionzoo_amd.multisample import sample_n  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-refiner", action="store_true")
    a = ap.parse_args()
    K, T, R, D = 5, 20, 36, 2048
    torch.manual_seed(0)
    cap = AoADetection_Captioner(bench.V, 8, 1024, 1024, num_regions=R, enc_dim=D, max_batch=64, max_beam=5).cuda()
    with torch.no_grad():
        cap.decoder.predict.weight_g.mul_(6.0)
    named = {k: p.data for k, p in cap._named().items()}
    B = cap.max_rows // K
    feats = torch.relu(torch.randn(B, R, D, device="cuda"))
    feats_rep = feats.repeat_interleave(K, 0).contiguous()
    reward = torch.randn(B * K, 1, device="cuda").repeat(1, T).contiguous()

    def handle(graphs):
        h = cap._new_handle(cap.max_rows, T, torch.device("cuda:0"))
        h.bind(named)
        if a.train_refiner:
            h.set_option("train_refiner", 1)
        h.enable_graphs(graphs)
        return h

    legs = {}
    for name, graphs in (("sample_n", False), ("repeated", False), ("sample_n graphs", True)):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        h = handle(graphs)
        legs[name] = {"h": h, "grads": h.new_grads(), "ms": [], "roll": [], "back": [], "seed": 1}

        def step(leg=legs[name], repeated=name == "repeated"):
            h_ = leg["h"]
            leg["seed"] += 1
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            if repeated:
                h_.sample(feats_rep, T, make_aoa_rng(leg["seed"]))
            else:
                sample_n(h_, feats, K, T, make_aoa_rng(leg["seed"]))
            ev[1].record()
            h_.sample_backward(reward, leg["grads"])
            ev[2].record()
            return ev

        legs[name]["step"] = step
        step()
        torch.cuda.synchronize()
        legs[name]["mem_mb"] = (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20

    for rnd in range(3):
        for name, leg in legs.items():
            for _ in range(a.warmup):
                leg["step"]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evs = [leg["step"]() for _ in range(a.steps)]
            torch.cuda.synchronize()
            leg["ms"].append((time.perf_counter() - t0) / a.steps * 1e3)
            leg["roll"].append(statistics.median(e[0].elapsed_time(e[1]) for e in evs))
            leg["back"].append(statistics.median(e[1].elapsed_time(e[2]) for e in evs))
            print("round %d  %-16s step %.3f ms  rollout %.3f ms  backward %.3f ms" % (rnd, name, leg["ms"][-1], leg["roll"][-1], leg["back"][-1]),
                  flush=True)
    out = {name: {"step_ms_median": round(statistics.median(leg["ms"]), 3), "step_ms": [round(x, 3) for x in leg["ms"]],
                  "rollout_ms_median": round(statistics.median(leg["roll"]), 3), "backward_ms_median": round(statistics.median(leg["back"]), 3),
                  "sampled_captions_per_s_median": round(B * K / statistics.median(leg["ms"]) * 1e3, 1),
                  "device_mb_after_first_step": round(leg["mem_mb"], 1)} for name, leg in legs.items()}
    print(json.dumps({"tool": "perf_scst_n_aoa", "device": torch.cuda.get_device_name(0), "images": B, "K": K, "steps": a.steps,
                      "train_refiner": bool(a.train_refiner), "legs": out}))


if __name__ == "__main__":
    main()
