"""dev tool: what AoADetection_Eng(train_refiner=True) costs.  The AoA SCST step and XE step through the Engine at bench.py's model
size (B = 64, 36 regions, Hd = E = 1024), option off and on, three alternating rounds in ONE process: median wall time per step,
the SCST step's per-phase GPU times, and the device memory each leg's first step allocates.  One JSON line at the end.

  python tools/perf_aoa_refiner_train.py [--steps 10] [--warmup 3] [--only on|off]     (--only on: the leg to put under a kernel trace)
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
from simpleimagecaptionzoo_amd.aoa import make_aoa_rng  # noqa: E402
from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, init_optimizer  # noqa: E402
from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references  # noqa: E402
from simpleimagecaptionzoo_amd.vocab import synthetic_vocab  # noqa: E402


class _Crit:
    smoothing = 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("on", "off"), default=None)
    a = ap.parse_args()
    B, V, L = 64, bench.V, 18
    vocab = synthetic_vocab(V)
    words = [vocab.ix2word[i] for i in range(V)]
    df = document_frequency(synthetic_references(2000, words, seed=0))
    batches = bench.make_batches(2, B, words, "cuda:0", 0)
    g = torch.Generator().manual_seed(3)
    lengths = sorted((int(x) for x in torch.randint(8, L, (B,), generator=g)), reverse=True)
    caps = torch.randint(4, V, (B, L + 1), generator=g)
    caps[:, 0] = 1
    xe_batches = [(b[0], b[1], caps, lengths, b[3]) for b in batches]
    legs = {}
    for on in ((False, True) if a.only is None else (a.only == "on",)):
        free0 = torch.cuda.mem_get_info()[0]
        eng = AoADetection_Eng({"model_type": "AoADetection", "embed_dim": 1024, "hidden_dim": 1024}, "SYN", vocab, data_dir="/tmp/",
                               use_bu="fixed", device="cuda:0", cider_df=df, max_batch=B, train_refiner=on)
        opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
        legs[on] = {"eng": eng, "opt": opt, "scst": [], "xe": []}
        eng.SCST_training_epoch(batches[:1], opt, None, tqdm_visible=False)
        eng.training_epoch(xe_batches[:1], opt, _Crit(), tqdm_visible=False)
        torch.cuda.synchronize()
        legs[on]["mem_mb"] = (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20

    def timed(fn, n):
        fn(a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for rnd in range(3):
        for on, leg in legs.items():
            eng, opt = leg["eng"], leg["opt"]
            leg["scst"].append(timed(lambda n: eng.SCST_training_epoch([batches[i % 2] for i in range(n)], opt, None, tqdm_visible=False), a.steps))
            leg["xe"].append(timed(lambda n: eng.training_epoch([xe_batches[i % 2] for i in range(n)], opt, _Crit(), tqdm_visible=False), a.steps))
            print("round %d train_refiner=%-5s SCST %.2f ms  XE %.2f ms" % (rnd, on, leg["scst"][-1], leg["xe"][-1]), flush=True)
    out = {}
    for on, leg in legs.items():
        eng, opt = leg["eng"], leg["opt"]
        eng.phase_events = []
        eng.SCST_training_epoch([batches[i % 2] for i in range(a.steps)], opt, None, tqdm_visible=False)
        torch.cuda.synchronize()
        out["on" if on else "off"] = {"scst_ms_median": round(statistics.median(leg["scst"]), 3), "scst_ms": [round(x, 3) for x in leg["scst"]],
                                      "xe_ms_median": round(statistics.median(leg["xe"]), 3), "xe_ms": [round(x, 3) for x in leg["xe"]],
                                      "scst_phases_ms": {k: round(v, 3) for k, v in eng.phase_times(skip=2).items()},
                                      "device_mb_after_first_steps": round(leg["mem_mb"], 1)}
    print(json.dumps({"tool": "perf_aoa_refiner_train", "B": B, "steps": a.steps, "legs": out}))


if __name__ == "__main__":
    main()
