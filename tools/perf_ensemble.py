"""Model ensembles (include/icz.h: icz_ensemble_*) against their members, same process, bench.py's model size: BUTD beam search
(beam 5, 64 images) and greedy (128 images) for one BUTD model, one AoA model, two BUTD models and BUTD + AoA.  Single models run
through their captioner, ensembles through CaptionEnsemble.  Legs alternate over three rounds; per leg: ms per batch (wall,
synchronised) and captions per second, median of the rounds.
usage: perf_ensemble.py [batches per leg]   (1 with --quick: one round, for a kernel-trace run)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from simpleimagecaptionzoo_amd.aoa import AoADetection_Captioner  # noqa: E402
from simpleimagecaptionzoo_amd.captioner import BUTDDetection_Captioner  # noqa: E402
from simpleimagecaptionzoo_amd.ensemble import CaptionEnsemble  # noqa: E402
from simpleimagecaptionzoo_amd.synth import random_butd_params  # noqa: E402

quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else (1 if quick else 5)
dev = "cuda:0"
R, D, H, E, A, V = bench.R, bench.D, bench.H, bench.E, bench.A, bench.V


def butd(seed):
    c = BUTDDetection_Captioner(A, E, H, V, device=dev, enc_dim=D, num_regions=R, max_batch=128, max_beam=5)
    c.decoder.load_state_dict(random_butd_params(R, D, H, E, A, V, dev, seed=seed))
    return c.to(dev).eval()


torch.manual_seed(0)
b1, b2 = butd(1234), butd(99)
aoa = AoADetection_Captioner(vocab_size=V, hidden_dim=H, embed_dim=E, device=dev, num_regions=R, enc_dim=D, max_batch=128).to(dev).eval()
feats = {B: torch.relu(torch.randn(B, R, D, device=dev)) for B in (64, 128)}
vis = {B: {"bu_feats": f, "bu_masks": None} for B, f in feats.items()}
ens = {"2xBUTD": CaptionEnsemble([b1, b2]), "BUTD+AoA": CaptionEnsemble([b1, aoa])}
members = {"2xBUTD": [b1, b2], "BUTD+AoA": [b1, aoa]}


def run(kind, what, B):
    v = vis[B]
    if what in ens:
        vl = [v] * len(members[what])
        return ens[what].beam_search_sampler(vl, 5) if kind == "beam" else ens[what].sampler(vl, 20)
    c = b1 if what == "BUTD" else aoa
    return c.beam_search_sampler(v, 5) if kind == "beam" else c.sampler(v, 20)


LEGS = [(kind, what, B) for kind, B in (("beam", 64), ("greedy", 128)) for what in ("BUTD", "AoA", "2xBUTD", "BUTD+AoA")]


def leg(kind, what, B):
    with torch.no_grad():
        run(kind, what, B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            run(kind, what, B)
        torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    return ms, B / ms * 1e3


res = {"%s %s B%d" % L: [] for L in LEGS}
for r in range(1 if quick else 3):
    for L in LEGS:
        ms, caps = leg(*L)
        res["%s %s B%d" % L].append((ms, caps))
        print("round %d  %-24s %8.2f ms  %8.0f captions/s" % (r, "%s %s B%d" % L, ms, caps), flush=True)
summary = {}
for name, rows in res.items():
    mid = len(rows) // 2
    summary[name] = {"ms_median": round(sorted(x[0] for x in rows)[mid], 3), "ms": [round(x[0], 3) for x in rows],
                     "captions_per_s_median": round(sorted(x[1] for x in rows)[mid], 1)}
print(json.dumps({"device": torch.cuda.get_device_name(0), "batches_per_leg": n, "legs": summary}))
