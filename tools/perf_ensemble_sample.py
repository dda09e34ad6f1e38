"""The select stage of one step of an ensemble's sampling decode (include/icz.h: icz_ensemble_sample_decode), timed two ways in one
process on the same inputs: as two launches -- ensemble_logprob_kernel<false> writing the combined rows lp [rows, Vp] (icz_ensemble_logprob),
then the single-source sample_decode_kernel reading them (icz_sample_filter_draw) -- and as the one fused launch of the ensemble
instance (icz_ensemble_sample_filter_draw), which keeps the combined row in LDS.  M = 2 and 4 members' finished logits, 128 images x 2
samples = 256 rows, bench.py's vocabulary, filters off and temperature 0.8 / top_k 50 / top_p 0.9.  Per leg an event pair around
`iters` back-to-back calls on preallocated outputs; the routes alternate over the rounds; median microseconds per step.  The host
time of the same window is printed beside it: were it the larger, the figure would measure the enqueue, not the kernels.
usage: perf_ensemble_sample.py [iters per leg] [rounds]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from simpleimagecaptionzoo_amd._lib import SampleOpts, check, lib, stream_ptr  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 300
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = "cuda:0"
rows, V = 128 * 2, bench.V
Vp = (V + 63) & ~63
L = lib()
torch.manual_seed(0)
logits = [torch.randn(rows, Vp, device=dev) * 3.0 for _ in range(4)]
u = torch.rand(rows, device=dev)
lp = torch.zeros(rows, Vp, device=dev)
tok = torch.zeros(rows, dtype=torch.int64, device=dev)
logp = torch.zeros(rows, device=dev)
vp = lambda t: C.c_void_p(t.data_ptr())


def two_launches(M, opts):
    lg = (C.c_void_p * M)(*[t.data_ptr() for t in logits[:M]])
    ns, ld = (C.c_int32 * M)(*[1] * M), (C.c_int32 * M)(*[Vp] * M)
    st = stream_ptr()

    def run():
        check(L.icz_ensemble_logprob(M, lg, None, ns, ld, None, rows, V, vp(lp), Vp, None, st))
        check(L.icz_sample_filter_draw(vp(lp), None, 1, Vp, rows, V, C.byref(opts), vp(u), vp(tok), vp(logp), None, st))
    return run


def fused(M, opts):
    lg = (C.c_void_p * M)(*[t.data_ptr() for t in logits[:M]])
    ns, ld = (C.c_int32 * M)(*[1] * M), (C.c_int32 * M)(*[Vp] * M)
    st = stream_ptr()

    def run():
        check(L.icz_ensemble_sample_filter_draw(M, lg, None, ns, ld, None, rows, V, C.byref(opts), vp(u), vp(tok), vp(logp), None, st))
    return run


def leg(run):
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        run()
    b.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters, host * 1e6 / iters


OPTS = {"filters off": SampleOpts(1.0, 0, 1.0), "t=0.8 k=50 p=0.9": SampleOpts(0.8, 50, 0.9)}
legs = {}
for M in (2, 4):
    for oname, opts in OPTS.items():
        legs["M=%d %s | two launches" % (M, oname)] = two_launches(M, opts)
        legs["M=%d %s | fused" % (M, oname)] = fused(M, opts)
# the two routes draw the same tokens (the lse of a member is reduced in another order: the last bits of lp may differ)
same = {}
for M in (2, 4):
    for oname in OPTS:
        legs["M=%d %s | two launches" % (M, oname)]()
        a = tok.clone()
        legs["M=%d %s | fused" % (M, oname)]()
        torch.cuda.synchronize()
        same["M=%d %s" % (M, oname)] = int((a == tok).sum())
res = {k: [] for k in legs}
for r in range(rounds):
    for name, run in legs.items():
        us, host = leg(run)
        res[name].append((us, host))
        print("round %d  %-40s %8.2f us per step (host enqueue %6.2f us)" % (r, name, us, host), flush=True)
med = lambda v: round(sorted(v)[len(v) // 2], 2)
summary = {k: {"us_median": med([x[0] for x in v]), "us": [round(x[0], 2) for x in v], "host_us_median": med([x[1] for x in v])}
           for k, v in res.items()}
print(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows, "V": V, "iters_per_leg": iters, "rounds": rounds,
                  "rows_with_equal_tokens": same, "legs": summary}))
