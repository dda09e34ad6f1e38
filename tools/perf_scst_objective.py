"""What the SCST objectives (include/icz.h "SCST objectives", csrc/scst_objective.hip) cost at the benchmark width: V 10 102 (row
stride 10 112), 64 images x K 5 samples, T 20 -- 6 400 stored rows of 40 KB.  Four variants of the rollout's loss head:
  (p) the parent's: reinforce_loss_kernel + reinforce_dlogits_kernel (icz_test_reinforce / sample_backward);
  (0) kind 0, entropy_weight 0 through the new entry: the same kernels, must agree with (p) within the run-to-run spread;
  (e) kind 0, entropy_weight 0.01: scst_entropy_dlogits_kernel in the place of reinforce_dlogits_kernel (the row is read twice);
  (r) risk, entropy_weight 0.01: scst_risk_kernel + scst_risk_sum_kernel in front of it.
Measured twice: the loss head alone on given logits (every row live: the most bytes the head can move; the logits are restored from
a copy outside the timed region, the head overwrites them), and the whole backward pass of a BUTD handle (H = E = A 1024, graphs on,
as the Engine runs it) behind sample_n.  Device events around synchronised work, two warm-up rounds, the variants alternated in one
process (the whole backward: on a stream of its own, the order rotated every round), the median of R rounds; the box's own stream rate (icz_prof_stream_rate) beside them.
usage: perf_scst_objective.py [R]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from simpleimagecaptionzoo_amd._lib import check, lib  # noqa: E402
from simpleimagecaptionzoo_amd.captioner import BUTDDetection_Captioner  # noqa: E402
from simpleimagecaptionzoo_amd.scst_objective import make_objective, objective_loss, sample_backward_objective  # noqa: E402
from simpleimagecaptionzoo_amd.token_choice import entry_reinforce  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 12
N_IMG, K, T, V, LDL = 64, 5, 20, 10102, 10112
ROWS = N_IMG * K
B_ENT = 0.01


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stream_rate():
    buf = torch.empty(1 << 28, dtype=torch.float32, device="cuda")          # 1 GiB: four times the Infinity Cache
    gbs, best = C.c_double(), 0.0
    for _ in range(3):
        check(lib().icz_prof_stream_rate(C.c_void_p(buf.data_ptr()), C.c_size_t(buf.numel() * 4), 10,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(gbs)))
        best = max(best, gbs.value)
    return best


def report(title, legs, times, bytes_of=None, rate=None):
    print(title)
    for name, _ in legs:
        ms = float(np.median(times[name]))
        line = "  %-40s %8.3f ms   (min %.3f, max %.3f)" % (name, ms, min(times[name]), max(times[name]))
        if bytes_of:
            gb = bytes_of[name] / 1e9
            line += "   %6.3f GB moved  %7.0f GB/s" % (gb, gb / ms * 1e3)
            if rate:
                line += "  %4.0f %% of the stream rate" % (100.0 * gb / ms * 1e3 / rate)
        print(line)


def head_alone(rate):
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    pristine = torch.randn(T * ROWS, LDL, device="cuda", generator=g) * 2.0
    lse = torch.logsumexp(pristine[:, :V], 1).contiguous()
    draw = torch.randint(0, V, (T * ROWS,), device="cuda", dtype=torch.int32, generator=g)
    seq = torch.randint(3, V, (ROWS, T), device="cuda", generator=g)          # no row ends: every stored row is live
    logp = (pristine[torch.arange(T * ROWS, device="cuda"), draw.long()] - lse).view(T, ROWS).t().contiguous()
    reward = torch.randn(ROWS, 1, device="cuda", generator=g).expand(ROWS, T).contiguous()
    scores = torch.rand(ROWS, device="cuda", dtype=torch.float64, generator=g) * 3
    work = torch.empty_like(pristine)
    coef, loss, ms = torch.empty(ROWS, T, device="cuda"), torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    objs = {"0": make_objective("reinforce", K, reward=reward), "e": make_objective("reinforce", K, 1.0, B_ENT, reward=reward),
            "r": make_objective("risk", K, 1.0, B_ENT, scores=scores)}
    legs = [("(p) parent: icz_test_reinforce", lambda: entry_reinforce(logp, seq, reward, ROWS, T, None, coef, loss, ms, work, V, LDL, draw, lse)),
            ("(0) kind 0, b = 0", lambda: objective_loss(objs["0"], logp, seq, work, V, draw, lse, want_entropy=False)),
            ("(e) kind 0, b = %g" % B_ENT, lambda: objective_loss(objs["e"], logp, seq, work, V, draw, lse, want_entropy=False)),
            ("(r) risk, b = %g" % B_ENT, lambda: objective_loss(objs["r"], logp, seq, work, V, draw, lse, want_entropy=False))]
    row_r, row_w = T * ROWS * V * 4, T * ROWS * LDL * 4
    bytes_of = {legs[0][0]: row_r + row_w, legs[1][0]: row_r + row_w, legs[2][0]: 2 * row_r + row_w, legs[3][0]: 2 * row_r + row_w}
    times = {name: [] for name, _ in legs}
    for rnd in range(R + 2):
        for name, fn in legs:
            work.copy_(pristine)
            t = timed(fn)
            if rnd >= 2:
                times[name].append(t)
    report("loss head alone, %d rows of %d logits (all live), median of %d rounds after 2 warm-up rounds, variants alternated; GB moved = "
           "row reads (pass 2 of the entropy kernel counted as a read) + the gradient write" % (T * ROWS, V, R), legs, times, bytes_of, rate)


def whole_backward():
    cap = BUTDDetection_Captioner(1024, 1024, 1024, V, max_batch=ROWS, max_beam=1).cuda()
    h = cap._handle()
    h.enable_graphs(True)
    feats = torch.rand(N_IMG, 36, 2048, device="cuda")
    grads = h.new_grads()
    from simpleimagecaptionzoo_amd.butd import make_rng
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    reward = torch.randn(ROWS, 1, device="cuda", generator=g).expand(ROWS, T).contiguous()
    scores = torch.rand(ROWS, device="cuda", dtype=torch.float64, generator=g) * 3
    objs = {"0": make_objective("reinforce", K, reward=reward), "e": make_objective("reinforce", K, 1.0, B_ENT, reward=reward),
            "r": make_objective("risk", K, 1.0, B_ENT, scores=scores)}
    legs = [("(p) parent: sample_backward", lambda: h.sample_backward(reward, grads)),
            ("(0) kind 0, b = 0", lambda: sample_backward_objective(h, objs["0"], grads)),
            ("(e) kind 0, b = %g" % B_ENT, lambda: sample_backward_objective(h, objs["e"], grads)),
            ("(r) risk, b = %g" % B_ENT, lambda: sample_backward_objective(h, objs["r"], grads))]
    times = {name: [] for name, _ in legs}
    by_pos = [[] for _ in legs]
    live = []
    # on a stream of its own, as the Engine runs its steps (eager launches on the null stream behind graph replays are slow on this
    # runtime); the order of the variants rotates from round to round, so that no variant owns a position
    with torch.cuda.stream(torch.cuda.Stream()):
        for rnd in range(R + 2):
            for pos in range(len(legs)):
                name, fn = legs[(pos + rnd) % len(legs)]
                seq, _ = h.sample_n(feats, K, T, make_rng(100 + rnd))        # the same rollout for the four variants of a round
                if not live:
                    live.append(float(((seq[:, :-1] > 0).sum() + ROWS).item()) / (ROWS * T))
                t = timed(fn)
                if rnd >= 2:
                    times[name].append(t)
                    by_pos[pos].append(t)
    report("whole backward pass, BUTD at H = E = A 1024, %d images x %d samples, %d steps, graphs on (share of live (row, step) pairs %.2f); "
           "the order rotates every round" % (N_IMG, K, T, live[0]), legs, times)
    print("  by position in the round (all variants): " + "  ".join("%.3f" % float(np.median(x)) for x in by_pos) + " ms")


def main():
    rate = stream_rate()
    print("stream rate of this box (icz_prof_stream_rate, 1 GiB, best of 3 x 10 launches): %.0f GB/s" % rate)
    head_alone(rate)
    whole_backward()


if __name__ == "__main__":
    main()
