"""What SCST on without-replacement samples (include/icz.h "SCST on without-replacement samples", csrc/swor_objective.hip) costs at the
benchmark width (R 36, D 2048, H = E = A 1024, V 10 102, row stride 10 112), 128 images per step:
  (d) Engine.SCST_distinct_training_epoch, n = 5 slots per image (4 samples + the threshold): stochastic beam search over 640 rows,
      CIDEr-D of 640 captions, a teacher-forced training-mode forward over 512 rows, xe_backward_swor, clamp + Adam;
  (m) Engine.SCST_multisample_training_epoch(samples_per_image=4) on the same batches in the same run: 512 sampled rollouts with the
      leave-one-out baseline, the step this one is an alternative to;
  (k) the head alone, one call of swor.swor_loss (icz_test_swor_objective: three kernels) on 512 rows x 20 steps of given logits,
      every row live and of full length -- the most bytes the head can move.  A CALL time: the host's check, the upload of perm and
      the scratch allocation are inside it; the kernels' own times come from a kernel trace of this leg alone (see usage), to be set
      against the byte floor printed here: one read and one write of every row at the box's own stream rate (icz_prof_stream_rate).
      The logits are restored from a copy outside the timed region: the head overwrites them.
The model has random weights: no caption ends, all 20 steps run in both steps.  Device events around synchronised work, two warm-up
rounds, the legs alternated in one process, the median of R rounds with min and max beside it.
usage: perf_swor.py [R [head]]      head: leg (k) alone, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/perf_swor.py 20 head)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from simpleimagecaptionzoo_amd._lib import check, lib  # noqa: E402
from simpleimagecaptionzoo_amd.swor import SworBatch, swor_loss  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
HEAD_ONLY = len(sys.argv) > 2 and sys.argv[2] == "head"
N_IMG, N, K, T, V, LDL, STEPS = 128, 5, 4, 20, 10102, 10112, 2


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


def head_leg():
    """the head alone: (restore, run)"""
    rows, m = N_IMG * (N - 1), N - 1
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    pristine = torch.randn(T * rows, LDL, device="cuda", generator=g) * 2.0
    work = torch.empty_like(pristine)
    caps = torch.randint(3, V, (rows, T + 1), generator=torch.Generator().manual_seed(1)).cuda()
    perm = torch.tensor([i * N + j for i in range(N_IMG) for j in range(m)], dtype=torch.int32)
    batch = SworBatch(caps, [T] * rows, perm, torch.arange(rows).view(N_IMG, m))
    phi = (-torch.rand(N_IMG * N) * 30.0 - 1.0).cuda()                      # on the device already, like the captions: the timed call uploads perm alone
    G = torch.sort(torch.randn(N_IMG, N, dtype=torch.float64) * 3.0 - 20.0, dim=1, descending=True)[0].reshape(-1).cuda()
    scores = (torch.rand(N_IMG * N, dtype=torch.float64) * 3.0).cuda()
    run = lambda: swor_loss(work, V, batch, phi, G, scores)
    return (lambda: work.copy_(pristine)), run


def main():
    rate = stream_rate()
    print("stream rate of this box (icz_prof_stream_rate, 1 GiB, best of 3 x 10 launches): %.0f GB/s" % rate)
    restore, head = head_leg()
    legs = [("(k) the head alone, per call", 1, restore, head)]
    eng = None
    if not HEAD_ONLY:
        eng, opt, _, words = bench.build_engine("cuda:0", N_IMG * N)
        batches = bench.make_batches(2, N_IMG, words, "cuda:0", 0)
        data = [batches[i % 2] for i in range(STEPS)]
        legs = [("(d) SCST_distinct step, n = %d" % N, STEPS, None,
                 lambda: eng.SCST_distinct_training_epoch(data, opt, None, tqdm_visible=False, samples_per_image=N)),
                ("(m) SCST_multisample step, K = %d" % K, STEPS, None,
                 lambda: eng.SCST_multisample_training_epoch(data, opt, None, tqdm_visible=False, samples_per_image=K))] + legs
    times = {name: [] for name, _, _, _ in legs}
    for rnd in range(R + 2):
        for name, per, before, fn in legs:
            if before:
                before()
            ms = timed(fn)
            if rnd >= 2:
                times[name].append(ms / per)
    print("BUTD at H = E = A 1024, V = %d, %d images per step; median of %d rounds after 2 warm-up rounds, legs alternated" % (V, N_IMG, R))
    med = {}
    for name, _, _, _ in legs:
        med[name] = ms = float(np.median(times[name]))
        tail = ""
        if name.startswith("(k)"):
            floor = (V + LDL) * 4 * T * N_IMG * (N - 1) / (rate * 1e9) * 1e3
            tail = "   host work included; the kernels' byte floor is %.3f ms (one read + one write of %.3f GB at the stream rate)" % (
                floor, (V + LDL) * 4 * T * N_IMG * (N - 1) / 1e9)
        else:
            tail = "   %7.0f images/s" % (N_IMG / ms * 1e3)
        print("  %-36s %9.3f ms%s   (min %.3f, max %.3f)" % (name, ms, tail, min(times[name]), max(times[name])))
    if eng is None:
        return
    d, m = med[legs[0][0]], med[legs[1][0]]
    print("SCST_distinct step: %.2f x the multi-sample step; per trained caption %.3f ms against %.3f ms" % (d / m, d / (N_IMG * (N - 1)), m / (N_IMG * K)))
    if eng.last_swor_stats:
        ess = eng.last_swor_stats[-1][:, 2]
        print("effective sample size of the last step's images: mean %.2f of %d samples (min %.2f)" % (float(ess.mean()), N - 1, float(ess.min())))


if __name__ == "__main__":
    main()
