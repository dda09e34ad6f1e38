"""Word-level distillation at the benchmark width (R 36, D 2048, H = E = A 1024, V 10 102), B = 64 captions of 8 - 17 tokens, a BUTD
student under M = 1 and M = 3 BUTD teachers.  ms per step and captions/s of
  (a) the plain XE step, Engine.training_epoch, exactly tools/perf_xe.py's step (this change leaves its launches alone);
  (b) Engine.distill_training_epoch with M = 1 and with M = 3 teachers (alpha 0.5, temperature 2);
  (c) the teachers' share on its own: distill.teacher_logits, M evaluation-mode xe_forward calls with packed logits;
  (d) the loss kernel on its own (icz_distill_loss on the step's packed rows: distill_loss_dlogits_kernel + the one-workgroup sum of
      the per-row losses) against its byte floor, (M + 1) row reads + one row write at the nominal 8 TB/s, with the rows at stride
      V = 10 102 (not 16-byte aligned: the scalar path) and padded to 10 104 (the vector path); M = 0 is the same kernel at
      alpha = 0, which reads no teacher (the hard term alone).  200 back-to-back calls into preallocated outputs per round; the
      host's enqueue time per call is printed beside the device time (a leg is a device time only where it is the smaller).
Device events around synchronised work, two warm-up rounds, the legs alternated in one process, median of R rounds.
usage: perf_distill.py [R]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from simpleimagecaptionzoo_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from simpleimagecaptionzoo_amd.distill import _opts, teacher_logits  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
B, STEPS, HBM = 64, 4, 8.0e12


class Crit:
    smoothing = 0.1


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    student, opt, vocab, _ = bench.build_engine("cuda:0", B)
    teachers = [bench.build_engine("cuda:0", B)[0] for _ in range(3)]
    V = len(vocab)
    rs = np.random.RandomState(0)
    batches = []
    for i in range(2):                                         # tools/perf_xe.py's batches
        lens = sorted(rs.randint(9, 19, size=B).tolist(), reverse=True)
        caps = torch.zeros(B, max(lens), dtype=torch.int64)
        for b, n in enumerate(lens):
            caps[b, 0] = 1
            caps[b, 1:n - 1] = torch.from_numpy(rs.randint(4, V, size=n - 2))
            caps[b, n - 1] = 2
        batches.append((tuple(range(B)), None, caps, lens, {"bu_feats": torch.relu(torch.randn(B, 36, 2048, device="cuda"))}))
    data = [batches[i % 2] for i in range(STEPS)]
    ids, imgs, caps, lens, supp = batches[0]
    steps = [n - 1 for n in lens]
    N = sum(steps)
    for e in teachers:
        e.model.eval()
    feats = lambda M: [e._features(e.modify_visual_inputs(imgs, supp)) for e in teachers[:M]]
    handles = lambda M: [e.model._handle() for e in teachers[:M]]
    # the loss kernel's inputs: one step's packed rows, at stride V and padded to a 16-byte multiple
    rows = teacher_logits(handles(3), feats(3), caps, steps) + [torch.randn(N, V, device="cuda")]
    ldp = (V + 3) // 4 * 4
    padded = []
    for t in rows:
        p = torch.zeros(N, ldp, device="cuda")
        p[:, :V] = t
        padded.append(p[:, :V])
    targets = torch.randint(4, V, (N,), device="cuda")
    K, host_us = 200, {}

    def kernel_leg(name, src, ld, M):
        o, keep = _opts(src[:max(M, 1)], N, V, None, 0.5 if M else 0.0, 2.0, 0.1)
        out, out3 = torch.empty(N, ld, device="cuda"), torch.zeros(3, device="cuda")
        fn, st = lib().icz_distill_loss, stream_ptr()

        def run():
            t0 = time.perf_counter()
            for _ in range(K):
                check(fn(ptr(src[3]), src[3].stride(0), C.byref(o), ptr(targets), N, V, float(N), ptr(out), ld, ptr(out3), st))
            host_us[name] = (time.perf_counter() - t0) / K * 1e6
            return keep
        return run
    legs = [("(a) plain XE step", STEPS, lambda: student.training_epoch(data, opt, Crit(), tqdm_visible=False))]
    for M in (1, 3):
        legs.append(("(b) distill step, M = %d" % M, STEPS,
                     lambda M=M: student.distill_training_epoch(data, opt, Crit(), teachers[:M], tqdm_visible=False, alpha=0.5, temperature=2.0)))
        legs.append(("(c) teacher forwards, M = %d" % M, 1, lambda M=M: teacher_logits(handles(M), feats(M), caps, steps)))
    for name, src, ld in (("stride %d" % V, rows, V), ("stride %d" % ldp, padded, ldp)):
        for M in (0, 1, 3):
            leg = "(d) loss kernel, M = %d, %s" % (M, name)
            legs.append((leg, K, kernel_leg(leg, src, ld, M)))
    times = {name: [] for name, _, _ in legs}
    for rnd in range(R + 2):
        for name, per, fn in legs:
            ms, _ = timed(fn)
            if rnd >= 2:
                times[name].append(ms / per)
    print("BUTD student, B = %d captions, %d tokens in the step, V = %d; median of %d rounds after 2 warm-up rounds, legs alternated" % (B, N, V, R))
    med = {}
    for name, _, _ in legs:
        med[name] = ms = float(np.median(times[name]))
        tail = ""
        if name.startswith("(a)") or name.startswith("(b)"):
            tail = "  %7.0f captions/s" % (B / ms * 1e3)
        elif "loss kernel" in name:
            M = int(name.split("M = ")[1][0])
            floor = (M + 2) * N * V * 4 / HBM * 1e3
            tail = "  byte floor %.4f ms (%d row passes at 8 TB/s): %.2f of it, %.0f GB/s; host enqueue %.1f us per call" % (
                floor, M + 2, floor / ms, (M + 2) * N * V * 4 / ms / 1e6, host_us[name])
        print("%-44s %9.4f ms%s   (min %.4f, max %.4f)" % (name, ms, tail, min(times[name]), max(times[name])))
    for M in (1, 3):
        print("distill step, M = %d: %.2f x the plain XE step; the teachers' forwards are %.0f %% of the difference" % (
            M, med["(b) distill step, M = %d" % M] / med["(a) plain XE step"],
            100 * med["(c) teacher forwards, M = %d" % M] / (med["(b) distill step, M = %d" % M] - med["(a) plain XE step"])))


if __name__ == "__main__":
    main()
