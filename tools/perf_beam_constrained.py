"""The cost of the constrained search's select kernels at the benchmark width (R 36, D 2048, H = E = A 1024, V 10 102), BUTD, 48
images, 20 steps:
  (a) constrained.beam_search with one constraint per image and beam 3: 2 states x 3 = 6 decoder rows per image;
  (b) beam_search_opts with beam 6: the same 6 decoder rows per image through today's row top-k and merge.
Both step 288 decoder rows, so (a) - (b) is what the constrained row top-k, beam_merge_states_kernel and beam_finalize_states_kernel cost
over beam_rowtopk_reg_kernel<10>, beam_merge_kernel and beam_finalize_kernel.  Random weights keep every beam alive to the step limit:
both run all 20 steps.  Device events around synchronised work, two warm-up rounds, the two alternated in one process, median of R
rounds; the result also goes to the file named by the second argument.
usage: perf_beam_constrained.py [R] [log file]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from simpleimagecaptionzoo_amd import constrained  # noqa: E402
from simpleimagecaptionzoo_amd.captioner import BUTDDetection_Captioner  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
N_IMG, V, STEPS = 48, 10102, 20


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    torch.manual_seed(0)
    rs = np.random.RandomState(0)
    feats = torch.rand(N_IMG, 36, 2048, device="cuda")
    h = BUTDDetection_Captioner(1024, 1024, 1024, V, max_batch=N_IMG, max_beam=6).cuda()._handle()
    cons = [[[int(w)]] for w in rs.randint(4, V, size=N_IMG)]
    legs = [("(a) constrained, 1 constraint, beam 3 (6 rows / image)", lambda: constrained.beam_search(h, feats, cons, 3, STEPS)),
            ("(b) beam_search_opts, beam 6 (6 rows / image)", lambda: h.beam_search_opts(feats, 6, STEPS))]
    times = {name: [] for name, _ in legs}
    steps = {}
    for rnd in range(R + 2):
        for name, fn in legs:
            ms, out = timed(fn)
            steps[name] = int(out[1].max().item()) - 1
            if rnd >= 2:
                times[name].append(ms)
    lines = ["constrained beam search vs plain beam search, BUTD at the benchmark width, %d images, %d steps, median of %d rounds"
             % (N_IMG, STEPS, R)]
    med = {}
    for name, _ in legs:
        med[name] = float(np.median(times[name]))
        lines.append("%-58s %8.3f ms per search  (min %.3f, max %.3f; longest caption %d steps)"
                     % (name, med[name], min(times[name]), max(times[name]), steps[name]))
    a, b = (med[name] for name, _ in legs)
    lines.append("difference (a) - (b): %.3f ms per search = %.1f us per step" % (a - b, 1000.0 * (a - b) / STEPS))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
