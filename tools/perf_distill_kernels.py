"""Per-dispatch durations of the loss kernels of tools/perf_distill.py from a kernel trace of it: distill_loss_dlogits_kernel on the
handle path (M = 1, 3) and alone (M = 0, 1, 3 at both row strides; the last of the tool's three rounds), xe_loss_dlogits_kernel of
the plain XE step and distill_sum_kernel.
usage: rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/perf_distill.py 1
       perf_distill_kernels.py OUT/<host>/<pid>_kernel_trace.csv"""
import csv
import statistics
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
d = [dur(r) for r in rows if "distill_loss_dlogits_kernel" in r["Kernel_Name"]]
x = [dur(r) for r in rows if "xe_loss_dlogits_kernel" in r["Kernel_Name"]]
s = [dur(r) for r in rows if "distill_sum_kernel" in r["Kernel_Name"]]
print("dispatches: distill_loss_dlogits_kernel %d, xe_loss_dlogits_kernel %d, distill_sum_kernel %d" % (len(d), len(x), len(s)))
print("xe_loss_dlogits_kernel (plain XE step, grid 64 x 17): median %.2f us (min %.2f, max %.2f)" % (statistics.median(x), min(x), max(x)))
print("distill_sum_kernel: median %.2f us" % statistics.median(s))
last = d[-1208:]
for name, part in (("handle path, M = 1 (grid 64 x 17, in place, ld 10112)", last[0:4]), ("handle path, M = 3", last[4:8])):
    print("%-60s median %.2f us (min %.2f, max %.2f)" % (name, statistics.median(part), min(part), max(part)))
alone = last[8:]
i = 0
for stride in (10102, 10104):
    for M in (0, 1, 3):
        part = alone[i * 200:(i + 1) * 200]
        i += 1
        med = statistics.median(part)
        by = (M + 2) * 795 * 10102 * 4
        print("kernel alone, M = %d, stride %d: median %.2f us (min %.2f, max %.2f) = %.0f GB/s over %d row passes, %.2f of 8 TB/s" % (
            M, stride, med, min(part), max(part), by / med / 1e3, M + 2, by / med / 1e3 / 8000))
