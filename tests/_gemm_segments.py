"""Case table of the GEMMs over several K segments (tests/test_cpu_gemm_segments.py checks its claims on the host,
tests/test_gpu_gemm_segments.py runs it).  No pytest in here.

A case names a product C[M, N] = sum_s A_s B_s, the kernel it is there for (a name from butd.GEMM_ROUTES) and what makes it worth
running: which split-K ranges hold a segment boundary strictly inside them -- the places where a kernel's segment walk has to step
from one operand pair to the next in the middle of its pipeline.  The claims were worked out by hand from the host logic of
csrc/gemm_f32.hip and csrc/gemm_resident_x3.hip; the CPU test recomputes them, so a retuned threshold turns a claim red instead of
quietly moving a case to another kernel.

Fields:  layout, M, N, Ks        the product
         splits                  the nsplit values to run (0 = the split of a decoder step)
         route                   the kernel, for every split run (x3 cases: per large-tile switch, see X3_ROUTES)
         bk                      depth of one pipeline stage / chunk of that kernel at this shape (split ranges are counted in it)
         picked                  the split that nsplit = 0 takes
         crossing                {split: ranges of that split which hold a segment boundary strictly inside}
         half_crossing           512-deep resident form only: {range: its four-stage halves (0, 1) that hold a boundary inside}
"""
import collections

Case = collections.namedtuple("Case", "name layout M N Ks splits route bk picked crossing half_crossing accumulate_only")


def _case(name, layout, M, N, Ks, splits, route, bk, picked, crossing, half_crossing=None, accumulate_only=False):
    return Case(name, layout, M, N, tuple(Ks), tuple(splits), route, bk, picked, crossing, half_crossing or {}, accumulate_only)


CASES = [
    # three one-stage segments, two of them partial (20 and 36 of 64)
    _case("nt_mt1_tail", "nt", 5, 70, (20, 64, 36), (0, 1, 2, 3), "nt_fp32_mt1", 64, 3, {1: (0,), 2: (0,), 3: ()}),
    # a segment shorter than one 16-deep k group between two longer ones (8 stages, so that four splits leave no empty one)
    _case("nt_mt2_tail", "nt", 20, 132, (100, 8, 320), (0, 1, 4), "nt_fp32_mt2", 64, 8, {1: (0,), 4: (1,), 8: ()}),
    # 64-deep stages, tail kernel
    _case("nt_mt4_64[33]", "nt", 33, 200, (64, 192, 100), (0, 1, 2), "nt_fp32_mt4", 64, 6, {1: (0,), 2: (0, 1), 6: ()}),
    _case("nt_mt4_64[64]", "nt", 64, 200, (64, 192, 100), (0, 1, 2), "nt_fp32_mt4", 64, 6, {1: (0,), 2: (0, 1), 6: ()}),
    # 128-deep stages, not the spread variant (64 < M < 1024)
    _case("nt_mt4_128", "nt", 100, 256, (128, 256, 128), (0, 1, 2), "nt_fp32_mt4", 128, 4, {1: (0,), 2: (0, 1), 4: ()}),
    # the spread-load variant: M <= 64 ...
    _case("nt_mt4_spread[40]", "nt", 40, 256, (256, 128, 128), (0, 1, 2), "nt_fp32_mt4", 128, 4, {1: (0,), 2: (1,), 4: ()}),
    _case("nt_mt4_spread[64]", "nt", 64, 256, (256, 128, 128), (0, 1, 2), "nt_fp32_mt4", 128, 4, {1: (0,), 2: (1,), 4: ()}),
    # ... and M >= 1024
    _case("nt_mt4_spread_tall", "nt", 1024, 64, (128, 128), (0, 1), "nt_fp32_mt4", 128, 2, {1: (0,), 2: ()}),
    # one 512-deep k range: finished output, bias fused; both half-plane loads cross a segment boundary (stages 3 | 2 | 3)
    _case("res_512_one", "nt", 40, 2052, (192, 128, 192), (0, 1), "resident_512deep", 64, 1, {1: (0,)}, {0: (0, 1)}),
    # two ranges; the boundary at stage 5 falls in the second half of range 0
    _case("res_512_two[64]", "nt", 64, 2048, (320, 192, 512), (0,), "resident_512deep", 64, 2, {2: (0,)}, {0: (1,), 1: ()}),
    _case("res_512_two[36]", "nt", 36, 2060, (320, 192, 512), (0,), "resident_512deep", 64, 2, {2: (0,)}, {0: (1,), 1: ()}),
    # three four-stage ranges; ranges 0 and 1 each hold a boundary (stages 3 | 2 | 7)
    _case("res_4stage[47]", "nt", 47, 2052, (192, 128, 448), (0,), "resident_4stage", 64, 3, {3: (0, 1)}),
    _case("res_4stage[64]", "nt", 64, 2048, (192, 128, 448), (0,), "resident_4stage", 64, 3, {3: (0, 1)}),
    _case("res_128row[65]", "nt", 65, 2052, (192, 128, 448), (0,), "resident_128row", 64, 3, {3: (0, 1)}),
    _case("res_128row[100]", "nt", 100, 2052, (192, 128, 448), (0,), "resident_128row", 64, 3, {3: (0, 1)}),
    _case("res_128row[128]", "nt", 128, 2052, (192, 128, 448), (0,), "resident_128row", 64, 3, {3: (0, 1)}),
    # three splits of four 128-deep chunks (5 | 3 | 4), the middle one spanning two segments
    _case("nt_x3_320", "nt", 320, 2048, (640, 384, 512), (0, 1), "x3", 128, 3, {1: (0,), 3: (1,)}),
    # ragged rows and columns, two splits of eight chunks (6 | 6 | 4)
    _case("nt_x3_129", "nt", 129, 4100, (768, 768, 512), (0, 1), "x3", 128, 2, {1: (0,), 2: (0, 1)}),
    # 128-deep stages
    _case("nn_128", "nn", 40, 256, (256, 128), (0, 1, 2), "nn_fp32", 128, 3, {1: (0,), 2: (), 3: ()}),
    # tail kernel
    _case("nn_tail", "nn", 20, 132, (100, 64), (0, 1, 3), "nn_fp32", 64, 3, {1: (0,), 3: ()}),
    # the NIC `w_ih +=` use: only with accumulate
    _case("tn_acc", "tn", 64, 52, (100,), (1,), "tn_fp32_64", 64, 2, {1: ()}, accumulate_only=True),
]
BY_NAME = {c.name: c for c in CASES}

# the many-row split-precision cases run under each large-tile switch (butd.gemm_set_big_cfg): the kernel each one means
X3_CFGS = (0, -1, 4)
X3_ROUTES = {0: ("x3_128tile",), -1: ("x3_128tile", "large_tile"), 4: ("large_tile",)}

# one case per route for the live-flag runs
LIVE_CASES = ("nt_mt1_tail", "nt_mt2_tail", "nt_mt4_64[33]", "nt_mt4_spread[64]", "res_512_one", "res_512_two[36]", "res_4stage[47]",
              "res_128row[100]", "nt_x3_320", "nn_128", "nn_tail", "tn_acc")

# the resident pair launch: (problem a, problem b, stages per k range, ranges of each)
PAIRS = [((40, 2048, (512, 512)), (40, 2052, (1024,)), 8, 2),
         ((64, 2048, (384, 384)), (33, 2052, (768,)), 4, 3)]
PAIR_MIXED = ((40, 2048, (512, 512)), (33, 2052, (768,)))        # 512-deep with four-stage: refused

FP32_ROUTES = ("nt_fp32_mt1", "nt_fp32_mt2", "nt_fp32_mt4", "nn_fp32")


def stages(Ks, bk):
    return [(k + bk - 1) // bk for k in Ks]


def split_ranges(Ks, bk, nsplit):
    """[lo, hi) in stages of depth bk for every split, the way gemm_f32 cuts them; None where a split would be empty."""
    tot = sum(stages(Ks, bk))
    if nsplit < 1 or nsplit > tot:
        return None
    cps = (tot + nsplit - 1) // nsplit
    if (tot + cps - 1) // cps != nsplit:
        return None
    return [(z * cps, min(tot, (z + 1) * cps)) for z in range(nsplit)]


def boundaries(Ks, bk):
    """Stage indices at which a new segment starts (the first segment's 0 left out)."""
    out, acc = [], 0
    for n in stages(Ks, bk)[:-1]:
        acc += n
        out.append(acc)
    return out


def crossing_ranges(Ks, bk, nsplit):
    """The splits whose stage range holds a segment boundary strictly inside."""
    bs = boundaries(Ks, bk)
    return tuple(z for z, (lo, hi) in enumerate(split_ranges(Ks, bk, nsplit)) if any(lo < b < hi for b in bs))


def half_crossing(Ks, nranges):
    """512-deep resident form: per eight-stage range, which of its two four-stage halves hold a boundary strictly inside."""
    bs = boundaries(Ks, 64)
    return {z: tuple(h for h in (0, 1) if any(8 * z + 4 * h < b < 8 * z + 4 * h + 4 for b in bs)) for z in range(nranges)}


# ---- the seeded sweep on the fp32-MFMA kernels: 40 cases, fixed here so that a failure names its case
SWEEP_SEED = 20240607


def _lcg(seed):
    s = seed & 0x7fffffff
    while True:
        s = (s * 1103515245 + 12345) & 0x7fffffff
        yield s >> 8


def _sweep(n, seed):
    r = _lcg(seed)
    pick = lambda lo, hi: lo + next(r) % (hi - lo + 1)
    out = []
    for i in range(n):
        layout = ("nt", "nn")[pick(0, 1)]
        nseg = pick(1, 4)
        M = pick(1, 130)
        N = 4 * pick(1, 75) if layout == "nn" else pick(1, 300)
        Ks = tuple(4 * pick(1, 65) for _ in range(nseg))
        nsplit = 1 if (M * N) % 4 else pick(0, 1)
        out.append(("sweep%02d" % i, layout, M, N, Ks, nsplit))
    return out


SWEEP = _sweep(40, SWEEP_SEED)
# pinned ends: a changed generator shows up on the host
SWEEP_FIRST = ("sweep00", "nn", 110, 256, (8, 168, 228, 52), 1)
SWEEP_LAST = ("sweep39", "nt", 53, 48, (212, 108, 104), 0)
