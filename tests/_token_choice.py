"""Case tables and float64 reference of the kernels that turn a row of logits into a token, a log-probability or a gradient
(csrc/token_kernels.h: argmax_part_kernel + embed_argmax_kernel, greedy_select_kernel, sample_select_kernel<false / true>,
ss_select_kernel, xe_loss_dlogits_kernel + sum_scale_kernel, reinforce_loss_kernel + reinforce_dlogits_kernel), each on given logits
(tests/test_cpu_token_choice.py holds every case to its stated purpose; tests/test_gpu_token_choice.py runs the tables through the
icz_test_* entries of include/icz.h).  Plain numpy, not collected by pytest.

A case is name -> shape -> purpose; the purpose is data the CPU test recomputes from the case alone.

No case needs an excuse: every comparison that decides a token is exact by construction or separated by MARGIN = 64 x a counted bound.

Finished logits.  ns > 1: the row is slab0 + slab1 + ... + bias in fp32, in that order, adds only: finish() does the same adds in
numpy.float32 and the bits must agree (logits_store).  "rand" rows draw every slab at random, so the order of the adds shows; every DESIGNED
row (ties, one-hot, constant, few-live) is made of multiples of 2^-8 below 1024, for which every partial sum is exact and the finished
row is the designed one bit for bit.

Argmax.  Device and reference compare the same bits, so the winner (largest value, lowest index among equals, 0 for a row without any
value above -inf) is exact for every row; the tie cases place equal bits where a kernel's rule could slip: in one thread's vector
sweep (v, v + 4096 and inside one group of four), in one thread of the scalar path (v, v + 1024), across lanes, waves and the parts of
the two-kernel form, across the end of the vector body.  (The lowest index wins, so a TIED loser never sits below the scalar tail
[V & ~3, V): the tail is asked with a tie that the body must win, with a tie inside the tail, and with a strict maximum at V & ~3 and
at V - 1.)

Multinomial draw (smallest v with cumsum(p)[v] > u sum(p), float64 sums).  Four row families keep it off the device's expf:
  (a) one-hot: one maximum, the rest at least 150 below: expf(<= -150) = 0, se = 1, lse = logf(1) = 0, p is one-hot in fp32 and every u
      in {0, 2^-24, 0.5, 1 - 2^-24} draws the maximum; logp = 0 and lse = the maximum exactly (bound 0); u = 1.0 (what a float64
      uniform just below 1 becomes in fp32) leaves no cumulative sum above the target and must give V - 1 through the clamp;
  (b) constant: every p is the same fp32 p0 and k p0 is exact in float64 for k <= 2^29, so the CDF is k p0 whatever p0 is and the total
      is V p0; the target fl64(u V p0) and (v + 1) p0 differ by at least 2^-38 relative (u V is a multiple of 2^-24 below 2^14) against
      the product's 2^-53 unless u V is an integer, where they are equal and the strict > moves on: the draw is floor(u V) for EVERY
      fp32 u, and u = fp32((j + 1/2) / V) draws j (asserted: |u V - (j + 1/2)| < 0.01);
  (c) few-live: 2..8 live tokens, the rest 150 below; u in the middle of a live token's CDF interval, at least MARGIN x cdf_bound from
      both edges in the float64 reference;
  (d) the scan's one-ulp gap: a small token 25 .. 27 below a big one in the next thread slice of the same wave, the rest 150 below.
      se = fl32(1 + 1e-11) = 1, lse = 0, p_big = 1 exactly, and the big token's lane holds inc = fl64(p_small + 1), on the 2^-52
      grid, so inc - loc is p_small ROUNDED to that grid while the previous lane's scan value is p_small itself.  The depth is the
      first fp32 whose exp lies 0.70 .. 0.80 of the way between two grid points (it rounds up with >= 51 fp32 ulps of p to spare,
      expf has 4), and u is 10 ulps above fp32(p_small): p_small <= u total < the grid point.  The float64 answer is the big token
      (cdf[small] < u); a kernel whose lower bound is inc - loc leaves the target to no lane and falls through to V - 1.  Exact given
      expf within E_EXP ulp, like (a) and (b); gap_holds() states the conditions and the CPU test asserts them.  Finished rows only.
Slice width of a thread is per = ceil(V / 1024), wave width 64 per: the maxima / targets sit at 0, V - 1, token 2 (<end>), and on both
sides of the first slice edge and the first wave edge.

Bounds (u = 2^-24, counted, never fitted; expf / logf ASSUMED within E_EXP = E_LOG = 4 ulp as in _beam_step.py), for a row of range
d = max - min and ls = log sum exp(x - max), n_add = additions on an element's path + 2:
  lp_bound   |logp - ref|     u (d + (d + |ls|))  [x - mx, (.) - ls]  +  (n_add + 2 E_EXP + d) u  [se, relative]  +  2 E_LOG u |ls|
  lse_bound  |lse - ref|      u |mx + ls|  +  (n_add + 2 E_EXP + d) u  +  2 E_LOG u |ls|
  cdf_bound  normalised CDF   2 (lp_bound + 2 E_EXP u)      (numerator and total each carry the relative error of p)
n_add: sample_select / ss_select ceil(V / 1024) + 6 + 16 + 2; xe_loss_dlogits ceil(V / 256) + 6 + 4 + 2.
  XE gradient        ((lp_bound + 2 E_EXP u) p + TINY + 3 u (p + true)) / N                  exp, subtraction, product, 1 / N
  XE row loss        (ceil(ldl / 256) + 6 + 4 + 2 + 2) u sum|term| + lp_bound + 2 E_LOG u max|log true|
  XE loss            ((ceil(T B / 256) + 6 + 4 + 2 + 1) u sum|row| + sum row bounds) / N
  REINFORCE coef     2 u |coef|;  loss (ceil(B T / 256) + 6 + 4 + 2 + 3) u sum|term| / denom;  mask sum exact
  REINFORCE gradient |c| (p (u |l - lse| + 2 E_EXP u) + TINY + u |1[v = d] - p|) + 3 u |g|    given l, lse, c in fp32
TINY = 2^-126: an expf below the smallest normal fp32 number may come out as a denormal or as zero (a saturated row), which no relative
bound covers.
"""
import collections
import math
import zlib

import numpy as np

import _philox

U = 2.0 ** -24
E_EXP = E_LOG = 4
MARGIN = 64.0
SENT = 0x7fffffff
END = 2
CANARY = -7
FILL = 7.0
PARTS = 8                          # ARGMAX_PARTS
SEL_THREADS = 1024
XE_MAX_T = 128
TINY = 2.0 ** -126                 # the smallest normal fp32 number: the absolute error of an expf that underflows
Q = 2.0 ** -8                      # grain of every designed value
US_ONEHOT = (0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24)


def seeded(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def pad_vocab(V):
    return (V + 63) & ~63


def per_thread(V):
    return -(-V // SEL_THREADS)


# ======================================================================================================================
# layouts: how the logits (and bias, logits_store) lie in memory.  off / bias_off / store_off: floats behind a 16-byte boundary.
Layout = collections.namedtuple("Layout", "name ldl_odd off stride_odd bias_off store_off")
LAYOUTS = {l.name: l for l in (
    Layout("aligned", 0, 0, 0, 0, 0),
    Layout("ldl_odd", 1, 0, 0, 0, 0),          # ldl % 4 != 0
    Layout("base_off", 0, 1, 0, 0, 0),         # the logits start 4 bytes behind a 16-byte boundary
    Layout("stride_odd", 0, 0, 1, 0, 0),       # slab_stride % 4 != 0
    Layout("bias_off", 0, 0, 0, 1, 0),         # a misaligned bias
    Layout("store_off", 0, 0, 0, 0, 1),        # a misaligned logits_store (sample_select only)
)}


def geometry(lay, V, rows, ns):
    ldl = pad_vocab(V) + (1 if lay.ldl_odd else 0)
    n = rows * ldl
    if ns == 1:
        return ldl, 0
    return ldl, n + ((1 - n) % 4 if lay.stride_odd else (-n) % 4)         # stride % 4 == 1, or the next multiple of 4


def takes_vector_loads(lay, V, rows, ns, bias, store=False):
    """the kernels' own switch (greedy_select_kernel; sample_select_kernel for ns > 1 with store = True)"""
    ldl, stride = geometry(lay, V, rows, ns)
    ok = ldl % 4 == 0 and stride % 4 == 0 and lay.off % 4 == 0 and (not bias or lay.bias_off % 4 == 0)
    return ok and (not store or lay.store_off % 4 == 0)


# ======================================================================================================================
# rows.  spec:
#   ("rand",)                        every slab random: the finished row is whatever the fp32 adds give
#   ("ties", positions[, above])     multiples of 2^-8 over [-8, 4], the positions all at 6.0 (`above`: one position at 6.0 + 2^-8)
#   ("zeros", plus, minus)           -1 everywhere, +0 at `plus`, -0 at `minus` (ns = 1, no bias only)
#   ("nan",) / ("ninf",)             every logit NaN / -inf
#   ("onehot", tok)                  1.0 at tok, the others over [-158, -150]
#   ("const",)                       every logit 0.5
#   ("live", positions)              live tokens 0, -0.5, -1, -0.25, ... at the positions, the others over [-158, -150]
#   ("gap", small, big, delta)       0 at `big`, -delta (any fp32, ns = 1 only) at `small`, the others over [-158, -150]
LIVE_VALUES = (0.0, -0.5, -1.0, -0.25, -1.5, -0.75, -2.0, -1.25)


def designed_row(V, spec, rs):
    kind = spec[0]
    if kind == "ties":
        x = rs.randint(-2048, 1025, size=V) * Q
        x[np.asarray(spec[1], dtype=np.int64)] = 6.0
        if len(spec) > 2:
            x[spec[2]] = 6.0 + Q
    elif kind == "zeros":
        x = np.full(V, -1.0)
        x[np.asarray(spec[1], dtype=np.int64)] = 0.0
        x[np.asarray(spec[2], dtype=np.int64)] = -0.0
    elif kind in ("nan", "ninf"):
        x = np.full(V, np.nan if kind == "nan" else -np.inf)
    elif kind == "onehot":
        x = -150.0 - rs.randint(0, 2049, size=V) * Q
        x[spec[1]] = 1.0
    elif kind == "const":
        x = np.full(V, 0.5)
    elif kind == "gap":
        x = -150.0 - rs.randint(0, 2049, size=V) * Q
        x[spec[1]], x[spec[2]] = -spec[3], 0.0
    elif kind == "live":
        x = -150.0 - rs.randint(0, 2049, size=V) * Q
        x[np.asarray(spec[1], dtype=np.int64)] = LIVE_VALUES[:len(spec[1])]
    else:
        raise ValueError(spec)
    return x.astype(np.float32)


def make_slabs(V, specs, ns, bias, rs):
    """(slabs [ns, rows, V] fp32, bias [V] fp32 or None) whose fp32 sum in slab order + bias is the designed row (random for "rand")"""
    rows = len(specs)
    slabs = np.zeros((ns, rows, V), dtype=np.float32)
    b = (rs.randint(-1024, 1025, size=V) * Q).astype(np.float32) if bias else None
    for r, spec in enumerate(specs):
        if spec[0] == "rand":
            slabs[:, r] = (3.0 * rs.standard_normal((ns, V))).astype(np.float32)
            continue
        x = designed_row(V, spec, rs)
        rest = (rs.randint(-1024, 1025, size=(ns - 1, V)) * Q).astype(np.float32)
        slabs[1:, r] = rest
        special = ~np.isfinite(x)
        with np.errstate(invalid="ignore"):
            first = x.astype(np.float64) - rest.astype(np.float64).sum(0) - (b.astype(np.float64) if bias else 0.0)
        slabs[0, r] = np.where(special, x, first).astype(np.float32)
        if spec[0] == "zeros":
            assert ns == 1 and not bias
            slabs[0, r] = x
    return slabs, b


def finish(slabs, bias):
    """slab0 + slab1 + ... + bias in numpy.float32, in that order"""
    with np.errstate(invalid="ignore"):
        x = slabs[0].copy()
        for z in range(1, slabs.shape[0]):
            x = (x + slabs[z]).astype(np.float32)
        if bias is not None:
            x = (x + bias[None, :]).astype(np.float32)
    return x


def place(slabs, lay, ldl, stride):
    """the slabs as one flat fp32 array: slab z at z * stride, row r at r * ldl, NaN in the pad columns and between the slabs"""
    ns, rows, V = slabs.shape
    flat = np.full((ns - 1) * stride + rows * ldl, np.nan, dtype=np.float32)
    for z in range(ns):
        for r in range(rows):
            flat[z * stride + r * ldl:z * stride + r * ldl + V] = slabs[z, r]
    return flat


def argmax_rule(x):
    """largest value, lowest index among equals; 0 for a row without any value above -inf"""
    with np.errstate(invalid="ignore"):
        ok = x > -np.inf
    if not ok.any():
        return 0
    m = x[ok].max()
    return int(np.flatnonzero(ok & (x == m))[0])


def embed_ref(table, ids, relu):
    e = table[np.asarray(ids, dtype=np.int64)]
    return np.maximum(e, np.float32(0)) if relu else e


def make_table(V, E, rs):
    """embedding rows with both signs (and row 0 not zero: a fall back to <pad> shows)"""
    return rs.standard_normal((V, E)).astype(np.float32)


# ======================================================================================================================
# greedy cases
Greedy = collections.namedtuple("Greedy", "name V ns bias layout E relu specs purpose")


def tie_positions(V, n):
    """n positions with the structure the kernels' tie rules are asked about, lowest first"""
    want = [5, 6, 5 + 1024, 5 + 4096, (V & ~3) - 1, V & ~3, V - 1, V // 2, 64, 65, 255, 256, 1023, 1024]
    pos = []
    for p in want:
        if 0 <= p < V and p not in pos:
            pos.append(p)
    have = set(pos[:n])
    for p in np.linspace(0, V - 1, n).astype(int).tolist() + list(range(V)):
        if len(have) == n:
            break
        have.add(p)
    assert len(have) == n, (V, n)
    return sorted(have)


def part_of(V, v):
    per = ((V + PARTS - 1) // PARTS + 3) & ~3
    return v // per


def _greedy_specs(V, rows, ns, bias, rs):
    """the standard row set of a greedy case, cycled to `rows` rows"""
    Vv = V & ~3
    base = [("rand",), ("onehot", 0), ("onehot", V - 1), ("onehot", min(END, V - 1)), ("nan",), ("ninf",), ("const",),
            ("onehot", Vv if Vv < V else V - 1), ("onehot", max(Vv - 1, 0))]
    for n in (2, 64, 65, 1024, 1025):
        if V >= n:
            base.append(("ties", tie_positions(V, n)))
    if V >= 8:
        base.append(("ties", [1, V - 1]))                                   # body against tail: the body wins
        base.append(("ties", [1, V // 2], V - 1))                           # a strict maximum at V - 1
        base.append(("ties", [V // 2, V - 1], 0))                           # a strict maximum at 0
        base.append(("ties", [0, V - 1]))                                   # first and last part of the two-kernel form
        if Vv < V:
            base.append(("ties", [0, V - 1], Vv))                           # a strict maximum on the first tail element
        if V - Vv >= 2:
            base.append(("ties", [Vv, V - 1]))                              # a tie inside the tail
    if ns == 1 and not bias and V >= 4:
        base.append(("zeros", [V - 1], [1]))                                # -0 in front of +0
        base.append(("zeros", [1], [V - 1]))
    return [base[i % len(base)] for i in range(rows if rows else len(base))]      # rows = None: each once


def _g(name, V, rows, ns=1, bias=False, layout="aligned", E=4, relu=1, purpose=()):
    specs = _greedy_specs(V, rows, ns, bias, None)
    return Greedy(name, V, ns, bias, layout, E, relu, specs, dict(purpose))


GREEDY_CASES = (
    [_g("V%d" % V, V, 33 if V >= 1023 else None, purpose={"V": V}) for V in (1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097)]
    + [_g("V8195_rows64", 8195, 64, E=1024, purpose={"rows": 64}),
       _g("V10239_ns4_bias", 10239, 33, ns=4, bias=True, E=1024, relu=0, purpose={"ns": 4}),
       _g("V4097_ns2_nobias", 4097, 33, ns=2, E=4100, purpose={"ns": 2, "E": 4100}),
       _g("V4097_ns1_bias", 4097, 33, ns=1, bias=True, purpose={"ns": 1, "bias": True}),
       _g("V1025_row1", 1025, 1, ns=2, bias=True, relu=0, purpose={"rows": 1}),
       _g("V5_parts", 5, None, purpose={"empty_parts": 6})]
    + [_g("V4097_ns2_%s" % lay, 4097, 33, ns=2, bias=True, layout=lay, purpose={"scalar": lay != "aligned", "twin": "V4097_ns2_aligned"})
       for lay in ("aligned", "ldl_odd", "base_off", "stride_odd", "bias_off")]
    + [_g("V8195_ns1_%s" % lay, 8195, 33, layout=lay, purpose={"scalar": lay != "aligned", "twin": "V8195_ns1_aligned"})
       for lay in ("aligned", "ldl_odd", "base_off")]
)
GREEDY_BY_NAME = {c.name: c for c in GREEDY_CASES}


def greedy_inputs(c):
    rs = seeded("greedy/" + (c.purpose.get("twin") or c.name))         # a layout's twin holds the same values
    slabs, bias = make_slabs(c.V, c.specs, c.ns, c.bias, rs)
    return {"slabs": slabs, "bias": bias, "table": make_table(c.V, c.E, rs)}


def greedy_routes(c):
    """the forms that take the case: 1 two kernels (finished rows, no bias), 2 one kernel, 0 the decoders' pick"""
    return (0, 1, 2) if c.ns == 1 and not c.bias else ((0, 2) if c.ns > 1 else (2,))


def greedy_ref(c, inp):
    x = finish(inp["slabs"], inp["bias"])
    ids = np.array([argmax_rule(r) for r in x], dtype=np.int64)
    return {"x": x, "ids": ids, "emb": embed_ref(inp["table"], ids, c.relu)}


def greedy_bookkeeping(ids, t, unf_in, n_prev):
    """(unfinished out, count) of greedy_select_kernel at step t: a row stays unfinished while it was (t == 0: every row is) and its token is
    not <end>; n_prev == 0 at t > 0: the dead step (None, None)"""
    if t > 0 and n_prev == 0:
        return None, None
    unf = (((unf_in != 0) | (t == 0)) & (ids != END)).astype(np.uint8)
    return unf, int(unf.sum())


# ======================================================================================================================
# bounds
def row_bounds(x, n_add):
    """(lp_bound, lse_bound, cdf_bound) of a finite row (module docstring); all 0 for a one-hot row"""
    x = np.asarray(x, dtype=np.float32)
    mx = float(x.max())
    if is_onehot(x):
        return 0.0, 0.0, 0.0
    d64 = x.astype(np.float64) - mx
    ls = math.log(np.exp(d64).sum())
    d = mx - float(x.min())
    se = (n_add + 2 * E_EXP + d) * U
    lp = U * (d + (d + abs(ls))) + se + 2 * E_LOG * U * abs(ls)
    lse = U * abs(mx + ls) + se + 2 * E_LOG * U * abs(ls)
    return lp, lse, 2 * (lp + 2 * E_EXP * U)


def is_onehot(x):
    mx = x.max()
    return int((x == mx).sum()) == 1 and (x.size == 1 or np.partition(x, -2)[-2] <= mx - 150.0)


def n_add_select(V):
    return per_thread(V) + 6 + 16 + 2


def n_add_xe(V):
    return -(-V // 256) + 6 + 4 + 2


def draw_ref(x, u, log, what):
    """(draw, logp, lse, lp_bound, lse_bound) of the float64 reference for one finished row and a uniform u (fp32); logs the distance of
    the target from both neighbouring CDF edges as a multiple of cdf_bound (inf for an exact row)"""
    x = np.asarray(x, dtype=np.float32)
    V = x.size
    mx = float(x.max())
    lpb, lseb, cdfb = row_bounds(x, n_add_select(V))
    if is_onehot(x):
        d = V - 1 if float(u) >= 1.0 else int(np.argmax(x))       # u = 1: no cumulative sum is above the total -- the last token
        log.append((what, math.inf))
        return d, float(x[d]) - mx, mx, 0.0, 0.0                  # x - mx is exact on the grain of the designed rows
    d64 = x.astype(np.float64) - mx
    ls = math.log(np.exp(d64).sum())
    g = gap_facts(x, u)
    if g is not None:                                             # family (d): exact given expf within E_EXP ulp
        assert gap_holds(g), g
        log.append((what, math.inf))
        return g["big"], -ls, mx + ls, lpb, lseb
    if (x == x[0]).all():
        d = min(int(math.floor(float(np.float32(u)) * V)), V - 1)      # the CDF is k p0 exactly: floor(u V) (u V is exact in float64)
        log.append((what, math.inf))
        return d, -ls, mx + ls, lpb, lseb
    cdf = np.cumsum(np.exp(d64 - ls))
    cdf /= cdf[-1]
    uu = float(np.float32(u))
    d = min(int(np.searchsorted(cdf, uu, side="right")), V - 1)
    live = np.flatnonzero(x > mx - 100.0)
    lo = cdf[d - 1] if d > 0 else 0.0
    gaps = [uu - lo] if lo > 0 else []
    if d != live[-1]:
        gaps.append(cdf[d] - uu)
    log.append((what, min(gaps) / cdfb if gaps else math.inf))
    return d, float(d64[d] - ls), mx + ls, lpb, lseb


# ======================================================================================================================
# family (d): the one-ulp gap of the scan (module docstring)
GAP_START = (25.0, 26.5)           # where the search for the small token's depth starts, per row
GAP_U_ULPS = 10                    # u sits this many fp32 ulps above fp32(exp(-delta))


def gap_delta(start):
    """the first fp32 delta >= start whose exp(-delta) lies 0.70 .. 0.80 of the way between two points of the 2^-52 grid"""
    d = np.float32(start)
    for _ in range(4096):
        cell = math.exp(-float(d)) * 2.0 ** 52
        if 0.70 <= cell - math.floor(cell) <= 0.80:
            return d
        d = np.nextafter(d, np.float32(np.inf))
    raise AssertionError(start)


def gap_u(delta):
    p32 = np.float32(math.exp(-float(delta)))
    return (p32.view(np.uint32) + np.uint32(GAP_U_ULPS)).view(np.float32)


def gap_positions(V):
    """(small, big) token pairs in adjacent thread slices of one wave: across a slice edge, and mid-slice in the second wave"""
    per = per_thread(V)
    pairs = [(3 * per - 1, 3 * per), (70 * per + per // 2, 71 * per + per - 1)]
    return [(a, b) for a, b in pairs if b < V - 1]


def gap_facts(x, u):
    """None unless the row is of family (d): two live tokens, the lower-index one 20 .. 40 below the other, the rest 150 below.  Else
    where exp(-delta) sits in its 2^-52 cell, and in fp32 ulps of p: how far u is above fp32(p) and below the rounded-up grid point."""
    x = np.asarray(x, dtype=np.float32)
    mx = x.max()
    live = np.flatnonzero(x > mx - np.float32(100.0))
    if len(live) != 2 or x[live[1]] != mx or not (20.0 <= float(mx) - float(x[live[0]]) <= 40.0):
        return None
    small, big = int(live[0]), int(live[1])
    delta = float(mx) - float(x[small])                            # exact: the device forms fp32(x - mx) without rounding
    p = math.exp(-delta)
    p32 = np.float32(p)
    ulp = float(np.spacing(p32))
    cell = p * 2.0 ** 52
    up = math.ceil(cell) * 2.0 ** -52                              # fl64(1 + p) - 1 when p rounds up
    per = per_thread(x.size)
    return {"small": small, "big": big, "delta": delta, "cell": cell - math.floor(cell), "grid_ulps": 2.0 ** -52 / ulp,
            "u_above": (float(np.float32(u)) - float(p32)) / ulp, "u_below": (up - float(np.float32(u)) * (1.0 + 2.0 ** -30)) / ulp,
            "exact_sub": float(np.float32(x[small] - mx)) == -delta, "lanes": (small // per, big // per), "p": p,
            "dead_below": float(mx) - float(np.partition(x, -3)[-3]) if x.size > 2 else math.inf, "last": big == x.size - 1}


def gap_holds(g):
    """p rounds UP on the 2^-52 grid with 25 ulp to spare against expf's E_EXP, u is above every admissible p and below the grid point
    by more than E_EXP + 1 ulp, both tokens sit in adjacent slices of one wave, se = fl32(1 + p) = 1, and the big token is not V - 1"""
    la, lb = g["lanes"]
    return (0.5 + (25 + E_EXP) / g["grid_ulps"] <= g["cell"] <= 1.0 - (25 + E_EXP) / g["grid_ulps"] and g["grid_ulps"] >= 256.0
            and g["u_above"] >= E_EXP + 2 and g["u_below"] >= E_EXP + 2 and g["exact_sub"] and lb == la + 1 and la // 64 == lb // 64
            and g["p"] * (1 + 2 * E_EXP * U) < 2.0 ** -25 and g["dead_below"] >= 150.0 and not g["last"])


# ======================================================================================================================
# multinomial cases
def draw_positions(V):
    per = per_thread(V)
    want = [0, V - 1, END, per - 1, per, 64 * per - 1, 64 * per, V // 2]
    pos = []
    for p in want:
        if 0 <= p < V and p not in pos:
            pos.append(p)
    return pos


def live_sets(V):
    per = per_thread(V)
    W = 64 * per
    sets = [[per - 1, per], [W - 2, W - 1, W, W + 1], [0, per - 1, per, W - 1, W, V // 2, V - 2, V - 1], [V - 2, V - 1]]
    out = []
    for s in sets:
        s = sorted({p for p in s if 0 <= p < V})
        if len(s) >= 2 and s not in out:
            out.append(s)
    return out


def live_u(n, k):
    """fp32 u in the middle of live token k's CDF interval (float64 softmax of LIVE_VALUES[:n]; the dead tokens weigh exp(-150))"""
    p = np.exp(np.asarray(LIVE_VALUES[:n], dtype=np.float64))
    c = np.concatenate([[0.0], np.cumsum(p / p.sum())])
    return np.float32(0.5 * (c[k] + c[k + 1]))


def draw_rows(V, exact_only=False, gap=False):
    """[(spec, u)] of the row families for a vocabulary (module docstring); exact_only: the rows whose draw is exact for ANY u (a, b);
    gap: with family (d), whose depth is finer than the grain of a designed slab sum (finished rows, ns = 1, only)"""
    rows = []
    if gap and not exact_only:
        for (a, b), start in zip(gap_positions(V), GAP_START):
            delta = gap_delta(start)
            rows.append((("gap", a, b, float(delta)), gap_u(delta)))
    for m in draw_positions(V):
        rows += [(("onehot", m), np.float32(u)) for u in US_ONEHOT]
    if V >= 2:
        for j in draw_positions(V):
            rows.append((("const",), np.float32((j + 0.5) / V)))
    # u = 1.0 (a float64 uniform just below 1 rounds to it in fp32): nothing is above the target, the draw is clamped to V - 1
    rows.append((("onehot", 0), np.float32(1.0)))
    if V >= 2:
        rows.append((("const",), np.float32(1.0)))
    for s in ([] if exact_only else live_sets(V)):
        for k in sorted({0, len(s) // 2, len(s) - 1}):
            rows.append((("live", s), live_u(len(s), k)))
    return rows


Sample = collections.namedtuple("Sample", "name V ns layout E emb_mode t row0 gate philox purpose")
# gate: "alive", "dead" (the counter that gates the kernel is 0 at t - 1), "sampled_dead" (merged: n_unfinished[t - 1] = 0, n_any[t - 1] > 0)
T_STEPS = 4


def _s(name, V, ns=1, layout="aligned", E=4, emb_mode=0, t=0, row0=0, gate="alive", philox=False, purpose=()):
    return Sample(name, V, ns, layout, E, emb_mode, t, row0, gate, philox, dict(purpose))


SAMPLE_CASES = (
    [_s("V%d" % V, V, t=(1 if V % 2 else 0), purpose={"V": V}) for V in (1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8195)]
    + [_s("V10239_ns4", 10239, ns=4, E=1024, emb_mode=1, t=2, purpose={"ns": 4, "emb_mode": 1}),
       _s("V4097_ns2_philox_emb", 4097, ns=2, E=4100, emb_mode=2, t=1, purpose={"ns": 2, "emb_mode": 2}),
       _s("V1025_emb_eval", 1025, E=1024, emb_mode=0, t=1, purpose={"emb_mode": 0, "E": 1024}),
       _s("V1025_dead", 1025, E=4, t=2, gate="dead", purpose={"gate": "dead"}),
       _s("V1025_philox", 1025, t=2, philox=True, E=4, emb_mode=2, purpose={"philox": True}),
       _s("V1025_merged1_alive", 1025, ns=2, E=1024, emb_mode=1, t=1, row0=1, purpose={"row0": 1, "gate": "alive"}),
       _s("V4097_merged32_alive", 4097, E=4, emb_mode=2, t=0, row0=32, purpose={"row0": 32, "gate": "alive"}),
       _s("V1025_merged32_sampled_dead", 1025, E=1024, emb_mode=1, t=2, row0=32, gate="sampled_dead", purpose={"row0": 32, "gate": "sampled_dead"}),
       _s("V1025_merged1_dead", 1025, E=4, t=3, row0=1, gate="dead", purpose={"row0": 1, "gate": "dead"})]
    + [_s("V4097_ns2_%s" % lay, 4097, ns=2, layout=lay, t=1, purpose={"scalar": lay != "aligned", "twin": "V4097_ns2_aligned"})
       for lay in ("aligned", "ldl_odd", "base_off", "stride_odd", "bias_off", "store_off")]
)
SAMPLE_BY_NAME = {c.name: c for c in SAMPLE_CASES}


def sample_inputs(c):
    """everything one launch reads: the sampled rows of draw_rows(V) behind row0 greedy rows (the standard greedy row set)"""
    rs = seeded("sample/" + (c.purpose.get("twin") or c.name))
    dr = draw_rows(c.V, exact_only=c.philox, gap=c.ns == 1)
    B = len(dr)
    gspecs = _greedy_specs(c.V, c.row0, c.ns, c.ns > 1, None) if c.row0 else []
    specs = gspecs + [s for s, _ in dr]
    slabs, bias = make_slabs(c.V, specs, c.ns, c.ns > 1, rs)
    seed = 0x1234ABCD5678EF01 ^ zlib.crc32(c.name.encode())
    u = np.array([uu for _, uu in dr], dtype=np.float32)
    if c.philox:
        u = _philox._uniforms(seed, T_STEPS, B)[c.t]
    unf = np.array([0 if r % 3 == 2 else 1 for r in range(B)], dtype=np.uint8)      # rows that finished at an earlier step
    gunf = np.array([0 if r % 3 == 2 else 1 for r in range(c.row0)], dtype=np.uint8)
    nunf, nany = np.zeros(T_STEPS, dtype=np.int32), np.zeros(T_STEPS, dtype=np.int32)
    if c.t > 0:
        nunf[c.t - 1] = 0 if c.gate in ("dead", "sampled_dead") else 3
        nany[c.t - 1] = 0 if c.gate == "dead" else 5
    mask = (rs.rand(B, c.E) < 0.5).astype(np.uint8)
    if c.emb_mode == 2:
        mask = _philox._keep_bits(seed, _philox.RNG_EMB, c.t + 1, B * c.E).reshape(B, c.E)
    return {"slabs": slabs, "bias": bias, "table": make_table(c.V, c.E, rs), "u": u, "unf": unf, "gunf": gunf, "nunf": nunf, "nany": nany,
            "mask": mask, "seed": seed, "B": B, "rows": B + c.row0}


def sample_ref(c, inp, log):
    """every output of one launch; None: left as it was.  Floats that carry a bound come as (values, bounds)."""
    B, rows, row0, t, V = inp["B"], inp["rows"], c.row0, c.t, c.V
    x = finish(inp["slabs"], inp["bias"])
    out = {"x": x if c.ns > 1 else None}
    dead_all = t > 0 and (inp["nany"] if row0 else inp["nunf"])[t - 1] == 0
    dead_s = dead_all or (row0 > 0 and t > 0 and inp["nunf"][t - 1] == 0)
    it_next, draw, lse, lseb = np.zeros(rows, np.int64), np.full(rows, -1, np.int32), np.zeros(rows), np.zeros(rows)
    emb = np.full((rows, c.E), FILL, dtype=np.float32)
    nunf, nany, unf, gunf = inp["nunf"].copy(), inp["nany"].copy(), inp["unf"].copy(), inp["gunf"].copy()
    seq, logp, lpb = np.zeros(B, np.int64), np.zeros(B), np.zeros(B)
    ids = np.zeros(row0, np.int64)
    if dead_all:
        out["x"] = None
    if not dead_all:
        for r in range(row0):                                   # greedy rows: evaluation mode
            ids[r] = it_next[r] = argmax_rule(x[r])
            gunf[r] = 1 if (t == 0 or inp["gunf"][r]) and ids[r] != END else 0
            nany[t] += int(gunf[r])
            emb[r] = embed_ref(inp["table"], ids[r], 1)
    if dead_s and not dead_all:                                 # the greedy half goes on: the sampled rows run on <pad>
        emb[row0:] = embed_ref(inp["table"], np.zeros(B, np.int64), 1)
        x_s = out["x"]
        if x_s is not None:
            out["x_rows"] = row0                                # only the greedy rows' finished logits are stored
    if not dead_s:
        sc = np.float32(2.0 if c.emb_mode else 1.0)
        for b in range(B):
            r = row0 + b
            d, lp, ls, b_lp, b_lse = draw_ref(x[r], inp["u"][b], log, (c.name, "row", b))
            alive = bool(inp["unf"][b]) and d != END
            tok = d if alive else 0
            unf[b], seq[b], it_next[r], draw[r] = int(alive), tok, tok, d
            logp[b], lpb[b], lse[r], lseb[r] = lp, b_lp, ls, b_lse
            nunf[t] += int(alive)
            nany[t] += int(alive) if row0 else 0
            e = np.maximum(inp["table"][tok], np.float32(0))
            emb[r] = np.where(inp["mask"][b] != 0, e * sc, np.float32(0)) if c.emb_mode else e
    out.update(seq=seq, logp=(logp, lpb), it_next=it_next, draw=draw, lse=(lse, lseb), unf=unf, nunf=nunf, gunf=gunf, nany=nany if row0 else None,
               ids=ids, emb=None if dead_all or t + 1 >= T_STEPS else emb, live_rows=None if dead_s else (t + 1) * rows, dead_all=dead_all, dead_s=dead_s)
    return out


# ======================================================================================================================
# scheduled sampling (ss_select_kernel): the draw rows of families (a) - (c) (its scan has no lower-bound test: no gap to ask about); gate g against ss_prob decides who draws
SsCase = collections.namedtuple("SsCase", "name V ss_prob philox purpose")
SS_CASES = ([SsCase("V%d_p%s" % (V, p), V, p, False, {"V": V}) for V, p in ((3, 0.5), (1025, 0.5), (4097, 1.0), (4097, 0.0), (8195, 0.5))]
            + [SsCase("V1025_philox", 1025, 0.5, True, {"philox": True})])
SS_T = 3                           # gate / draw are [SS_T, B]; the step under test is SS_T - 1


def ss_inputs(c):
    rs = seeded("ss/" + c.name)
    dr = draw_rows(c.V, exact_only=c.philox)
    B = len(dr)
    slabs, _ = make_slabs(c.V, [s for s, _ in dr], 1, False, rs)
    seed = 0x0F1E2D3C4B5A6978 ^ zlib.crc32(c.name.encode())
    gate = np.full((SS_T, B), np.nan, dtype=np.float32)
    draw = np.full((SS_T, B), np.nan, dtype=np.float32)
    gate[SS_T - 1] = np.where(np.arange(B) % 3 == 1, 0.75, 0.25)
    draw[SS_T - 1] = [uu for _, uu in dr]
    if c.philox:
        gate = _philox._uniforms(seed, SS_T, B, _philox.RNG_SS_GATE)
        draw = _philox._uniforms(seed, SS_T, B, _philox.RNG_SS_DRAW)
    tok = (3 + np.arange(B) % 5).astype(np.int64)
    return {"x": slabs[0], "gate": gate, "draw": draw, "tok": tok, "seed": seed, "B": B}


def ss_ref(c, inp, log):
    tok = inp["tok"].copy()
    for b in range(inp["B"]):
        if inp["gate"][SS_T - 1, b] < np.float32(c.ss_prob):
            tok[b] = draw_ref(inp["x"][b], inp["draw"][SS_T - 1, b], log, (c.name, "row", b))[0]
    return tok


# ======================================================================================================================
# XE loss.  B x T, ragged rows_t, smoothing, n_dev (None absent, 0.0, positive)
Xe = collections.namedtuple("Xe", "name B T V smoothing n_dev purpose")
XE_CASES = (
    Xe("5x4_s0.1", 5, 4, 203, 0.1, None, {"ragged": True}),
    Xe("5x4_s0", 5, 4, 203, 0.0, 0.0, {"smoothing": 0, "n_dev": 0}),
    Xe("5x4_s1", 5, 4, 203, 1.0, 37.0, {"smoothing": 1, "n_dev": 37}),
    Xe("33x3_V1025", 33, 3, 1025, 0.1, None, {"B": 33}),
    Xe("2x128_V5", 2, XE_MAX_T, 5, 0.1, 11.0, {"T": XE_MAX_T}),
    Xe("5x4_V2", 5, 4, 2, 0.1, None, {"V": 2}),
)


def xe_inputs(c):
    rs = seeded("xe/" + c.name)
    B, T, V = c.B, c.T, c.V
    lengths = np.sort(rs.randint(1, T + 1, size=B))[::-1].copy()
    lengths[0] = T
    rows_t = [int((lengths > t).sum()) for t in range(T)]
    L = T + 2
    cap = rs.randint(0, V, size=(B, L)).astype(np.int64)
    cap[0, 1], cap[0, 2 if T > 1 else 1] = 0, V - 1               # targets at 0 and at V - 1 (steps 0 and 1 of row 0)
    if T == 1:
        cap[0, 1] = V - 1
    x = (4.0 * rs.standard_normal((T * B, V))).astype(np.float32)
    for i, (t, b) in enumerate([(0, 0), (1 % T, 0)]):              # sharpened until the softmax saturates: on and off the target
        row = -150.0 - rs.randint(0, 2049, size=V) * Q
        row[cap[b, t + 1] if i == 0 else (cap[b, t + 1] + 1) % V] = 1.0
        if V > 2 or i == 0:
            x[t * B + b] = row.astype(np.float32)
    return {"x": x, "cap": cap, "rows_t": rows_t, "L": L, "n_tokens": float(sum(rows_t))}


def xe_ref(c, inp):
    """(grad [TB, V], grad bound, loss_rows, row bounds, loss, loss bound, active [TB])"""
    B, T, V, s = c.B, c.T, c.V, c.smoothing
    ldl = pad_vocab(V)
    n32 = np.float32(c.n_dev) if c.n_dev else np.float32(inp["n_tokens"])
    N = float(n32)
    conf, low = float(np.float32(1.0) - np.float32(s)), float(np.float32(s) / np.float32(V - 1))
    g, gb = np.zeros((T * B, V)), np.zeros((T * B, V))
    rows, rb, act = np.zeros(T * B), np.zeros(T * B), np.zeros(T * B, dtype=bool)
    for t in range(T):
        for b in range(inp["rows_t"][t]):
            r = t * B + b
            act[r] = True
            x = inp["x"][r]
            lpb = row_bounds(x, n_add_xe(V))[0]
            d64 = x.astype(np.float64) - float(x.max())
            lp = d64 - math.log(np.exp(d64).sum())
            tr = np.full(V, low)
            tr[inp["cap"][b, t + 1]] = conf
            p = np.exp(lp)
            g[r] = (p - tr) / N
            gb[r] = ((lpb + 2 * E_EXP * U) * p + TINY + 3 * U * (p + tr)) / N
            with np.errstate(divide="ignore", invalid="ignore"):
                ltr = np.where(tr > 0, np.log(np.where(tr > 0, tr, 1.0)), 0.0)
            term = np.where(tr > 0, tr * (ltr - lp), 0.0)
            rows[r] = term.sum()
            rb[r] = (-(-ldl // 256) + 14) * U * np.abs(term).sum() + lpb + 2 * E_LOG * U * np.abs(ltr).max()
    loss = rows.sum() / N
    lb = ((-(-T * B // 256) + 13) * U * np.abs(rows).sum() + rb.sum()) / N
    return g, gb, rows, rb, loss, lb, act


# ======================================================================================================================
# REINFORCE.  msum: None absent, 0.0, positive; Bs / row0: the merged layout
Rf = collections.namedtuple("Rf", "name B T V msum Bs row0 purpose")
RF_CASES = (
    Rf("5x4", 5, 4, 203, None, 0, 0, {}),
    Rf("5x4_msum0", 5, 4, 203, 0.0, 0, 0, {"msum": 0}),
    Rf("33x9_msum", 33, 9, 1025, 123.0, 0, 0, {"BT>256": True, "msum": 123}),
    Rf("4x5_merged", 4, 5, 203, None, 8, 4, {"merged": True}),
    Rf("3x4_merged_row0_2", 3, 4, 5, 7.0, 5, 2, {"merged": True}),
)


def rf_inputs(c):
    rs = seeded("rf/" + c.name)
    B, T, V = c.B, c.T, c.V
    Bs = c.Bs or B
    seq = rs.randint(1, V, size=(B, T)).astype(np.int64)
    for b in range(B):                                           # rows end at different steps; behind the end: zeros
        end = rs.randint(0, T + 1)
        seq[b, end:] = 0
    seq[0, :] = 1 + np.arange(T) % (V - 1)                       # one row never ends
    seq[B - 1, :] = 0                                            # one row ends at once: only its t == 0 column counts
    logp = (-3.0 * rs.rand(B, T)).astype(np.float32)
    reward = rs.standard_normal((B, T)).astype(np.float32)
    reward[1 % B, :] = 0.0                                       # a zero reward: an exactly zero gradient row, even over NaN logits
    x = (4.0 * rs.standard_normal((T * Bs, V))).astype(np.float32)
    d64 = x.astype(np.float64)
    lse = (d64.max(1) + np.log(np.exp(d64 - d64.max(1, keepdims=True)).sum(1))).astype(np.float32)
    draw = rs.randint(0, V, size=T * Bs).astype(np.int32)
    draw[c.row0::Bs] = np.where(np.arange(T) % 2 == 0, 0, V - 1)       # draws at 0 and at V - 1 (the rollout's first row)
    for t in range(T):
        for j in range(Bs):
            b = j - c.row0
            if b < 0 or b >= B:
                draw[t * Bs + j] = -1                            # an evaluation-mode row of the merged chain
                x[t * Bs + j] = np.nan
            elif b == 1 % B:
                x[t * Bs + j] = np.nan
    return {"seq": seq, "logp": logp, "reward": reward, "x": x, "lse": lse, "draw": draw, "Bs": Bs}


def rf_ref(c, inp):
    B, T, V, Bs = c.B, c.T, c.V, inp["Bs"]
    mask = np.ones((B, T))
    mask[:, 1:] = inp["seq"][:, :-1] > 0
    ms = mask.sum()
    denom = float(np.float32(c.msum)) if c.msum else ms
    terms = -inp["logp"].astype(np.float64) * inp["reward"].astype(np.float64) * mask
    loss = terms.sum() / denom
    lb = (-(-B * T // 256) + 15) * U * np.abs(terms).sum() / denom
    coef = -inp["reward"].astype(np.float64) * mask / denom
    g, gb = np.zeros((T * Bs, V)), np.zeros((T * Bs, V))
    zero = np.ones(T * Bs, dtype=bool)
    for t in range(T):
        for b in range(B):
            r = t * Bs + c.row0 + b
            cc = coef[b, t]
            if cc == 0.0 or inp["draw"][r] < 0:
                continue
            zero[r] = False
            a = inp["x"][r].astype(np.float64) - float(inp["lse"][r])
            p = np.exp(a)
            ind = (np.arange(V) == inp["draw"][r]).astype(np.float64)
            g[r] = cc * (ind - p)
            gb[r] = abs(cc) * (p * (U * np.abs(a) + 2 * E_EXP * U) + TINY + U * np.abs(ind - p)) + 3 * U * np.abs(g[r])
    return {"mask": mask, "ms": ms, "loss": loss, "loss_bound": lb, "coef": coef, "coef_bound": 2 * U * np.abs(coef), "g": g, "g_bound": gb,
            "zero_rows": zero}
