"""Case tables and float64 references of the kernels that finish a backward pass and apply the update, each on its own
(tests/test_cpu_support_kernels.py holds every case to its stated purpose on the host and every reference to an independent
statement; tests/test_gpu_support_kernels.py runs the tables through the icz_test_* entries).  Plain numpy, no pytest, no torch.

A case is name -> shape -> purpose: the purpose is data (which side of a threshold, which occurrence counts, which job has ragged
rows), so that the CPU test can recompute it; where the threshold is the library's it asks icz_embed_grad_route_for.

Bounds are a-priori rounding bounds (u = 2^-24, one fp32 rounding), never fitted to a device:
  a sum            (fp32 additions on the element's path + 2) u sum|addends|, magnitudes in float64
  weight_norm      (cols + 8) u relative on w and norm; the backward the same count on |dw| + |v| sum|v dw| / ||v||^2, times |g| / ||v||
  Adam             4 u on m and v against |m b1| + |g (1 - b1)| (and likewise v), 16 u on the step against |p| + |update|
Every reference returns (value, bound) pairs as float64 arrays."""
import collections
import math
import zlib

import numpy as np

U = 2.0 ** -24
GUARD = 7.0


def seeded(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


# ======================================================================================================================
# embedding gradient (embed_grad_kernel = route 1, embed_grad_win_kernel = route 2; route 0 = what the decoders' launch picks)
EG_ROWS, EG_WIN, EG_BATCH = 8, 1024, 8         # vocabulary rows per workgroup, list entries per window, loads in flight
EG_SCALES, EG_RELU = (1.0, 2.0), (0, 1)

EgCase = collections.namedtuple("EgCase", "name n_tok E V tokens routes ns live purpose")


def _eg(name, n_tok, E, V, tokens, routes=(1, 2), ns=1, live=None, **purpose):
    return EgCase(name, n_tok, E, V, tokens, tuple(routes), ns, live, purpose)


# tokens: ("counts", {token: occurrences})   shuffled; every other token absent
#         ("whole", token)                   one token fills the list
#         ("pair", token, (i, j))            the token at exactly these indices, the other tokens anywhere else
#         ("random", heavy)                  uniform over the vocabulary with ~30 % of the entries the heavy token
# purpose keys (each one recomputed by test_cpu_support_kernels.py):
#   counts          occurrence counts that individual tokens have: 0, and both sides of the 8-deep load batch and of two batches
#   last_block_rows rows of the last vocabulary block (< 8)
#   windows         windows the list spans;  straddle = (token, i, j): its only occurrences, i in one window and j in the next
#   live_cut        where rows_live cuts: "empty", "first", "boundary" (exactly one window), "inside" (inside the second window and
#                   inside the heavy token's list), "beyond" (more than n_tok: the whole list)
#   e_trips         column groups of 1024 a wave walks on the LDS form;  e_wave = side of one wave's 256 columns (-1, 0, +1)
#   lds_side        side of the 48 KB dynamic-LDS opt-in (-1: at or below, +1: above)
#   route0          the form route 0 takes (the library's switch at ~159 KB of LDS)
#   slabs           slabs summed per occurrence
EG_CASES = [
    _eg("hits", 58, 8, 21, ("counts", {1: 1, 2: 7, 3: 8, 4: 9, 17: 16, 20: 17}), counts=(0, 1, 7, 8, 9, 16, 17), last_block_rows=5),
    _eg("whole_1023", 1023, 8, 21, ("whole", 5), windows=1, counts=(1023,)),
    _eg("whole_1024", 1024, 8, 21, ("whole", 5), windows=1, counts=(1024,)),
    _eg("whole_1025", 1025, 8, 21, ("whole", 5), windows=2, counts=(1025,)),
    _eg("whole_2049", 2049, 8, 21, ("whole", 13), windows=3, counts=(2049,)),
    _eg("straddle_1025", 1025, 8, 21, ("pair", 6, (1023, 1024)), windows=2, straddle=(6, 1023, 1024)),
    _eg("straddle_2049", 2049, 8, 21, ("pair", 18, (1023, 1024)), windows=3, straddle=(18, 1023, 1024)),
    _eg("live_0", 1040, 8, 21, ("random", 3), live=0, live_cut="empty"),
    _eg("live_1", 1040, 8, 21, ("random", 3), live=1, live_cut="first"),
    _eg("live_1024", 1040, 8, 21, ("random", 3), live=1024, live_cut="boundary"),
    _eg("live_1030", 1040, 8, 21, ("random", 3), live=1030, live_cut="inside"),
    _eg("live_5000", 1040, 8, 21, ("random", 3), live=5000, live_cut="beyond"),
    _eg("wide_4", 40, 4, 10, ("random", 9), e_trips=1, e_wave=-1, last_block_rows=2),
    _eg("wide_252", 40, 252, 10, ("random", 9), routes=(1,), e_trips=1, e_wave=-1),
    _eg("wide_256", 40, 256, 10, ("random", 9), routes=(1,), e_trips=1, e_wave=0),
    _eg("wide_260", 40, 260, 10, ("random", 9), routes=(1,), e_trips=1, e_wave=1),
    _eg("wide_1020", 40, 1020, 10, ("random", 9), routes=(2,), e_trips=1),
    _eg("wide_1024", 40, 1024, 10, ("random", 9), e_trips=1),
    _eg("wide_1028", 40, 1028, 10, ("random", 9), routes=(1,), e_trips=2),
    _eg("lds_1365", 1365, 4, 21, ("random", 0), routes=(0, 1), lds_side=-1, route0=1),
    _eg("lds_1366", 1366, 4, 21, ("random", 0), routes=(0, 1), lds_side=1, route0=1),
    _eg("switch_4522", 4522, 4, 21, ("random", 20), routes=(0, 1, 2), route0=1),
    _eg("switch_4523", 4523, 4, 21, ("random", 20), routes=(0, 2), route0=2),
    _eg("slabs_1", 70, 8, 21, ("random", 2), ns=1, slabs=1),
    _eg("slabs_3", 70, 8, 21, ("random", 2), ns=3, slabs=3),
]
EG_BY_NAME = {c.name: c for c in EG_CASES}
# refused: (n_tok, E, route) -- the windowed form above 1024 columns, the LDS form above its list length, E no multiple of 4
EG_REFUSED = [(40, 1028, 2), (4523, 4, 1), (40, 6, 0), (40, 6, 1), (4523, 1028, 0)]
EG_SLAB_PAD = 12          # floats of NaN between two slabs (slab_stride = n_tok E + 12)


def eg_tokens(c):
    rs = seeded("tok " + c.name)
    kind = c.tokens[0]
    if kind == "counts":
        t = np.concatenate([np.full(n, tok) for tok, n in sorted(c.tokens[1].items())])
        assert len(t) == c.n_tok
        return rs.permutation(t).astype(np.int64)
    if kind == "whole":
        return np.full(c.n_tok, c.tokens[1], dtype=np.int64)
    if kind == "pair":
        tok, where = c.tokens[1], c.tokens[2]
        others = np.array([v for v in range(c.V) if v != tok])
        t = others[rs.randint(0, len(others), c.n_tok)]
        t[list(where)] = tok
        return t.astype(np.int64)
    heavy = c.tokens[1]
    t = rs.randint(0, c.V, c.n_tok)
    t[rs.rand(c.n_tok) < 0.3] = heavy
    return t.astype(np.int64)


def eg_inputs(c):
    """(tok [n_tok] int64, demb [ns, n_tok, E] fp32, emb [n_tok, E] fp32).  emb is exactly 0 where (i + j) % 5 == 0 and negative
    where (i + j) % 5 == 1: the places where `> 0` differs from `>= 0` and from no test at all."""
    rs = seeded("in " + c.name)
    tok = eg_tokens(c)
    demb = rs.standard_normal((c.ns, c.n_tok, c.E)).astype(np.float32)
    emb = rs.standard_normal((c.n_tok, c.E)).astype(np.float32)
    ij = np.add.outer(np.arange(c.n_tok), np.arange(c.E)) % 5
    emb[ij == 0] = 0.0
    emb[ij == 1] = -np.abs(emb[ij == 1]) - np.float32(0.125)
    return tok, demb, emb


def embed_grad_ref(tok, demb, emb, scale, relu, V, live=None):
    """dE [V, E] in float64 and its bound.  Per occurrence the kernels add ns - 1 times for the slabs and once onto the row's sum
    (the product with scale = 1 or 2 is exact): nh ns roundings for a token that occurs nh times, + 2."""
    ns, n, E = demb.shape
    n = n if live is None else min(n, max(int(live), 0))
    t = tok[:n]
    keep = (emb[:n] > 0) if relu else np.ones((n, E), dtype=bool)
    val = demb[:, :n].astype(np.float64).sum(0) * keep * float(scale)
    mag = np.abs(demb[:, :n].astype(np.float64)).sum(0) * keep * float(scale)
    ref, amag = np.zeros((V, E)), np.zeros((V, E))
    np.add.at(ref, t, val)
    np.add.at(amag, t, mag)
    nh = np.bincount(t, minlength=V)[:V]
    return ref, (nh * ns + 2)[:, None] * U * amag


# ======================================================================================================================
# weight_norm / weight_norm_bwd: single-matrix kernels and the table forms (4 rows per block, blocks job after job)
WN_ROWS, WN_COLS = (1, 3, 4, 5, 9), (4, 252, 256, 260, 1028)          # columns: both sides of one wave's 256-column trip, five trips
WN_SINGLE = [(r, c) for r in WN_ROWS for c in WN_COLS]
# table name -> [(rows, cols)]; ragged = jobs whose rows % 4 != 0 and which another job follows (its last block's idle waves sit
# beside the next job's rows)
WN_TABLES = collections.OrderedDict([
    ("1job", [(5, 260)]),
    ("2jobs", [(3, 256), (4, 4)]),
    ("3jobs", [(4, 252), (5, 1028), (1, 4)]),
    ("4jobs", [(9, 260), (3, 4), (1, 1028), (8, 256)]),
])
WN_RAGGED = {"1job": (), "2jobs": (0,), "3jobs": (1,), "4jobs": (0, 1, 2)}
WN_MAX_JOBS = 4
WN_BWD_PAD = 8            # lddw = cols + 8, NaN in the padding


def wn_inputs(rows, cols, tag=""):
    """(v, g, dw) fp32; g of both signs, bounded away from 0."""
    rs = seeded("wn %d %d %s" % (rows, cols, tag))
    v = rs.standard_normal((rows, cols)).astype(np.float32)
    g = (rs.uniform(0.5, 2.0, rows) * rs.choice([-1.0, 1.0], rows)).astype(np.float32)
    dw = rs.standard_normal((rows, cols)).astype(np.float32)
    return v, g, dw


def weight_norm_ref(v, g):
    """w = v g / ||v||, norm = ||v|| -> ((w, bound), (norm, bound)): cols squares and additions, a square root, a division, a
    product: (cols + 8) u relative."""
    v64, g64 = v.astype(np.float64), g.astype(np.float64)
    nrm = np.sqrt((v64 * v64).sum(1))
    w = v64 * (g64 / nrm)[:, None]
    k = (v.shape[1] + 8) * U
    return (w, k * np.abs(w)), (nrm, k * nrm)


def weight_norm_bwd_ref(dw, v, g, norm):
    """dg = dw . v / ||v||, dv = (g / ||v||) (dw - (dg / ||v||) v) with ||v|| the fp32 `norm` the kernel is handed ->
    ((dv, bound), (dg, bound)).  The dot product's error, (cols + 8) u sum|v dw|, reaches dv through |v| / ||v||^2."""
    dw64, v64, g64, n64 = dw.astype(np.float64), v.astype(np.float64), g.astype(np.float64), norm.astype(np.float64)
    dot, adot = (dw64 * v64).sum(1), np.abs(dw64 * v64).sum(1)
    dg = dot / n64
    dv = (g64 / n64)[:, None] * (dw64 - (dg / n64)[:, None] * v64)
    k = (v.shape[1] + 8) * U
    bdv = k * (np.abs(dw64) + np.abs(v64) * (adot / (n64 * n64))[:, None]) * (np.abs(g64) / n64)[:, None]
    return (dv, bdv), (dg, k * adot / n64)


# ======================================================================================================================
# transpose_multi: table name -> [(rows, cols, ld, column offset of the source inside its [rows, ld] buffer)]
TR_TABLES = collections.OrderedDict([
    ("1job", [(64, 64, 64, 0)]),
    ("2jobs", [(128, 192, 200, 0), (64, 64, 72, 4)]),
    ("3jobs", [(192, 64, 64, 0), (64, 192, 196, 4), (128, 64, 136, 68)]),
    ("4jobs", [(128, 192, 192, 0), (128, 64, 64, 0), (128, 64, 328, 8), (192, 192, 192, 0)]),       # the decoder's four, td_w_ih third
])
TR_MAX_JOBS = 4
# refused single jobs (rows, cols, ld): ragged rows, ragged columns, ld below the columns, ld no multiple of 4
TR_REFUSED = [(96, 64, 64), (64, 96, 96), (64, 128, 64), (64, 64, 66), (0, 64, 64)]


# ======================================================================================================================
# colsum / colsum_multi: 32 columns x 8 row groups per block; a group loads 8 rows at once while k + 56 < K
COLSUM_K = (0, 1, 7, 8, 9, 56, 57, 63, 64, 65, 121, 129)
COLSUM_N = (1, 31, 32, 33, 65)
COLSUM_PAD = 3            # ldx = N + 3, NaN in the padding
# table name -> [(K, N, ldx, out2 present)]
COLSUM_TABLES = collections.OrderedDict([
    ("1job", [(9, 33, 36, False)]),
    ("3jobs", [(57, 65, 68, True), (0, 1, 1, False), (8, 31, 31, False)]),
    ("6jobs", [(64, 32, 32, True), (65, 33, 40, True), (7, 1, 4, False), (129, 65, 65, False), (121, 32, 35, False), (0, 1, 1, False)]),
    ("8jobs", [(1, 1, 1, False), (63, 31, 33, True), (0, 33, 33, True), (56, 65, 66, False), (9, 32, 32, False), (57, 1, 2, True),
               (64, 33, 36, False), (129, 31, 31, True)]),
])
COLSUM_MAX_JOBS = 8


def colsum_batches(K, g):
    """8-row load batches row group g takes before its one-by-one tail."""
    n, k = 0, g
    while k + 56 < K:
        n, k = n + 1, k + 64
    return n


def colsum_ref(X):
    """Column sums of X [K, N] and their bound: a group adds ceil(K / 8) rows, the eight groups meet in 7 more additions."""
    x = X.astype(np.float64)
    K = X.shape[0]
    return x.sum(0), ((K + 7) // 8 + 8) * U * np.abs(x).sum(0)


# ======================================================================================================================
# timesum / rowgroup_sum: one thread per 4 floats, 1024 floats per block
SUM_DEPTHS = (1, 2, 5, 8)
SUM_WIDTHS = (4, 1020, 1024, 1028)
SUM_IMAGES = (1, 3)


def depth_sum_ref(X):
    """Sum over axis 0 of X [depth, ...], added in order: depth - 1 additions, + 2."""
    x = X.astype(np.float64)
    return x.sum(0), (X.shape[0] - 1 + 2) * U * np.abs(x).sum(0)


# ======================================================================================================================
# Adam with clamped gradients: adam_clamp_kernel (one element per thread) and adam_clamp_multi_kernel (four per thread: a 16-byte
# path, and a scalar path at a tensor's tail or when one of the four pointers is not 16-byte aligned)
ADAM_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4097)
ADAM_STEPS = (1, 2, 1000)
ADAM_CLIP, ADAM_LR = 0.1, 0.05
ADAM_BLOCK = 1024
# float offsets of (p, g, m, v) from a 16-byte boundary
ADAM_VARIANTS = collections.OrderedDict([
    ("aligned", (0, 0, 0, 0)), ("off1", (1, 1, 1, 1)), ("off2", (2, 2, 2, 2)), ("off3", (3, 3, 3, 3)),
    ("only_p", (1, 0, 0, 0)), ("only_g", (0, 1, 0, 0)), ("only_m", (0, 0, 1, 0)), ("only_v", (0, 0, 0, 1)),
])
ADAM_MAX_TENSORS = 32
ADAM_32 = (1024, 3, 2048, 1, 1025, 4, 1023, 5, 4097, 7, 1024, 2, 9, 3072, 6, 1, 1026, 8, 2047, 1024, 5, 4096, 3, 2049, 11, 4, 1022, 1, 2048,
           13, 1025, 1024)
ADAM_ZERO_STRETCH = (500, 520)       # sizes above 520: g = m = v = 0 here (whole 16-byte groups and more)


def adam_inputs(n, tag=""):
    """(p, g, m, v) fp32 of n elements.  Gradients by index % 8: inside the clip (0, 6, 7), above it (1), exactly +clip (2), exactly
    -clip (3), below -clip (4), and g = m = v = 0 (5; and the whole ADAM_ZERO_STRETCH).  |p| in [0.25, 1] and sqrt(v) in [0.05, 0.2]
    keep the step's bound away from cancellation in m."""
    rs = seeded("adam %d %s" % (n, tag))
    clip = np.float32(ADAM_CLIP)
    p = (rs.uniform(0.25, 1.0, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    g = rs.uniform(-0.09, 0.09, n).astype(np.float32)
    m = rs.uniform(-0.2, 0.2, n).astype(np.float32)
    v = (rs.uniform(0.05, 0.2, n) ** 2).astype(np.float32)
    i = np.arange(n)
    g[i % 8 == 1] = np.float32(0.5)
    g[i % 8 == 2] = clip
    g[i % 8 == 3] = -clip
    g[i % 8 == 4] = np.nextafter(-clip, np.float32(-1.0))
    zero = adam_zero_state(n)
    g[zero], m[zero], v[zero] = 0.0, 0.0, 0.0
    return p, g, m, v


def adam_zero_state(n):
    i = np.arange(n)
    return (i % 8 == 5) | ((i >= ADAM_ZERO_STRETCH[0]) & (i < ADAM_ZERO_STRETCH[1]))


def adam_constants(step):
    """The constants as the host and the kernels form them: the bias corrections in double, rounded to fp32; 0.9f, 0.999f, 1e-8f."""
    bc1 = float(np.float32(1.0 - 0.9 ** step))
    sbc2 = float(np.float32(math.sqrt(1.0 - 0.999 ** step)))
    b1, b2, eps = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))
    return bc1, sbc2, b1, float(np.float32(1.0) - np.float32(0.9)), b2, float(np.float32(1.0) - np.float32(0.999)), eps


def adam_ref(p, g, m, v, lr, clip, step):
    """torch.optim.Adam's update on gradients clamped to +-clip, in float64 -> {"p" / "m" / "v": (value, bound)}.
    m and v: two products and a sum, 4 u.  The step: m (4), sqrt v (2), / sqrt_bc2, + eps, the quotient, lr / bc1, the product, the
    difference: 12 roundings, 16 u against |p| + |update|."""
    bc1, sbc2, b1, omb1, b2, omb2, eps = adam_constants(step)
    lr, clip = float(np.float32(lr)), float(np.float32(clip))
    p64, m64, v64 = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    gc = np.clip(g.astype(np.float64), -clip, clip)
    mn = m64 * b1 + gc * omb1
    vn = v64 * b2 + gc * gc * omb2
    upd = (lr / bc1) * (mn / (np.sqrt(vn) / sbc2 + eps))
    return {"m": (mn, 4 * U * (np.abs(m64 * b1) + np.abs(gc * omb1))),
            "v": (vn, 4 * U * (np.abs(v64 * b2) + np.abs(gc * gc * omb2))),
            "p": (p64 - upd, 16 * U * (np.abs(p64) + np.abs(upd)))}
