"""Case tables, float64 references and a-priori bounds of the AoA kernels, each on its own (tests/test_cpu_aoa_kernels.py holds every case
to its stated purpose, every reference to oracle/aoa.py in float64 and every bound to "neither too tight nor too loose";
tests/test_gpu_aoa_kernels.py runs the tables through the icz_test_aoa_* entries).  Plain numpy, no pytest, no torch.

Kernels: layer_norm_kernel (both launch geometries), mha_self_kernel (route 1, any query chunk) and mha_self_mfma_kernel (route 2),
aoa_dec_attn_kernel, aoa_dec_attn_bwd_kernel, aoa_dkv_kernel, aoa_ln_bwd_kernel, aoa_ln_bwd_dense_kernel and mha_self_bwd_kernel (the
bounds of the last five stand above their sections).  A case is name -> shape -> purpose; the purpose is data, so that the CPU test can
recompute it from predicates written out from the code (and, where the threshold is the library's, from icz_aoa_self_attn_route_for).

Bounds (u = 2^-24, one fp32 rounding; every one first order in u with the additions counted two too many for the terms of second
order; magnitudes in float64).  A sum of fp32 terms along a path of L additions is off by at most L u sum|terms|, whatever the order and
whether or not products are fused into the additions.

  LayerNorm  L = ceil(n / 64) + 12 covers the longest addition chain of either branch (registers: 4 ceil(n / 256) per lane + 6 shuffle
             levels; re-read: ceil(n / 64) + 6).  With c = x - mean, q = sum c^2, s = sqrt(q / (n - 1)), inv = 1 / (s + eps):
    E_mean = (L + 1) u sum|x| / n                                   the sum, then one division
    E_c    = E_mean + u |c|                                         the subtraction
    E_q    = 2 sum(|c| E_c) + (L + 2) u q                           d(c^2) = 2 c dc; products and additions of the second sum
    E_s    = s (E_q / (2 q) + 2 u)                                  sqrt halves a relative error; division and sqrt round once each
    E_inv  = inv ((E_s + u (s + eps)) / (s + eps) + u)              the addition of eps, then one division
    E_y    = |g| (E_c inv + |c| E_inv) + 3 u |g c inv| + u |b|      two products and the last addition
  attention (both kinds)  d = head width, len = valid keys, A = sum_j |q_j k_j|, scale = 1 / sqrt(d):
    E_S    = (d + 5) u A scale                                      d additions + 2, the scale's sqrt and division, the product
    eta    = E_S + u |S - max S| + 2 u                              the subtraction in front of expf, expf within 1 ulp = 2 u
    E_P    = P (eta + sum_k P_k eta_k + 10 u)                       softmax is shift invariant, so the rounded maximum costs nothing;
                                                                    d log P_k = eta_k - sum_j P_j eta_j; the sum of len <= 128 positive
                                                                    terms has <= 8 additions on a path, one division
    E_Pd   = f (E_P + u P)                                          f = 0, 1 or the fp32 1 / (1 - p): one product
    E_O    = sum_k E_Pd |v_k| + (len + 2) u sum_k Pd_k |v_k|        len additions
  A row of P sums to 1 within 8 u = 4 ulps of 1: <= 7 additions of positive terms in front of the division, and the division.
Every reference returns (value, bound) pairs as float64 arrays; no element is excused."""
import collections
import math
import zlib

import numpy as np

U = 2.0 ** -24
EPS = float(np.float32(1e-6))          # the kernels' 1e-6f
GUARD = 7.0
LDS_BUDGET = 156 * 1024
LDS_OPTIN = 48 * 1024


def seeded(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def drop_scale(p):
    """The library's keep factor: 1.0f / (1.0f - p) in fp32 (aoa_dropp, aoa_impl.h), as a float64 number."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ---- fp32 sums in a stated order (the "not too tight" emulations) ---------------------------------------------------------------
def sum32(a, order):
    """Sum of the fp32 array over its last axis in fp32: 'ascending' (one running sum) or 'pairwise' (neighbours, level by level)."""
    a = np.asarray(a, dtype=np.float32)
    if order == "ascending":
        return np.cumsum(a, axis=-1, dtype=np.float32)[..., -1]
    assert order == "pairwise"
    while a.shape[-1] > 1:
        if a.shape[-1] & 1:
            a = np.concatenate([a, np.zeros(a.shape[:-1] + (1,), np.float32)], -1)
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


ORDERS = ("ascending", "pairwise")


# ======================================================================================================================
# layer_norm_kernel
LnCase = collections.namedtuple("LnCase", "name geometry rows n stats live purpose")
LN_N = (4, 8, 252, 256, 260, 1024, 2048, 2052, 10)
LN_ROWS = (1, 3, 4, 5)


def ln_path(n):
    """The kernel's branch, written out from layer_norm_kernel: the row in registers, or re-read with scalar loads."""
    return "registers" if n <= 2048 and n % 4 == 0 else "fallback"


def ln_blocks(geometry, rows):
    """(workgroups, waves per workgroup, idle waves of the last workgroup) of a launch geometry (aoa_launch_layer_norm)."""
    if geometry == 0:
        nb = (rows + 3) // 4
        return nb, 4, 4 * nb - rows
    return rows, 1, 0


def _ln(name, geometry, rows, n, stats, live, why):
    return LnCase(name, geometry, rows, n, stats, live,
                  dict(path=ln_path(n), trips=(n + 255) // 256 if ln_path(n) == "registers" else (n + 63) // 64,
                       idle_waves=ln_blocks(geometry, rows)[2], why=why))


def _ln_cases():
    out = []
    for g in (0, 1):           # every width in both geometries: 5 rows = one full workgroup and one wave of the next (geometry 0)
        for n in LN_N:
            out.append(_ln("g%d_n%d" % (g, n), g, 5, n, g == 1, None, "width %d: %s" % (n, ln_path(n))))
        for rows in LN_ROWS:   # the row tail of the four-rows-per-workgroup launch, one wave and a bit (260 columns)
            out.append(_ln("g%d_rows%d" % (g, rows), g, rows, 260, rows % 2 == 1, None, "%d rows" % rows))
        for n in (256, 10):    # the early return of a dead step, and a live one, on both branches
            for live in (1, 0):
                out.append(_ln("g%d_n%d_live%d" % (g, n, live), g, 3, n, True, live, "live = %d on the %s branch" % (live, ln_path(n))))
    return out


LN_CASES = _ln_cases()
LN_SCALES = ((1e-3, 0.0), (1.0, 0.0), (30.0, 0.0), (1.0, 3.0), (0.05, -2.0))      # (spread, offset) of row r % 5
# refused on the host: (geometry, rows, n, misaligned) -- a geometry that does not exist, no row, one column, a 16-byte path off a boundary
LN_REFUSED = [(2, 3, 8, False), (0, 0, 8, False), (1, 3, 1, False), (0, 3, 8, True)]


def ln_inputs(c):
    """x [rows, n], gain [n], bias [n] (fp32).  Row r has the spread and offset LN_SCALES[r % 5]: the first row's std of 1e-3 is where
    eps outside the sqrt differs from eps inside it."""
    rs = seeded("ln " + c.name)
    x = rs.standard_normal((c.rows, c.n))
    for r in range(c.rows):
        sc, of = LN_SCALES[r % len(LN_SCALES)]
        x[r] = x[r] * sc + of
    return x.astype(np.float32), rs.standard_normal(c.n).astype(np.float32), rs.standard_normal(c.n).astype(np.float32)


def ln_depth(n):
    return (n + 63) // 64 + 12


def layer_norm_ref(x, gain, bias, mut=None):
    """-> dict y / mean / inv -> (value, bound).  mut: 'biased_std' (divide by n), 'eps_inside' (sqrt(var + eps))."""
    x, g, b = (np.asarray(a, dtype=np.float64) for a in (x, gain, bias))
    n = x.shape[1]
    L = ln_depth(n)
    mean = x.mean(1, keepdims=True)
    c = x - mean
    q = (c * c).sum(1, keepdims=True)
    var = q / (n if mut == "biased_std" else n - 1)
    den = np.sqrt(var + EPS) if mut == "eps_inside" else np.sqrt(var) + EPS
    s = np.sqrt(var)
    inv = 1.0 / den
    y = g * c * inv + b
    e_mean = (L + 1) * U * np.abs(x).sum(1, keepdims=True) / n
    e_c = e_mean + U * np.abs(c)
    e_q = 2.0 * (np.abs(c) * e_c).sum(1, keepdims=True) + (L + 2) * U * q
    e_s = s * (e_q / (2.0 * q) + 2.0 * U)
    e_inv = inv * ((e_s + U * den) / den + U)
    e_y = np.abs(g) * (e_c * inv + np.abs(c) * e_inv) + 3.0 * U * np.abs(g * c * inv) + U * np.abs(b)
    return {"y": (y, e_y), "mean": (mean[:, 0], e_mean[:, 0]), "inv": (inv[:, 0], e_inv[:, 0])}


def layer_norm_f32(x, gain, bias, order):
    """The same operation in fp32 numpy, its two sums in the given order -> y, mean, inv (fp32)."""
    f = np.float32
    x, g, b = (np.asarray(a, dtype=f) for a in (x, gain, bias))
    n = x.shape[1]
    mean = (sum32(x, order) / f(n))[:, None]
    c = x - mean
    s = np.sqrt(sum32(c * c, order) / f(n - 1))
    inv = (f(1.0) / (s + f(1e-6)))[:, None]
    return g * c * inv + b, mean[:, 0], inv[:, 0]


LN_MUTATIONS = ("biased_std", "eps_inside")          # both apply to every case (every case has the row of std 1e-3)


# ======================================================================================================================
# attention: what the two kinds share
def head_attention(q, k, v, factor, d_scale=None, want_f32=None):
    """One head in float64.  q [nq, d], k, v [len, d], factor [nq, len] = what dropout multiplies P by (0, 1 or 1 / (1 - p)).
    -> O, E_O, P, E_P, Pd (module docstring); d_scale: the head width the scale is taken from (a mutation; default d)."""
    d = q.shape[1]
    n = k.shape[0]
    scale = 1.0 / math.sqrt(d_scale or d)
    S = (q @ k.T) * scale
    e_s = (d + 5) * U * (np.abs(q) @ np.abs(k).T) * scale
    mx = S.max(1, keepdims=True)
    eta = e_s + U * np.abs(S - mx) + 2.0 * U
    e = np.exp(S - mx)
    P = e / e.sum(1, keepdims=True)
    e_p = P * (eta + (P * eta).sum(1, keepdims=True) + 10.0 * U)
    Pd = P * factor
    e_pd = factor * (e_p + U * P)
    O = Pd @ v
    e_o = e_pd @ np.abs(v) + (n + 2) * U * (Pd @ np.abs(v))
    return O, e_o, P, e_p, Pd


def head_attention_f32(q, k, v, factor, order):
    """The same in fp32 numpy (products rounded, every sum in the given order) -> O, P, Pd (fp32)."""
    f = np.float32
    q, k, v, factor = (np.asarray(a, dtype=f) for a in (q, k, v, factor))
    d = q.shape[1]
    scale = f(1.0) / np.sqrt(f(d))
    S = sum32(q[:, None, :] * k[None, :, :], order) * scale
    e = np.exp(S - S.max(1, keepdims=True))
    P = e / sum32(e, order)[:, None]
    Pd = P * factor
    O = sum32(Pd[:, None, :] * v.T[None, :, :], order)
    return O, P, Pd


def drop_factor(n, mode, keep, p, idx0, scale=None):
    """What DropP::apply multiplies element i of a draw of n elements by: 1 in front of idx0 and without dropout, else keep[i - idx0] / (1 - p)
    (scale: the keep factor, default the library's fp32 one)."""
    fac = np.ones(n)
    if mode:
        fac[idx0:] = np.asarray(keep[:n - idx0], dtype=np.float64) * (scale or drop_scale(p))
    return fac


def offsets(counts, n_img, R):
    """First packed row of every image and the total (fixed region sets: img * R)."""
    lens = [R] * n_img if counts is None else list(counts)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    return lens, off


ATT_P = 0.1            # the drop probability of both attention draws (AoA_Model.py: dropout 0.1 on the attention weights)
RNG_REF_ATT, RNG_ATT = 11, 21          # AoaRngStream (aoa_impl.h)
SEED = 0x1234ABCD5678EF01


# ======================================================================================================================
# refiner self-attention: mha_self_kernel (route 1) and mha_self_mfma_kernel (route 2)
SaCase = collections.namedtuple("SaCase", "name n_img R Hd NH counts qc routes idx0 purpose")


def aoa_pitch(n):
    n4 = (n + 3) // 4
    if n4 % 2 == 0:
        n4 += 1
    return 4 * n4


def self_lds(R, d, qc):
    """mha_self_kernel's dynamic LDS in bytes, written out from aoa_self_lds (aoa_impl.h)."""
    ld, lp, R4, q4 = aoa_pitch(d), aoa_pitch(R), (R + 3) & ~3, (qc + 3) & ~3
    return 4 * (2 * R4 * ld + q4 * ld + q4 * lp)


def self_qc(R, d):
    if self_lds(R, d, R) <= LDS_BUDGET:
        return R
    qc = R & ~3
    while qc >= 4 and self_lds(R, d, qc) > LDS_BUDGET:
        qc -= 4
    return qc if qc >= 4 else 0


def self_route(R, Hd, NH, mfma=True):
    return 2 if mfma and R <= 64 and (Hd // NH) % 64 == 0 else 1


def sa_chunks(nrow, qc):
    """Query rows of every pass of mha_self_kernel's q0 loop."""
    return [min(qc, nrow - q0) for q0 in range(0, nrow, qc)]


def _sa(name, n_img, R, d, counts=None, qc=0, routes=(1,), idx0=0, NH=2, **purpose):
    return SaCase(name, n_img, R, d * NH, NH, counts, qc, tuple(routes), idx0, purpose)


# purpose keys (each recomputed by test_cpu_aoa_kernels.py):
#   pitch        LDS row pitch of the head tiles (aoa_pitch(d))        len_mod4   count % 4 of the images, as a set
#   chunks       query rows per pass of image 0                         lds_side   side of the 48 KB opt-in of the route-1 launch
#   route0       what route 0 takes                                     tiles      16-row tiles of route 2 (nt of the largest image)
#   second_key   some image has more than 64 keys (the second key per lane of the softmax)
SA_CASES = [
    # route 1: head widths whose pitch is d (4), d + 4 (8, 56); region counts around a wave and its second key; every count % 4
    _sa("w4_r5", 2, 5, 4, pitch=4, len_mod4={1}, chunks=[5], route0=1),
    _sa("w8_r1", 2, 1, 8, pitch=12, len_mod4={1}, chunks=[1], route0=1),
    _sa("w56_r36", 2, 36, 56, pitch=60, len_mod4={0}, chunks=[36], route0=1),
    _sa("w8_r49", 2, 49, 8, len_mod4={1}, chunks=[49], route0=1),
    _sa("w8_r64", 2, 64, 8, len_mod4={0}, chunks=[64], second_key=False, route0=1),
    _sa("w8_r65", 2, 65, 8, len_mod4={1}, chunks=[65], second_key=True, route0=1),
    _sa("w8_r128", 2, 128, 8, len_mod4={0}, chunks=[128], second_key=True, route0=1),
    _sa("w8_counts_mod4", 4, 36, 8, counts=[8, 5, 6, 7], len_mod4={0, 1, 2, 3}, chunks=[8], route0=1),
    _sa("w8_counts_r_1_17", 3, 36, 8, counts=[36, 1, 17], len_mod4={0, 1}, chunks=[36], route0=1),
    _sa("w8_counts_128_1_17", 3, 128, 8, counts=[128, 1, 17], len_mod4={0, 1}, chunks=[128], second_key=True, route0=1),
    # forced query chunks: the dropout index of a chunk is (q0 + q); the last chunk holds 4, 5 and 1 rows
    _sa("qc4_r36", 2, 36, 8, qc=4, chunks=[4] * 9, route0=1),
    _sa("qc8_count13", 2, 36, 8, counts=[13, 36], qc=8, chunks=[8, 5], route0=1),
    _sa("qc8_count9", 2, 36, 8, counts=[9, 20], qc=8, chunks=[8, 1], route0=1),
    _sa("qc64_r128", 2, 128, 8, qc=64, chunks=[64, 64], second_key=True, route0=1),
    # above the 48 KB opt-in, and the library's own chunking (K and V of 128 x 128 take 133 KB: the queries go through in chunks)
    _sa("lds_r100_w64", 2, 100, 64, lds_side=1, chunks=[100], second_key=True, route0=1),
    _sa("auto_chunk_r128_w64", 2, 128, 64, lds_side=1, chunks=[112, 16], second_key=True, route0=1),
    _sa("auto_chunk_r128_w128", 2, 128, 128, lds_side=1, chunks=[20] * 6 + [8], second_key=True, route0=1),
    # the evaluation-mode half of a paired pass: image 0 in front of idx0 passes unchanged
    _sa("pair_r36", 2, 36, 8, idx0=2 * 36 * 36, route0=1),
    # route 2 (every shape also on route 1): tile edges 16 / 17 / 64, one region, counts 1 beside 64
    _sa("m64_r1", 2, 1, 64, routes=(1, 2, 0), tiles=1, route0=2),
    _sa("m64_r5", 2, 5, 64, routes=(1, 2, 0), tiles=1, route0=2),
    _sa("m64_r16", 2, 16, 64, routes=(1, 2, 0), tiles=1, route0=2),
    _sa("m64_r17", 2, 17, 64, routes=(1, 2, 0), tiles=2, route0=2),
    _sa("m64_r36", 2, 36, 64, routes=(1, 2, 0), tiles=3, route0=2),
    _sa("m128_r49", 2, 49, 128, routes=(1, 2, 0), tiles=4, route0=2, lds_side=1),
    _sa("m128_r64", 2, 64, 128, routes=(1, 2, 0), tiles=4, route0=2, lds_side=1),
    _sa("m64_counts_36_5_17", 3, 36, 64, counts=[36, 5, 17], routes=(1, 2, 0), tiles=3, route0=2),
    _sa("m64_counts_1", 1, 36, 64, counts=[1], routes=(1, 2, 0), tiles=1, route0=2),
    _sa("m128_counts_64_16_33", 3, 64, 128, counts=[64, 16, 33], routes=(1, 2, 0), tiles=4, route0=2, lds_side=1),
    _sa("m64_pair_r36", 2, 36, 64, routes=(1, 2, 0), idx0=2 * 36 * 36, tiles=3, route0=2),
    # beside route 2's conditions: 65 regions, heads of 48 columns -- route 0 takes mha_self_kernel
    _sa("m64_r65", 2, 65, 64, routes=(1, 0), route0=1, second_key=True),
    _sa("w48_r36", 2, 36, 48, routes=(1, 0), route0=1),
]
SA_BY_NAME = {c.name: c for c in SA_CASES}
# refused on the host: (route, R, Hd, NH, qc) -- route 2 above 64 regions and at heads of 48 columns, chunks that are no multiple of 4 /
# above R, more than 128 regions, heads of 6 columns, no route 3
SA_REFUSED = [(2, 65, 128, 2, 0), (2, 36, 96, 2, 0), (1, 36, 16, 2, 6), (1, 36, 16, 2, 40), (1, 129, 16, 2, 0), (1, 36, 12, 2, 0), (3, 36, 16, 2, 0)]


def sa_inputs(c):
    """qkv [region rows, 3 Hd] fp32 (packed rows with counts).  Image i's keys are scaled by 1 + i / 2 so that no two images look alike."""
    lens, off = offsets(c.counts, c.n_img, c.R)
    rs = seeded("sa " + c.name)
    qkv = rs.standard_normal((off[-1], 3 * c.Hd))
    for i in range(c.n_img):
        qkv[off[i]:off[i + 1], c.Hd:2 * c.Hd] *= 1.0 + 0.5 * i
    return qkv.astype(np.float32)


def sa_draws(c):
    """Elements of the attention draw: [n_img, NH, R, R] in the padded strides."""
    return c.n_img * c.NH * c.R * c.R


def sa_keep(c):
    """The explicit keep flags of mode 1 (uint8, the elements behind idx0)."""
    return (seeded("keep " + c.name).rand(sa_draws(c) - c.idx0) >= ATT_P).astype(np.uint8)


SA_MUTATIONS = ("key_behind_count", "last_key_dropped", "drop_index_local_q", "drop_stride_len", "v_neighbour_head", "scale_wrong_d")


def sa_mutation_applies(c, mut, mode, qc):
    """Which cases a wrong reference must fall outside the bound on."""
    lens, _ = offsets(c.counts, c.n_img, c.R)
    if mut == "key_behind_count":          # needs a key behind the count inside the buffer: an image that is not the last, with counts
        return c.counts is not None and c.n_img >= 2
    if mut == "last_key_dropped":
        return max(lens) >= 2
    if mut == "drop_index_local_q":        # needs dropout and a second chunk
        return mode != 0 and any(qc < (n if c.counts is not None else c.R) for n in lens) and max(lens) >= 2
    if mut == "drop_stride_len":           # needs dropout and an image with fewer than R regions and a second query row
        return mode != 0 and any(1 < n < c.R for n in lens)
    return mut in ("v_neighbour_head", "scale_wrong_d") and (mut != "scale_wrong_d" or max(lens) >= 2)


def self_attn_ref(c, qkv, mode=0, keep=None, qc=None, mut=None, scale=None):
    """o [region rows, Hd] in float64 and its bound.  qc only matters to the mutation 'drop_index_local_q'."""
    lens, off = offsets(c.counts, c.n_img, c.R)
    R, Hd, NH, d = c.R, c.Hd, c.NH, c.Hd // c.NH
    x = np.asarray(qkv, dtype=np.float64)
    fac = drop_factor(sa_draws(c), mode, keep, ATT_P, c.idx0, scale)
    o, eo = np.zeros((off[-1], Hd)), np.zeros((off[-1], Hd))
    for img in range(c.n_img):
        n = lens[img]
        nrow = n if c.counts is not None else R
        r0 = off[img]
        nk = n
        if mut == "key_behind_count" and r0 + n < off[-1]:
            nk = n + 1
        if mut == "last_key_dropped" and n >= 2:
            nk = n - 1
        for h in range(NH):
            hv = (h + 1) % NH if mut == "v_neighbour_head" else h
            q = x[r0:r0 + nrow, h * d:(h + 1) * d]
            k = x[r0:r0 + nk, Hd + h * d:Hd + (h + 1) * d]
            v = x[r0:r0 + nk, 2 * Hd + hv * d:2 * Hd + (hv + 1) * d]
            qi = np.arange(nrow)
            if mut == "drop_index_local_q":
                qi = qi % qc
            stride = n if mut == "drop_stride_len" else R
            idx = np.minimum(((img * NH + h) * R + qi)[:, None] * stride + np.arange(nk)[None, :], len(fac) - 1)
            O, e_o = head_attention(q, k, v, fac[idx], d_scale=Hd if mut == "scale_wrong_d" else None)[:2]
            o[r0:r0 + nrow, h * d:(h + 1) * d] = O
            eo[r0:r0 + nrow, h * d:(h + 1) * d] = e_o
    return o, eo


def self_attn_f32(c, qkv, mode, keep, order):
    lens, off = offsets(c.counts, c.n_img, c.R)
    R, Hd, NH, d = c.R, c.Hd, c.NH, c.Hd // c.NH
    fac = drop_factor(sa_draws(c), mode, keep, ATT_P, c.idx0)
    o = np.zeros((off[-1], Hd), np.float32)
    for img in range(c.n_img):
        n, r0 = lens[img], off[img]
        nrow = n if c.counts is not None else R
        for h in range(NH):
            idx = ((img * NH + h) * R + np.arange(nrow))[:, None] * R + np.arange(n)[None, :]
            o[r0:r0 + nrow, h * d:(h + 1) * d] = head_attention_f32(qkv[r0:r0 + nrow, h * d:(h + 1) * d], qkv[r0:r0 + n, Hd + h * d:Hd + (h + 1) * d],
                                                                    qkv[r0:r0 + n, 2 * Hd + h * d:2 * Hd + (h + 1) * d], fac[idx], order)[0]
    return o


# ======================================================================================================================
# decoder attention: aoa_dec_attn_kernel
DaCase = collections.namedtuple("DaCase", "name rows n_img R Hd NH counts img_of_row qns p_out live idx0 purpose")


def dec_lds(R, d):
    """aoa_dec_attn_kernel's dynamic LDS in bytes, written out from aoa_dec_attn_lds (aoa_impl.h)."""
    return 4 * (2 * R * (d + 1) + d + 128 + 4)


def _da(name, R, d, n_img=3, rows=None, counts=None, img_of_row=None, qns=1, p_out=True, live=None, idx0=0, NH=2, **purpose):
    rows = rows if rows is not None else (len(img_of_row) if img_of_row is not None else n_img)
    return DaCase(name, rows, n_img, R, d * NH, NH, counts, img_of_row, qns, p_out, live, idx0, purpose)


# purpose keys: second_key (an attended image has more than 64 regions: waves 1's keys), j_trips (trips of the 256-thread loops over the
# head's columns), lds_side (side of the 48 KB opt-in), unused (images no row attends: their K / V rows are NaN on the device),
# one_key (an attended image has one region: P == 1 exactly)
DA_CASES = [
    _da("r1_w4", 1, 4, second_key=False, j_trips=1, lds_side=-1, one_key=True),
    _da("r36_w8", 36, 8, second_key=False, j_trips=1, lds_side=-1),
    _da("r63_w8", 63, 8, second_key=False, j_trips=1),
    _da("r64_w8", 64, 8, second_key=False, j_trips=1),
    _da("r65_w8", 65, 8, second_key=True, j_trips=1),
    _da("r128_w8", 128, 8, second_key=True, j_trips=1, lds_side=-1),
    _da("r36_w64", 36, 64, second_key=False, j_trips=1, lds_side=-1),
    _da("r36_w260", 36, 260, second_key=False, j_trips=2, lds_side=1),
    _da("r128_w64", 128, 64, second_key=True, j_trips=1, lds_side=1),
    _da("counts_1_r_17", 36, 8, counts=[1, 36, 17], one_key=True),
    _da("counts_128_1_65", 128, 8, counts=[128, 1, 65], second_key=True, one_key=True),
    _da("fan_out", 36, 8, counts=[36, 5, 17], img_of_row=[0, 0, 1, 1, 2, 2]),
    _da("permuted", 36, 8, counts=[7, 36, 20], img_of_row=[2, 0, 1]),
    _da("unused_image", 36, 8, n_img=4, counts=[9, 36, 20, 11], img_of_row=[3, 1, 1], unused=[0, 2]),
    _da("slabs_2", 36, 8, qns=2),
    _da("slabs_5", 36, 64, qns=5, counts=[36, 5, 17], img_of_row=[0, 0, 1, 1, 2, 2]),
    _da("no_p_out", 36, 8, p_out=False),
    _da("live_1", 36, 8, live=1, qns=2),
    _da("live_0", 36, 8, live=0, qns=2),
    _da("idx0", 36, 8, idx0=2 * 36),          # row 0 in front of idx0: its P passes undropped
]
DA_BY_NAME = {c.name: c for c in DA_CASES}
DA_SLAB_PAD = 12                               # floats of NaN between two slabs of the query projection
# refused on the host: (R, Hd, NH, qns, rows, n_img) -- K and V of 128 x 260 above the LDS budget, 129 regions, heads of 6 columns, no slab,
# more rows than images without img_of_row
DA_REFUSED = [(128, 520, 2, 1, 3, 3), (129, 16, 2, 1, 3, 3), (36, 12, 2, 1, 3, 3), (36, 16, 2, 0, 3, 3), (36, 16, 2, 1, 4, 3)]


def da_inputs(c):
    """slabs [qns, rows, Hd], q_bias [Hd], Kd, Vd [region rows, Hd] (fp32).  The slabs sum (with the bias) to a query of unit scale."""
    lens, off = offsets(c.counts, c.n_img, c.R)
    rs = seeded("da " + c.name)
    slabs = (rs.standard_normal((c.qns, c.rows, c.Hd)) / math.sqrt(c.qns)).astype(np.float32)
    bias = (0.1 * rs.standard_normal(c.Hd)).astype(np.float32)
    Kd = rs.standard_normal((off[-1], c.Hd)).astype(np.float32)
    Vd = rs.standard_normal((off[-1], c.Hd)).astype(np.float32)
    return slabs, bias, Kd, Vd


def da_query(c, slabs, bias):
    """The query the kernel works with, in ITS arithmetic: the only slab as it is (qns == 1: the bias is in it), else slab 0 + slab 1 + ...
    + bias in fp32, in that order (what Qp_store must hold bit for bit)."""
    q = slabs[0].copy()
    if c.qns > 1:
        for z in range(1, c.qns):
            q = q + slabs[z]
        q = q + bias[None, :]
    return q.astype(np.float32)


def da_draws(c):
    return c.rows * c.NH * c.R


def da_keep(c):
    return (seeded("keep " + c.name).rand(da_draws(c) - c.idx0) >= ATT_P).astype(np.uint8)


def da_images(c):
    return list(range(c.rows)) if c.img_of_row is None else list(c.img_of_row)


DA_MUTATIONS = ("key_behind_count", "last_key_dropped", "drop_stride_len", "v_neighbour_head", "scale_wrong_d")


def da_mutation_applies(c, mut, mode):
    if c.live == 0:
        return False
    lens, off = offsets(c.counts, c.n_img, c.R)
    att = [lens[i] for i in da_images(c)]
    if mut == "key_behind_count":
        return c.counts is not None and any(off[i] + lens[i] < off[-1] for i in da_images(c))
    if mut in ("last_key_dropped", "scale_wrong_d"):
        return max(att) >= 2
    if mut == "drop_stride_len":           # the draw's row stride: needs dropout, a row behind the first and fewer than R regions there
        return mode != 0 and any(1 < lens[i] < c.R for b, i in enumerate(da_images(c)) if b > 0)
    return True


def dec_attn_ref(c, q32, Kd, Vd, mode=0, keep=None, mut=None, scale=None):
    """-> dict xatt / P / Pd -> (value, bound): xatt [rows, Hd], P, Pd [rows, NH, R] (exact zeros with bound 0 behind the count)."""
    lens, off = offsets(c.counts, c.n_img, c.R)
    R, Hd, NH, d = c.R, c.Hd, c.NH, c.Hd // c.NH
    q64, K, V = (np.asarray(a, dtype=np.float64) for a in (q32, Kd, Vd))
    fac = drop_factor(da_draws(c), mode, keep, ATT_P, c.idx0, scale)
    x, ex = np.zeros((c.rows, Hd)), np.zeros((c.rows, Hd))
    P, eP, Pd, ePd = (np.zeros((c.rows, NH, R)) for _ in range(4))
    for b, img in enumerate(da_images(c)):
        n, r0 = lens[img], off[img]
        nk = n
        if mut == "key_behind_count" and r0 + n < off[-1]:
            nk = n + 1
        if mut == "last_key_dropped" and n >= 2:
            nk = n - 1
        for h in range(NH):
            hv = (h + 1) % NH if mut == "v_neighbour_head" else h
            stride = n if mut == "drop_stride_len" else R
            idx = np.minimum((b * NH + h) * stride + np.arange(nk), len(fac) - 1)        # (a wrong reference may leave the draw)
            O, e_o, p, e_p, pd = head_attention(q64[b:b + 1, h * d:(h + 1) * d], K[r0:r0 + nk, h * d:(h + 1) * d], V[r0:r0 + nk, hv * d:(hv + 1) * d],
                                                fac[idx][None, :], d_scale=Hd if mut == "scale_wrong_d" else None)
            x[b, h * d:(h + 1) * d], ex[b, h * d:(h + 1) * d] = O[0], e_o[0]
            m = min(nk, R)
            P[b, h, :m], eP[b, h, :m] = p[0, :m], e_p[0, :m]
            Pd[b, h, :m], ePd[b, h, :m] = pd[0, :m], (fac[idx] * (e_p[0] + U * p[0]))[:m]
    return {"xatt": (x, ex), "P": (P, eP), "Pd": (Pd, ePd)}


def dec_attn_f32(c, q32, Kd, Vd, mode, keep, order):
    lens, off = offsets(c.counts, c.n_img, c.R)
    R, Hd, NH, d = c.R, c.Hd, c.NH, c.Hd // c.NH
    fac = drop_factor(da_draws(c), mode, keep, ATT_P, c.idx0)
    x = np.zeros((c.rows, Hd), np.float32)
    P, Pd = np.zeros((c.rows, NH, R), np.float32), np.zeros((c.rows, NH, R), np.float32)
    for b, img in enumerate(da_images(c)):
        n, r0 = lens[img], off[img]
        for h in range(NH):
            idx = (b * NH + h) * R + np.arange(n)
            O, p, pd = head_attention_f32(q32[b:b + 1, h * d:(h + 1) * d], Kd[r0:r0 + n, h * d:(h + 1) * d], Vd[r0:r0 + n, h * d:(h + 1) * d],
                                          fac[idx][None, :], order)
            x[b, h * d:(h + 1) * d], P[b, h, :n], Pd[b, h, :n] = O[0], p[0], pd[0]
    return x, P, Pd


# ======================================================================================================================
# aoa_dkv_kernel: d K / d V of the hoisted decoder projections, summed over the (k, t) pairs of every image
#   bound: a sum of S = G T products, k-major and t-minor, in ONE fp32 accumulation (the chunks of tc pairs pass it through dKd / dVd, which
#   rounds nothing): (S + 2) u sum|terms|; and the same bits for every tc.
DkCase = collections.namedtuple("DkCase", "name n_img G T R Hd NH counts tcs purpose")
DKV_LDS = 48 * 1024


def dkv_lds(tc, R, d):
    return 4 * tc * 2 * (R + d)


def dkv_tc(pairs, R, d):
    """The handle's chunk, written out from aoa_dkv_tc (aoa_impl.h): every pair when they fit 48 KB, else as many as do."""
    return min(pairs, DKV_LDS // (4 * 2 * (R + d)))


def dkv_chunks(pairs, tc):
    return [min(tc, pairs - s0) for s0 in range(0, pairs, tc)]


def _dk(name, n_img, G, T, R, d, tcs, counts=None, NH=2, **purpose):
    return DkCase(name, n_img, G, T, R, d * NH, NH, counts, tuple(tcs), purpose)


# purpose: lib_chunks = the passes of the handle's own rule (tc = 0)
DK_CASES = [
    _dk("g1_t1", 2, 1, 1, 36, 8, (0, 1), lib_chunks=[1]),
    _dk("g1_t7", 2, 1, 7, 36, 8, (0, 1, 4, 7), lib_chunks=[7]),
    _dk("g3_t5", 2, 3, 5, 36, 8, (0, 1, 4, 15), lib_chunks=[15]),                    # 4 is no divisor of 15: a last pass of 3 pairs
    _dk("g3_t5_counts", 3, 3, 5, 36, 8, (0, 1, 4, 15), counts=[36, 5, 17], lib_chunks=[15]),
    _dk("g2_t5_w64", 2, 2, 5, 36, 64, (0, 3), lib_chunks=[10]),
    _dk("lib_chunked", 2, 3, 7, 128, 260, (0, 1, 4), counts=[128, 65], lib_chunks=[15, 6]),     # the handle's own rule chunks: 21 pairs, 15 fit
]
DK_BY_NAME = {c.name: c for c in DK_CASES}
# refused on the host: (n_img, B, T, tc, R, Hd, NH, G) -- rows that are not the images' rows (more and fewer), a chunk above the pairs,
# a chunk above 48 KB of LDS, 129 regions, no step
DK_REFUSED = [(2, 7, 5, 0, 36, 16, 2, 3), (2, 5, 5, 0, 36, 16, 2, 3), (2, 6, 5, 16, 36, 16, 2, 3), (2, 6, 7, 21, 128, 520, 2, 3),
              (2, 6, 5, 0, 129, 16, 2, 3), (2, 6, 0, 0, 36, 16, 2, 3)]


def dk_inputs(c):
    """dS, Pd [T, B, NH, R], Qp, dx [T, B, Hd] (fp32; B = n_img G).  Pd has exact zeros (dropped weights) at a tenth of its entries."""
    rs = seeded("dk " + c.name)
    B = c.n_img * c.G
    dS = rs.standard_normal((c.T, B, c.NH, c.R)).astype(np.float32)
    Pd = (np.abs(rs.standard_normal((c.T, B, c.NH, c.R))) * (rs.rand(c.T, B, c.NH, c.R) >= 0.1)).astype(np.float32)
    Qp = rs.standard_normal((c.T, B, c.Hd)).astype(np.float32)
    dx = rs.standard_normal((c.T, B, c.Hd)).astype(np.float32)
    return dS, Pd, Qp, dx


def _dk_terms(c, w, x, img):
    """[pairs, len-independent R, Hd] products of image img in the kernel's pair order (k-major, t-minor)."""
    d = c.Hd // c.NH
    rows = [img * c.G + k for k in range(c.G)]
    wv = np.stack([w[t, r] for r in rows for t in range(c.T)])            # [pairs, NH, R]
    xv = np.stack([x[t, r] for r in rows for t in range(c.T)]).reshape(-1, c.NH, d)      # [pairs, NH, d]
    return (wv[:, :, :, None] * xv[:, :, None, :]).transpose(0, 2, 1, 3).reshape(len(wv), c.R, c.Hd)


def dkv_ref(c, dS, Pd, Qp, dx, skip=None):
    """-> (dKd, bound), (dVd, bound), packed region rows [total, Hd].  skip: the index of one (k, t) pair left out (a wrong reference)."""
    lens, off = offsets(c.counts, c.n_img, c.R)
    S = c.G * c.T
    out = []
    for w, x in ((dS, Qp), (Pd, dx)):
        val, mag = np.zeros((off[-1], c.Hd)), np.zeros((off[-1], c.Hd))
        for img in range(c.n_img):
            t = _dk_terms(c, w.astype(np.float64), x.astype(np.float64), img)
            if skip is not None:
                t = np.delete(t, skip, axis=0)
            val[off[img]:off[img + 1]] = t.sum(0)[:lens[img]]
            mag[off[img]:off[img + 1]] = np.abs(t).sum(0)[:lens[img]]
        out.append((val, (S + 2) * U * mag))
    return out


def dkv_f32(c, dS, Pd, Qp, dx, order):
    lens, off = offsets(c.counts, c.n_img, c.R)
    out = []
    for w, x in ((dS, Qp), (Pd, dx)):
        val = np.zeros((off[-1], c.Hd), np.float32)
        for img in range(c.n_img):
            val[off[img]:off[img + 1]] = sum32(np.moveaxis(_dk_terms(c, w, x, img), 0, -1), order)[:lens[img]]
        out.append(val)
    return out


# ======================================================================================================================
# aoa_dec_attn_bwd_kernel: the backward of the decoder attention of one step, on the forward pass's P and Pd
#   E_dx   = ns u sum_z |slab_z|                                     ns - 1 additions in slab order (+ 1)
#   E_dPd  = sum_j E_dx |v_j| + (d + 2) u sum_j |dx_j v_j|           d additions
#   E_dP   = f (E_dPd + u |dPd|)                                     f = 0 or keep_scale: one product
#   E_dot  = sum_r P_r E_dP_r + 10 u sum_r |P_r dP_r|                the products, <= 7 additions on a path of the tree (+ 2)
#   E_dS   = (P (E_dP + E_dot + u |dP - dot|) + 4 u |P (dP - dot)|) / sqrt(d)    the subtraction; product, sqrt, division (+ 1)
#   E_dQp  = sum_r E_dS_r |k_r| + (len + 2) u sum_r |dS_r k_r|       len additions
# dx_out is the fp32 slab sum in slab order, bit for bit (db_dx).
DbCase = collections.namedtuple("DbCase", "name fwd ns drop")
DB_CASES = [DbCase("%s_ns%d_%s" % (f, ns, "drop" if dr else "nodrop"), f, ns, dr) for f, ns, dr in (
    ("r1_w4", 1, False), ("r36_w8", 3, True), ("r63_w8", 1, True), ("r64_w8", 3, False), ("r65_w8", 1, True), ("r128_w8", 3, True),
    ("r36_w64", 1, True), ("r36_w260", 1, True), ("r128_w64", 1, True), ("counts_1_r_17", 3, True), ("counts_128_1_65", 3, True),
    ("fan_out", 1, True), ("permuted", 3, False), ("unused_image", 1, True), ("live_1", 1, True), ("live_0", 1, True))]
DB_MUTATIONS = ("key_behind_count", "last_key_dropped", "v_neighbour_head", "scale_wrong_d", "keep_scale_forgotten")
# refused on the host: (R, Hd, NH, ns, rows, n_img, keep_scale)
DB_REFUSED = [(128, 520, 2, 1, 3, 3, 1.0), (129, 16, 2, 1, 3, 3, 1.0), (36, 12, 2, 1, 3, 3, 1.0), (36, 16, 2, 0, 3, 3, 1.0), (36, 16, 2, 1, 4, 3, 1.0),
              (36, 16, 2, 1, 3, 3, 0.5)]


def db_lds(R, d):
    """aoa_dec_attn_bwd_kernel's dynamic LDS in bytes, written out from aoa_dec_attn_bwd_lds (aoa_impl.h)."""
    return 4 * (2 * R * (d + 1) + 2 * d + 128 + 4)


def db_keep_scale(b):
    return drop_scale(ATT_P) if b.drop else 1.0


def db_inputs(b):
    """The forward case's q, Kd, Vd; P and Pd of its forward pass rounded to fp32 (Pd with the explicit keep flags when the case drops);
    dxq [ns, rows, 2 Hd] whose columns [Hd, 2 Hd) the kernel must not read (NaN on the device)."""
    c = DA_BY_NAME[b.fwd]
    slabs, bias, Kd, Vd = da_inputs(c)
    q = da_query(c, slabs, bias)
    fwd = dec_attn_ref(c, q, Kd, Vd, 1 if b.drop else 0, da_keep(c))
    dxq = (seeded("db " + b.name).standard_normal((b.ns, c.rows, 2 * c.Hd)) / math.sqrt(b.ns)).astype(np.float32)
    return c, q, Kd, Vd, fwd["P"][0].astype(np.float32), fwd["Pd"][0].astype(np.float32), dxq


def db_dx(c, dxq):
    """dx in the kernel's arithmetic: columns [0, Hd) of the slabs added in slab order in fp32."""
    dx = dxq[0][:, :c.Hd].copy()
    for z in range(1, len(dxq)):
        dx = dx + dxq[z][:, :c.Hd]
    return dx.astype(np.float32)


def db_mutation_applies(b, mut):
    c = DA_BY_NAME[b.fwd]
    if c.live == 0:
        return False
    lens, off = offsets(c.counts, c.n_img, c.R)
    att = [lens[i] for i in da_images(c)]
    if mut == "key_behind_count":
        return c.counts is not None and any(off[i] + lens[i] < off[-1] and lens[i] < c.R for i in da_images(c))
    if mut == "keep_scale_forgotten":
        return b.drop and max(att) >= 2
    return max(att) >= 2          # (one key: P = 1 and dS = 0 whatever the values)


def dec_attn_bwd_ref(c, q, Kd, Vd, P, Pd, dxq, keep_scale, mut=None):
    """-> dict dQp / dS / dx -> (value, bound).  P, Pd [rows, NH, R] as the forward pass left them (any float type)."""
    lens, off = offsets(c.counts, c.n_img, c.R)
    R, Hd, NH, d = c.R, c.Hd, c.NH, c.Hd // c.NH
    q, K, V, P, Pd, sl = (np.asarray(a, dtype=np.float64) for a in (q, Kd, Vd, P, Pd, dxq))
    ns = sl.shape[0]
    dx, e_dx = sl[:, :, :Hd].sum(0), ns * U * np.abs(sl[:, :, :Hd]).sum(0)
    rs = 1.0 / math.sqrt(Hd if mut == "scale_wrong_d" else d)
    ks = 1.0 if mut == "keep_scale_forgotten" else keep_scale
    dQ, eQ = np.zeros((c.rows, Hd)), np.zeros((c.rows, Hd))
    dS, eS = np.zeros((c.rows, NH, R)), np.zeros((c.rows, NH, R))
    for b, img in enumerate(da_images(c)):
        n, r0 = lens[img], off[img]
        nk = n
        if mut == "key_behind_count" and r0 + n < off[-1] and n < R:
            nk = n + 1
        if mut == "last_key_dropped" and n >= 2:
            nk = n - 1
        for h in range(NH):
            hv = (h + 1) % NH if mut == "v_neighbour_head" else h
            k, v = K[r0:r0 + nk, h * d:(h + 1) * d], V[r0:r0 + nk, hv * d:(hv + 1) * d]
            p, f = P[b, h, :nk].copy(), (Pd[b, h, :nk] != 0) * ks
            if nk > n:          # the wrong reference lets the key behind the count in with the weight of its neighbour
                p[n], f[n] = p[n - 1], ks
            g, eg = dx[b, h * d:(h + 1) * d], e_dx[b, h * d:(h + 1) * d]
            dPd = v @ g
            e_dPd = np.abs(v) @ eg + (d + 2) * U * (np.abs(v) @ np.abs(g))
            dP, e_dP = f * dPd, f * (e_dPd + U * np.abs(dPd))
            dot = (p * dP).sum()
            e_dot = (p * e_dP).sum() + 10 * U * np.abs(p * dP).sum()
            s = p * (dP - dot) * rs
            e_s = (p * (e_dP + e_dot + U * np.abs(dP - dot)) + 4 * U * np.abs(p * (dP - dot))) * rs
            dS[b, h, :nk if nk <= R else R], eS[b, h, :nk if nk <= R else R] = s[:R], e_s[:R]
            dQ[b, h * d:(h + 1) * d] = s @ k
            eQ[b, h * d:(h + 1) * d] = e_s @ np.abs(k) + (nk + 2) * U * (np.abs(s) @ np.abs(k))
    return {"dQp": (dQ, eQ), "dS": (dS, eS), "dx": (dx, e_dx)}


def dec_attn_bwd_f32(c, q, Kd, Vd, P, Pd, dxq, keep_scale, order):
    f = np.float32
    lens, off = offsets(c.counts, c.n_img, c.R)
    R, Hd, NH, d = c.R, c.Hd, c.NH, c.Hd // c.NH
    dx = db_dx(c, dxq)
    rsd = np.sqrt(f(d))
    dQ, dS = np.zeros((c.rows, Hd), f), np.zeros((c.rows, NH, R), f)
    for b, img in enumerate(da_images(c)):
        n, r0 = lens[img], off[img]
        for h in range(NH):
            k, v = Kd[r0:r0 + n, h * d:(h + 1) * d], Vd[r0:r0 + n, h * d:(h + 1) * d]
            p = P[b, h, :n].astype(f)
            dPd = sum32(v * dx[b, h * d:(h + 1) * d][None, :], order)
            dP = np.where(Pd[b, h, :n] != 0, dPd * f(keep_scale), f(0))
            dot = sum32(p * dP, order)
            s = p * (dP - dot) / rsd
            dS[b, h, :n] = s
            dQ[b, h * d:(h + 1) * d] = sum32((s[:, None] * k).T, order)
    return dQ, dS, dx


# ======================================================================================================================
# LayerNorm backward: aoa_ln_bwd_kernel (form 0: the forward pass's stats, two slab sets) and aoa_ln_bwd_dense_kernel (form 1: stats
# recomputed from x; dq_a slabs, dense dq_b, residual res, prod out).  One workgroup per row, a thread's 4 columns per 1024 in registers.
#   L = 4 ceil(n / 1024) + 12: a thread's additions, 6 shuffle levels, 3 across the waves (+ 3).  With xc = x - mean, dy = dq g:
#   E_dq   = (slabs + 1) u sum|pieces|                               the slab sums and the sum of the two sets
#   form 1: E_mean, E_xc, E_q, E_s, E_inv as LayerNorm forward (with this L);  form 0: the stats are inputs, E_xc = u |xc|, E_inv = 0,
#           std = 1 / inv - eps in fp32: E_s = 2 u / inv (the division and the subtraction)
#   E_dy   = |g| E_dq + u |dy|
#   E_s1   = sum E_dy + (L + 2) u sum|dy|;   E_s2 = sum(E_dy |xc| + |dy| E_xc) + (L + 2) u sum|dy xc|
#   kx = -inv^2 s2 / (s (n - 1)):  E_kx = |kx| (2 E_inv / inv + E_s / s + 6 u) + inv^2 E_s2 / (s (n - 1))
#   mdx = inv s1 / n:              E_mdx = |mdx| (E_inv / inv + 3 u) + inv E_s1 / n
#   E_dx   = E_dy inv + |dy| E_inv + E_kx |xc| + |kx| E_xc + E_mdx + 4 u (|res| + |dy inv| + |kx xc| + |mdx|)
#   E_prod = (E_dq |xc| + |dq| E_xc) inv + |dq xc| E_inv + 3 u |prod|
LbCase = collections.namedtuple("LbCase", "name form n rows ns_a ns_b has_a has_b has_res live")
LB_N = (4, 1020, 1024, 1028, 4096)


def _lb_cases():
    out = []
    for i, n in enumerate(LB_N):
        out.append(LbCase("dense_n%d" % n, 1, n, 3, 3 if i % 2 else 1, 0, True, True, True, None))
        out.append(LbCase("stats_n%d" % n, 0, n, 3, 1 if i % 2 else 3, 2 if i % 2 else 1, True, True, False, None))
    out.append(LbCase("dense_no_dq_a", 1, 1028, 3, 0, 0, False, True, True, None))
    out.append(LbCase("dense_no_dq_b", 1, 1028, 3, 3, 0, True, False, True, None))
    out.append(LbCase("dense_no_res", 1, 1028, 3, 1, 0, True, True, False, None))
    out.append(LbCase("stats_live1", 0, 1028, 3, 3, 2, True, True, False, 1))
    out.append(LbCase("stats_live0", 0, 1028, 3, 3, 2, True, True, False, 0))
    return out


LB_CASES = _lb_cases()
LB_SCALES = ((1e-3, 0.0), (1.0, 3.0), (30.0, 0.0))          # (spread, offset) of row r % 3; std 1e-3 is where eps inside the sqrt shows
LB_MUTATIONS = ("biased_std", "eps_inside")
# refused on the host: (form, n, what) -- 4100 and 6 columns, a form that does not exist, form 0 with a residual, form 1 with stats, a base
# 4 bytes off
LB_REFUSED = [(0, 4100, None), (1, 4100, None), (1, 6, None), (2, 8, None), (0, 8, "res"), (1, 8, "stats"), (1, 8, "odd")]


def lb_vectors(n):
    """float4 groups per thread: 1 up to 1024 columns, the multi-vector path above."""
    return (n + 1023) // 1024


def lb_inputs(c):
    """x [rows, n], gain [n] (no entry within 0.25 of 0), dq_a [ns_a, rows, n] or None, dq_b (form 0: [ns_b, rows, 2 n] whose columns [0, n) the kernel does not read;
    form 1: [rows, n]) or None, res [rows, n] or None, stats [rows, 2] (the float64 forward statistics rounded to fp32)."""
    rs = seeded("lb " + c.name)
    x = rs.standard_normal((c.rows, c.n))
    for r in range(c.rows):
        sc, of = LB_SCALES[r % len(LB_SCALES)]
        x[r] = x[r] * sc + of
    x = x.astype(np.float32)
    f = lambda *shape: rs.standard_normal(shape).astype(np.float32)
    gain = f(c.n)
    gain = (gain + np.sign(gain) * np.float32(0.25)).astype(np.float32)
    dq_a = f(c.ns_a, c.rows, c.n) if c.has_a else None
    dq_b = (f(c.ns_b, c.rows, 2 * c.n) if c.form == 0 else f(c.rows, c.n)) if c.has_b else None
    res = f(c.rows, c.n) if c.has_res else None
    x64 = x.astype(np.float64)
    # dq leans on x - mean, so that sum(dy xc) -- the term through which std acts -- does not cancel to nothing by chance
    lean = (0.5 * (x64 - x64.mean(1, keepdims=True)) / x64.std(1, ddof=1, keepdims=True) * np.sign(gain)).astype(np.float32)
    if dq_a is not None:
        dq_a[0] += lean
    elif c.form == 1:
        dq_b += lean
    stats = np.stack([x64.mean(1), 1.0 / (x64.std(1, ddof=1) + EPS)], 1).astype(np.float32)
    return x, gain, dq_a, dq_b, res, stats


def ln_bwd_ref(c, x, gain, dq_a, dq_b, res, stats, mut=None):
    """-> dict dx / dq_tot / prod -> (value, bound).  stats: the (mean, inv) form 0 works with (any float type)."""
    n = c.n
    L = 4 * lb_vectors(n) + 12
    x, g = np.asarray(x, np.float64), np.asarray(gain, np.float64)
    parts = []
    if dq_a is not None:
        parts += list(np.asarray(dq_a, np.float64))
    if dq_b is not None:
        parts += list(np.asarray(dq_b, np.float64)[:, :, n:]) if c.form == 0 else [np.asarray(dq_b, np.float64)]
    dq = np.sum(parts, 0) if parts else np.zeros_like(x)
    e_dq = (len(parts) + 1) * U * np.sum(np.abs(parts), 0) if parts else np.zeros_like(x)
    nm1 = n if mut == "biased_std" else n - 1
    if c.form == 1:
        mean = x.mean(1, keepdims=True)
        xc = x - mean
        q = (xc * xc).sum(1, keepdims=True)
        s = np.sqrt(q / nm1)
        den = np.sqrt(q / nm1 + EPS) if mut == "eps_inside" else s + EPS
        inv = 1.0 / den
        e_mean = (L + 1) * U * np.abs(x).sum(1, keepdims=True) / n
        e_xc = e_mean + U * np.abs(xc)
        e_q = 2.0 * (np.abs(xc) * e_xc).sum(1, keepdims=True) + (L + 2) * U * q
        e_s = s * (e_q / (2.0 * q) + 2.0 * U)
        e_inv = inv * ((e_s + U * den) / den + U)
    else:
        st = np.asarray(stats, np.float64)
        mean, inv = st[:, :1], st[:, 1:2]
        xc = x - mean
        s = 1.0 / inv if mut == "eps_inside" else 1.0 / inv - EPS          # (the wrong reference of form 0: eps left inside the std)
        e_xc, e_inv, e_s = U * np.abs(xc), np.zeros_like(inv), 2.0 * U / inv
    dy = dq * g
    e_dy = np.abs(g) * e_dq + U * np.abs(dy)
    sm = lambda a: a.sum(1, keepdims=True)
    s1, s2 = sm(dy), sm(dy * xc)
    e_s1 = sm(e_dy) + (L + 2) * U * sm(np.abs(dy))
    e_s2 = sm(e_dy * np.abs(xc) + np.abs(dy) * e_xc) + (L + 2) * U * sm(np.abs(dy * xc))
    kx = -inv * inv * s2 / (s * nm1)
    e_kx = np.abs(kx) * (2 * e_inv / inv + e_s / s + 6 * U) + inv * inv * e_s2 / (s * nm1)
    mdx = inv * s1 / n
    e_mdx = np.abs(mdx) * (e_inv / inv + 3 * U) + inv * e_s1 / n
    r = np.zeros_like(x) if res is None else np.asarray(res, np.float64)
    dx = r + dy * inv + kx * xc - mdx
    e_dx = e_dy * inv + np.abs(dy) * e_inv + e_kx * np.abs(xc) + np.abs(kx) * e_xc + e_mdx + 4 * U * (
        np.abs(r) + np.abs(dy * inv) + np.abs(kx * xc) + np.abs(mdx))
    prod = dq * xc * inv
    e_prod = (e_dq * np.abs(xc) + np.abs(dq) * e_xc) * inv + np.abs(dq * xc) * e_inv + 3 * U * np.abs(prod)
    return {"dx": (dx, e_dx), "dq_tot": (dq, e_dq), "prod": (prod, e_prod)}


def ln_bwd_f32(c, x, gain, dq_a, dq_b, res, stats, order):
    f = np.float32
    n = c.n
    dq = np.zeros_like(x)
    if dq_a is not None:
        a = dq_a[0]
        for z in range(1, len(dq_a)):
            a = a + dq_a[z]
        dq = a
    if dq_b is not None:
        if c.form == 0:
            b = dq_b[0][:, n:]
            for z in range(1, len(dq_b)):
                b = b + dq_b[z][:, n:]
        else:
            b = dq_b
        dq = dq + b
    if c.form == 1:
        mean = (sum32(x, order) / f(n))[:, None]
        xc = x - mean
        s = np.sqrt(sum32(xc * xc, order) / f(n - 1))[:, None]
        inv = f(1.0) / (s + f(1e-6))
    else:
        mean, inv = stats[:, :1], stats[:, 1:2]
        xc = x - mean
        s = f(1.0) / inv - f(1e-6)
    dy = dq * gain
    s1, s2 = sum32(dy, order)[:, None], sum32(dy * xc, order)[:, None]
    kx = -inv * inv * s2 / (s * f(n - 1))
    mdx = inv * s1 / f(n)
    dx = (res if res is not None else f(0)) + (dy * inv + kx * xc - mdx)
    return dx.astype(f), dq.astype(f), (dq * xc * inv).astype(f)


# ======================================================================================================================
# mha_self_bwd_kernel: the backward of the refiner self-attention; n = an image's rows (queries = keys)
#   E_S, eta, E_P, E_Pd as attention forward;  dPd = dO V^T: E_dPd = (d + 2) u |dO| |V|^T;  E_dP = f (E_dPd + u |dPd|)
#   dot = sum_k P dP:  E_dot = sum(E_P |dP| + P E_dP) + 10 u sum|P dP|          two products, <= 7 additions on a path (+ 1)
#   dS = P (dP - dot) scale:  E_dS = (E_P |dP - dot| + P (E_dP + E_dot + u |dP - dot|) + 4 u |P (dP - dot)|) scale
#   dQ = dS K, dK = dS^T Q, dV = Pd^T dO:  sum_k E_factor |other| + (n + 2) u sum_k |factor other|     n additions
SbCase = collections.namedtuple("SbCase", "name n_img R Hd NH counts idx0 purpose")


def sb_lds(R, d):
    """mha_self_bwd_kernel's dynamic LDS in bytes, written out from mha_self_bwd_lds_floats (aoa_kernels.h)."""
    return 4 * (3 * R * (d + 1) + 2 * R * (R + 1))


def _sb(name, R, d, n_img=2, counts=None, idx0=0, NH=2, **purpose):
    return SbCase(name, n_img, R, d * NH, NH, counts, idx0, purpose)


SB_CASES = [
    _sb("r1_w8", 1, 8, second_key=False, lds_side=-1),
    _sb("r5_w8", 5, 8, second_key=False, lds_side=-1),
    _sb("r36_w8", 36, 8, second_key=False, lds_side=-1),
    _sb("r65_w8", 65, 8, second_key=True, lds_side=-1),
    _sb("r128_w4", 128, 4, second_key=True, lds_side=1),
    _sb("r36_w64", 36, 64, second_key=False, lds_side=-1),
    _sb("counts_36_5_17", 36, 8, n_img=3, counts=[36, 5, 17], second_key=False),
    _sb("pair_r36", 36, 8, idx0=2 * 36 * 36),
]
SB_BY_NAME = {c.name: c for c in SB_CASES}
SB_REFUSED = [(128, 256, 2), (129, 16, 2), (36, 12, 2)]          # (R, Hd, NH): 128 regions x 128 columns above the LDS budget, ...
SB_MUTATIONS = ("last_key_dropped", "drop_stride_len", "v_neighbour_head", "scale_wrong_d")


def sb_inputs(c):
    """qkv [region rows, 3 Hd] and dO [region rows, Hd] (fp32)."""
    qkv = sa_inputs(c)
    return qkv, seeded("sb " + c.name).standard_normal((qkv.shape[0], c.Hd)).astype(np.float32)


def sb_mutation_applies(c, mut, mode):
    lens, _ = offsets(c.counts, c.n_img, c.R)
    if mut == "drop_stride_len":
        return mode != 0 and any(1 < n < c.R for n in lens)
    return max(lens) >= 2


def self_attn_bwd_ref(c, qkv, dO, mode=0, keep=None, mut=None, scale=None):
    """dqkv [region rows, 3 Hd] = [dQ | dK | dV] in float64 and its bound."""
    lens, off = offsets(c.counts, c.n_img, c.R)
    R, Hd, NH, d = c.R, c.Hd, c.NH, c.Hd // c.NH
    x, g = np.asarray(qkv, np.float64), np.asarray(dO, np.float64)
    fac = drop_factor(sa_draws(c), mode, keep, ATT_P, c.idx0, scale)
    out, eo = np.zeros((off[-1], 3 * Hd)), np.zeros((off[-1], 3 * Hd))
    for img in range(c.n_img):
        n, r0 = lens[img], off[img]
        nk = n - 1 if mut == "last_key_dropped" and n >= 2 else n
        for h in range(NH):
            hv = (h + 1) % NH if mut == "v_neighbour_head" else h
            q, k = x[r0:r0 + n, h * d:(h + 1) * d], x[r0:r0 + nk, Hd + h * d:Hd + (h + 1) * d]
            v, go = x[r0:r0 + nk, 2 * Hd + hv * d:2 * Hd + (hv + 1) * d], g[r0:r0 + n, h * d:(h + 1) * d]
            stride = n if mut == "drop_stride_len" else R
            F = fac[((img * NH + h) * R + np.arange(n))[:, None] * stride + np.arange(nk)[None, :]]
            _, _, P, e_p, Pd = head_attention(q, k, v, F, d_scale=Hd if mut == "scale_wrong_d" else None)
            sc = 1.0 / math.sqrt(Hd if mut == "scale_wrong_d" else d)
            e_pd = F * (e_p + U * P)
            dV = Pd.T @ go
            e_dV = e_pd.T @ np.abs(go) + (n + 2) * U * (Pd.T @ np.abs(go))
            dPd = go @ v.T
            dP = F * dPd
            e_dP = F * ((d + 2) * U * (np.abs(go) @ np.abs(v).T) + U * np.abs(dPd))
            sm = lambda a: a.sum(1, keepdims=True)
            dot = sm(P * dP)
            e_dot = sm(e_p * np.abs(dP) + P * e_dP) + 10 * U * sm(np.abs(P * dP))
            dS = P * (dP - dot) * sc
            e_dS = (e_p * np.abs(dP - dot) + P * (e_dP + e_dot + U * np.abs(dP - dot)) + 4 * U * np.abs(P * (dP - dot))) * sc
            dQ, e_dQ = dS @ k, e_dS @ np.abs(k) + (n + 2) * U * (np.abs(dS) @ np.abs(k))
            dK, e_dK = dS.T @ q, e_dS.T @ np.abs(q) + (n + 2) * U * (np.abs(dS).T @ np.abs(q))
            for w, (val, err, rows) in enumerate(((dQ, e_dQ, n), (dK, e_dK, nk), (dV, e_dV, nk))):
                out[r0:r0 + rows, w * Hd + h * d:w * Hd + (h + 1) * d] = val
                eo[r0:r0 + rows, w * Hd + h * d:w * Hd + (h + 1) * d] = err
    return out, eo


def self_attn_bwd_f32(c, qkv, dO, mode, keep, order):
    f = np.float32
    lens, off = offsets(c.counts, c.n_img, c.R)
    R, Hd, NH, d = c.R, c.Hd, c.NH, c.Hd // c.NH
    fac = drop_factor(sa_draws(c), mode, keep, ATT_P, c.idx0).astype(f)
    out = np.zeros((off[-1], 3 * Hd), f)
    mm = lambda a, b: sum32(a[:, None, :] * b.T[None, :, :], order)          # a @ b in fp32, the sum in the given order
    for img in range(c.n_img):
        n, r0 = lens[img], off[img]
        for h in range(NH):
            q, k, v = (qkv[r0:r0 + n, w * Hd + h * d:w * Hd + (h + 1) * d] for w in range(3))
            go = dO[r0:r0 + n, h * d:(h + 1) * d]
            F = fac[((img * NH + h) * R + np.arange(n))[:, None] * R + np.arange(n)[None, :]]
            _, P, Pd = head_attention_f32(q, k, v, F, order)
            sc = f(1.0) / np.sqrt(f(d))
            dP = F * mm(go, v.T)
            dot = sum32(P * dP, order)[:, None]
            dS = P * (dP - dot) * sc
            for w, val in enumerate((mm(dS, k), mm(dS.T.copy(), q), mm(Pd.T.copy(), go))):
                out[r0:r0 + n, w * Hd + h * d:w * Hd + (h + 1) * d] = val
    return out
