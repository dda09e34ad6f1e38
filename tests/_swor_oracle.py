"""SCST on without-replacement samples (include/icz.h "SCST on without-replacement samples"; csrc/swor_objective.hip) stated in float64
numpy, with per-element error bounds and the case table of tests/test_gpu_swor_step.py.  Plain numpy, not collected by pytest.

Statement (coefs, ref): per image, slots 0..n-1, kappa = G[n - 1], the m = n - 1 slots in front are the samples, f = scores:
  d = phi - kappa,  q = -expm1(-exp(d)),  log q = d - exp(d) / 2 where d < D_SWITCH = -18,  p = exp(phi),  w = exp(phi - log q)
  W = sum w,  Bu = sum w f (ascending slots),  "normalised" c = w / (W - w + p) (f - Bu / W),  "unbiased" c = w (f (1 + w - p) - Bu)
  coef = -c / N (0 in the threshold slot),  N = n_img_global if > 0 else the image count
  loss = sum_rows coef_row sum_t lp[row, t],  lp = x[y] - lse(x),  g[row t, v] = coef_row (1[v == y] - exp(x_v - lse))
The inputs (phi fp32, G, scores, the logits x fp32) are what the device holds; the statement takes them as given and works in float64.

Bounds, counted from the device's operations and never fitted to its output (u = 2^-24, u64 = 2^-53; expf and logf ASSUMED within
E_EXP = 4 ulp as in _token_choice.py, the float64 exp / log / expm1 within E64 = 4 ulp; TINY = 2^-126, an expf that underflows):
  weights (float64):
    rx   = u64 |d| + E64 u64                                  relative, of x = exp(d): the subtraction, then exp
    e_lq = (x e^-x / q) rx + E64 u64 + E64 u64 |log q|        d >= D_SWITCH: expm1 of an argument with relative error rx, then log
         = u64 |d| + x rx / 2 + u64 |log q| + x^2 / 24        d <  D_SWITCH: the subtraction, the product, the sum, the cut series
    rw   = expm1(e_lq + u64 |phi - log q|) + E64 u64          relative, of w;   rp = E64 u64 of p (phi is exact in float64)
    eW   = sum w rw + (m - 1) u64 W;   eBu = sum |w f| (rw + u64) + (m - 1) u64 sum |w f|;   e_base = eBu / W + |base| eW / W + u64 |base|
    normalised: e_den = eW + w rw + p rp + 2 u64 (W + w + p);  c = r (f - base), r = w / den:
                e_c = r (e_base + u64 |f - base|) + |c| (rw + e_den / den + u64) + u64 |c|
    unbiased:   e_t = w rw + p rp + 2 u64 (1 + w + p);  e_s = |f| e_t + u64 |f t| + eBu + u64 |f t - Bu|;  e_c = w e_s + |c| (rw + u64)
    coef: e_c / N + (3 u64 + u) |coef| + 2^-149                (1 / N, two products, the fp32 store)
    stats: W: eW;  base: e_base;  ess = 1 / sum (w / W)^2: ess (2 max_j (rw_j + eW / W + u64) + (m + 3) u64)
  a softmax row of V columns, k = 4 ceil(V / 1024) elements per thread, M its maximum, s = sum exp(x - M):
    e_lse = ((k + 9) (E_EXP + 2) + sum_v p_v (M - x_v)) u + V TINY     the online sum: a path of at most k + 9 steps (k elements, 6 lane
                                                                       and 3 wave combines) of one expf, one product and one addition;
                                                                       the rounded exponent arguments of an element telescope to M - x_v
          + E_EXP u |log s| + u |lse|                                  logf and the final sum
    e_lp  = e_lse + u |lp|;   ep_v = p_v (expm1(e_lse + u |x_v - lse|) + E_EXP u) + TINY
    g:    |coef| (ep + u |1[v = y] - p|) + u |g| + e_coef |1[v = y] - p| + 2^-149
  loss (float64 sums of the fp32 lp and coef):
    per image: sum_j (|coef_j| (sum_t e_lp + T u64 sum_t |lp|) + e_coef_j |s_j|) + (m + 1) u64 sum_j |coef_j s_j|, + u |S| for the fp32 store
    loss: the sum of those + (ceil(images / 256) + 8) u64 sum |S| + u |loss|
"""
import collections
import zlib

import numpy as np

U, U64 = 2.0 ** -24, 2.0 ** -53
E_EXP = E64 = 4
TINY = 2.0 ** -126
D_SWITCH = -18.0
ESTIMATORS = ("normalised", "unbiased")

Case = collections.namedtuple("Case", "name V n n_img T estimator n_glob kappa design")


def _c(name, V, n, n_img, T, estimator="normalised", n_glob=0.0, kappa=-3.0, design=""):
    return Case(name, V, n, n_img, T, estimator, n_glob, kappa, design)


# kappa: the threshold of every image (phi = kappa + d, d spread over [-60, +10] and clipped so that phi <= 0); design words:
# "equal" = equal scores within an image, "zero" = image 0 alone has them: under "normalised" its rows have coefficient 0 and hold NaN.
# The equal scores are powers of two: w f is then exact, Bu / W is f to the bit and c is exactly 0 on the device and here alike (any
# other f leaves a c of rounding size, whose being zero or not the two sides need not agree on).
CASES = [
    _c("v53_n3_1img_t1", 53, 3, 1, 1),                                         # ldl 64, one step, the smallest n
    _c("v53_n3_1img_t1_unbiased", 53, 3, 1, 1, "unbiased"),
    _c("v1000_n5_3img_t7", 1000, 5, 3, 7, kappa=-50.0),                        # phi near -40 and below; rows_t shrinks
    _c("v1000_n5_3img_t7_unbiased", 1000, 5, 3, 7, "unbiased", kappa=-50.0),
    _c("v10102_n8_3img_t7", 10102, 8, 3, 7, kappa=1.5),                        # the benchmark's width, ldl 10 112; a positive threshold
    _c("v10102_n5_1img_t7_unbiased_nglob", 10102, 5, 1, 7, "unbiased", n_glob=4.0),
    _c("v53_n8_7img_t7_big", 53, 8, 7, 7, kappa=-50.0),                        # 49 rows x 7 steps = 343 (b, t) pairs > 256
    _c("v53_n8_7img_t7_big_unbiased", 53, 8, 7, 7, "unbiased"),
    _c("v1000_n3_7img_t1", 1000, 3, 7, 1, n_glob=11.0),
    _c("equal_scores_n5_3img", 53, 5, 3, 7, design="equal"),                   # "normalised" c = 0: nothing is read, all zeros
    _c("equal_scores_unbiased_n5_3img", 53, 5, 3, 7, "unbiased", design="equal"),
    _c("zero_coef_image_n5_3img", 1000, 5, 3, 7, design="zero"),               # NaN in the rows of the zero-coefficient image
    _c("nglob_n8_1img", 1000, 8, 1, 7, n_glob=5.0, kappa=-50.0),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def ldl_of(V):
    """the row stride of a case's logits: V rounded up to 16 floats (64 / 1008 / 10 112 for 53 / 1000 / 10 102)"""
    return (V + 15) & ~15


def sorted_rows(lens_kept, kept):
    """the stable sort by decreasing length of make_batch: kept rows (img n + slot) -> perm"""
    order = sorted(range(len(kept)), key=lambda i: -lens_kept[i])
    return [kept[i] for i in order]


def inputs(c):
    """The device's inputs of a case (numpy): phi fp32 / G / scores [n_img n]; the sorted batch (captions [B, T + 1] with <sta> = 1 in
    front, lengths, perm) and the logits x [T B, ldl] fp32 with NaN in inactive rows, in rows of coefficient exactly 0 and in the pad
    columns"""
    rs = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    n, m, n_img, T, V = c.n, c.n - 1, c.n_img, c.T, c.V
    total, B, ldl = n_img * n, n_img * (c.n - 1), ldl_of(c.V)
    # phi - kappa spread over [-60, +10]: both log q branches, the switch point's neighbourhood and q -> 1
    d = np.linspace(-60.0, 10.0, n_img * m)
    d[:: 3] += rs.rand(d[::3].size)
    if n_img * m >= 4:
        d[1], d[2] = D_SWITCH - 1e-3, D_SWITCH + 1e-3
    d = rs.permutation(d)
    phi = np.zeros(total, dtype=np.float32)
    G = np.zeros(total)
    for i in range(n_img):
        di = np.minimum(d[i * m:(i + 1) * m], -c.kappa - 0.05)      # phi <= -0.05: a log-probability
        phi[i * n:i * n + m] = (c.kappa + di).astype(np.float32)
        phi[i * n + m] = np.float32(c.kappa - 2.0)
        G[i * n:i * n + m] = c.kappa + np.sort(rs.rand(m) * 5.0 + 0.1)[::-1]
        G[i * n + m] = c.kappa
    scores = rs.rand(total) * 3.0
    if c.design == "equal":
        scores = np.repeat(2.0 ** rs.randint(-2, 3, size=n_img), n)
    if c.design == "zero":
        scores[:n] = 2.0
    # lengths: unequal when T > 1 (rows_t shrinks), one row of every length bound
    lens = rs.randint(1, T + 1, size=total)
    lens[0], lens[total - 2] = T, 1 if T > 1 else T
    kept = [r for r in range(total) if r % n != m]
    perm = sorted_rows([int(lens[r]) for r in kept], kept)
    lengths = [int(lens[r]) for r in perm]
    caps = np.zeros((B, T + 1), dtype=np.int64)
    caps[:, 0] = 1
    for b in range(B):
        caps[b, 1:1 + lengths[b]] = rs.randint(0, V, size=lengths[b])
    caps[0, 1] = 0                                   # the targets 0 and V - 1
    caps[B - 1, 1] = V - 1
    coef, _, _ = coefs(phi, G, scores, n, c.estimator, n_of(c))
    x = np.full((T * B, ldl), np.nan, dtype=np.float32)
    live = 0
    for t in range(T):
        for b in range(B):
            if lengths[b] <= t or np.float32(coef[perm[b]]) == 0.0:
                continue
            if live % 5 == 3:                        # one logit 80 above the rest: p underflows to 0 elsewhere
                v = rs.randn(V).astype(np.float32)
                v[rs.randint(0, V)] += 80.0
            elif live % 5 == 4:                      # near uniform
                v = (rs.randn(V) * 1e-3).astype(np.float32)
            else:
                v = (rs.randn(V) * 2.0).astype(np.float32)
            live += 1
            x[t * B + b, :V] = v
    return {"phi": phi, "G": G, "scores": scores, "caps": caps, "lengths": lengths, "perm": np.array(perm, dtype=np.int32), "x": x, "ldl": ldl}


def n_of(c):
    return float(np.float32(c.n_glob)) if c.n_glob else float(c.n_img)


def log_q(d):
    """both branches of log q and the one the statement takes"""
    x = np.exp(d)
    series = d - 0.5 * x
    with np.errstate(divide="ignore"):
        direct = np.log(-np.expm1(-x))
    return np.where(d < D_SWITCH, series, direct), series, direct


def coefs(phi, G, scores, n, estimator, N):
    """float64 statement of the weights -> (coef [n_img n] = -c / N, its bound, stats [n_img, 3] with their bounds [n_img, 3])"""
    total = phi.shape[0]
    n_img, m = total // n, n - 1
    coef, ecoef = np.zeros(total), np.zeros(total)
    stats, estats = np.zeros((n_img, 3)), np.zeros((n_img, 3))
    for i in range(n_img):
        sl = slice(i * n, i * n + m)
        ph, f, kappa = phi[sl].astype(np.float64), scores[sl].astype(np.float64), float(G[i * n + m])
        d = ph - kappa
        x = np.exp(d)
        lq, _, _ = log_q(d)
        rx = U64 * np.abs(d) + E64 * U64
        q = -np.expm1(-x)
        with np.errstate(invalid="ignore", divide="ignore"):
            e_direct = np.where(q > 0, x * np.exp(-x) / q, 1.0) * rx + E64 * U64 + E64 * U64 * np.abs(lq)
        e_series = U64 * np.abs(d) + 0.5 * x * rx + U64 * np.abs(lq) + x * x / 24.0
        e_lq = np.where(d < D_SWITCH, e_series, e_direct)
        p, w = np.exp(ph), np.exp(ph - lq)
        rw = np.expm1(e_lq + U64 * np.abs(ph - lq)) + E64 * U64
        rp = E64 * U64
        W = Bu = 0.0
        for j in range(m):
            W += w[j]
            Bu += w[j] * f[j]
        eW = (w * rw).sum() + (m - 1) * U64 * W
        awf = np.abs(w * f)
        eBu = (awf * (rw + U64)).sum() + (m - 1) * U64 * awf.sum()
        base = Bu / W
        e_base = eBu / W + abs(base) * eW / W + U64 * abs(base)
        if estimator == "normalised":
            den = W - w + p
            r = w / den
            c = r * (f - base)
            e_den = eW + w * rw + p * rp + 2 * U64 * (W + w + p)
            e_c = r * (e_base + U64 * np.abs(f - base)) + np.abs(c) * (rw + e_den / den + U64) + U64 * np.abs(c)
        else:
            t = 1.0 + w - p
            c = w * (f * t - Bu)
            e_t = w * rw + p * rp + 2 * U64 * (1.0 + w + p)
            e_s = np.abs(f) * e_t + U64 * np.abs(f * t) + eBu + U64 * np.abs(f * t - Bu)
            e_c = w * e_s + np.abs(c) * (rw + U64)
        coef[sl] = -c / N
        ecoef[sl] = e_c / N + (3 * U64 + U) * np.abs(c / N) + 2.0 ** -149
        ess = 1.0 / ((w / W) ** 2).sum()
        stats[i] = (W, base, ess)
        estats[i] = (eW, e_base, ess * (2 * (rw + eW / W + U64).max() + (m + 3) * U64))
    return coef, ecoef, (stats, estats)


def row_terms(x, V):
    """lse, p and their bounds of one stored row x [V] (fp32)"""
    v = x.astype(np.float64)
    M = v.max()
    s = np.exp(v - M).sum()
    lse = M + np.log(s)
    p = np.exp(v - lse)
    k = 4 * -(-V // 1024)
    e_lse = ((k + 9) * (E_EXP + 2) + (p * (M - v)).sum()) * U + V * TINY + E_EXP * U * abs(np.log(s)) + U * abs(lse)
    ep = p * (np.expm1(e_lse + U * np.abs(v - lse)) + E_EXP * U) + TINY
    return lse, e_lse, p, ep


def ref(c, inp):
    """The statement and its bounds for a case (or anything with the fields V, n, n_img, estimator, n_glob) and its inputs"""
    n, m, V = c.n, c.n - 1, c.V
    caps, lengths, perm, x = inp["caps"], inp["lengths"], inp["perm"], inp["x"]
    B, T = len(lengths), max(lengths)
    n_img = B // m
    coef, ecoef, (stats, estats) = coefs(inp["phi"], inp["G"], inp["scores"], n, c.estimator, n_of(c))
    g, gb = np.zeros((T * B, V)), np.zeros((T * B, V))
    lp, elp = np.zeros((T, B)), np.zeros((T, B))
    read = np.zeros(T * B, dtype=bool)
    for t in range(T):
        for b in range(B):
            cf = coef[perm[b]]
            if lengths[b] <= t or np.float32(cf) == 0.0:
                continue
            row = t * B + b
            read[row] = True
            lse, e_lse, p, ep = row_terms(x[row, :V], V)
            y = int(caps[b, t + 1])
            lp[t, b] = float(x[row, y]) - lse
            elp[t, b] = e_lse + U * abs(lp[t, b])
            ind = (np.arange(V) == y).astype(np.float64)
            g[row] = cf * (ind - p)
            gb[row] = abs(cf) * (ep + U * np.abs(ind - p)) + U * np.abs(g[row]) + ecoef[perm[b]] * np.abs(ind - p) + 2.0 ** -149
    by_img, eby = np.zeros(n_img), np.zeros(n_img)
    row_of = {int(r): b for b, r in enumerate(perm)}
    for i in range(n_img):
        S = e = a = 0.0
        for j in range(m):
            b = row_of[i * n + j]
            s = 0.0
            for t in range(T):
                s += lp[t, b]
            cf = coef[i * n + j]
            S += cf * s
            a += abs(cf * s)
            e += abs(cf) * (elp[:, b].sum() + T * U64 * np.abs(lp[:, b]).sum()) + ecoef[i * n + j] * abs(s)
        by_img[i], eby[i] = S, e + (m + 1) * U64 * a
    loss = by_img.sum()
    eloss = eby.sum() + (-(-n_img // 256) + 8) * U64 * np.abs(by_img).sum() + U * abs(loss)
    return {"coef": coef, "coef_bound": ecoef, "stats": stats, "stats_bound": estats, "g": g, "g_bound": gb, "lp": lp, "lp_bound": elp,
            "read": read, "by_image": by_img, "by_image_bound": eby + U * np.abs(by_img), "loss": loss, "loss_bound": eloss}


# ---- a toy categorical: Gumbel top-n is a sample without replacement -------------------------------------------------------------
def gumbel_top_n(logp, n, draws, rs):
    """`draws` samples without replacement of n categories -> (idx [draws, n] sorted by perturbed value descending, G [draws, n])"""
    g = logp[None, :] - np.log(-np.log(rs.rand(draws, logp.shape[0])))
    idx = np.argsort(-g, axis=1, kind="stable")[:, :n]
    return idx, np.take_along_axis(g, idx, 1)


def toy_gradients(theta, f, n, draws, rs, form):
    """per-draw estimates [draws, V] of d E[f] / d theta from the m = n - 1 samples of a Gumbel top-n draw; form "normalised" /
    "unbiased" / "plain" (the normalised form without the - w_i + p_i term, not built on the device)"""
    V = theta.shape[0]
    logp = theta - (theta.max() + np.log(np.exp(theta - theta.max()).sum()))
    idx, G = gumbel_top_n(logp, n, draws, rs)
    m = n - 1
    kappa = G[:, m:n]
    ph = logp[idx[:, :m]]
    fs = f[idx[:, :m]]
    lq, _, _ = log_q(ph - kappa)
    p, w = np.exp(ph), np.exp(ph - lq)
    W = np.zeros(draws)
    Bu = np.zeros(draws)
    for j in range(m):
        W = W + w[:, j]
        Bu = Bu + w[:, j] * fs[:, j]
    W, Bu = W[:, None], Bu[:, None]
    if form == "normalised":
        c = w / (W - w + p) * (fs - Bu / W)
    elif form == "plain":
        c = w / W * (fs - Bu / W)
    else:
        c = w * (fs * (1.0 + w - p) - Bu)
    pr = np.exp(logp)
    out = -c.sum(1)[:, None] * pr[None, :]
    for j in range(m):
        np.add.at(out, (np.arange(draws), idx[:, j]), c[:, j])
    return out


def toy_exact(theta, f):
    pr = np.exp(theta - theta.max())
    pr /= pr.sum()
    return pr * (f - (pr * f).sum())
