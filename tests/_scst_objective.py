"""The SCST objectives of include/icz.h ("SCST objectives"; csrc/scst_objective.hip) stated in float64 numpy, with per-element error
bounds and the case table of tests/test_gpu_scst_objective_step.py.  Plain numpy, not collected by pytest.

Statement (ref): rows r = img K + k, mask[r, 0] = 1, mask[r, t] = seq[r, t - 1] > 0, M = the global mask sum if given, else sum(mask).
  kind 0   obj = -sum(logp reward mask) / M,  coef = -reward mask / M
  kind 1   s_r = sum_t mask logp (ascending t), Q = softmax over the image's K rows of a s (shifted by the largest, ascending j),
           L_img = sum_k Q_k c_k (c = -scores), obj = sum L_img / N, coef = mask a Q_r (c_r - L_img) / N
  entropy  with d_v = x_v - lse and p_v = exp(d_v) of a stored row: H = -sum_v p_v d_v (a column with p_v = 0 adds 0),
           ent = sum(mask H) / M, loss = obj - b ent (b = 0: no row is read for H; H and ent are reported as 0),
           g[row, v] = coef (1[v == draw] - p_v) + (b mask / M) p_v (d_v + H); dead rows (mask 0, draw < 0) are zero and never read.
The inputs x, lse, logp are what the device holds (fp32 values); the statement takes them as given and works in float64.

Bounds (counted from the device's operations, never fitted to its output; u = 2^-24, u64 = 2^-53; expf ASSUMED within E_EXP = 4 ulp as
in _token_choice.py, the float64 exp within E_EXP64 = 4 ulp; TINY = 2^-126 covers an expf that underflows, TINY64 = 2^-1022 an exp):
  kind 0   coef 2 u |coef|; obj (ceil(B T / 256) + 15) u sum|term| / M                        (_token_choice.rf_ref's)
  kind 1   es_r = T u64 sum_t|mask logp|              T sequential float64 additions
           ed_j = a (es_j + es_max) + u64 (|a s_j| + |a s_max| + |d_j|)     d_j = a s_j - max: two products, one subtraction
           ee_j = e_j (expm1(ed_j) + E_EXP64 u64) + TINY64                  e_j = exp(d_j)
           eZ   = sum ee_j + K u64 Z;   eQ_j = (ee_j + Q_j eZ) / Z + u64 Q_j
           eL   = sum_j eQ_j |c_j| + (K + 1) u64 sum_j |Q_j c_j|
           coef: a / N (eQ_r |c_r - L| + Q_r (eL + u64 |c_r - L|)) + (4 u64 + u) |coef| + 2^-149   (three products, 1 / N, the fp32 store)
           obj:  (sum eL + (ceil(images / 256) + 8) u64 sum|L|) / N + u |obj|
  entropy  ep_v = p_v (u |d_v| + 2 E_EXP u) + TINY                    d_v rounded to fp32, then expf
           eH   = sum_v (ep_v |d_v| + 2 u p_v |d_v| + TINY) + (ceil(V / 1024) + 16) u64 sum|p d| + u |H|     fp32 terms, float64 sums, fp32 H
           ent:  sum(mask eH) / M + (ceil(B T / 256) + 10) u64 sum|H| / M + u |ent|;   loss: e_obj + b e_ent + u |b ent| + u |loss|
           g:    |coef| (ep + u |1 - p|) + e_coef |1[v = d] - p|                               the REINFORCE part (rf_ref's) + coef's own error
                 + |w| (ep |d + H| + p (u |d| + eH + u |d + H|)) + 4 u |w p (d + H)|          w = b / M in fp32; the entropy part
                 + 3 u (|part 1| + |part 2|) + 2 TINY                                         the products and the final sum; a product
                                                                                              below the smallest normal fp32 number
"""
import collections
import zlib

import numpy as np

U, U64 = 2.0 ** -24, 2.0 ** -53
E_EXP = E_EXP64 = 4
TINY, TINY64 = 2.0 ** -126, 2.0 ** -1022

Case = collections.namedtuple("Case", "name kind n_img K T V a b row0 msum n_glob design")


def _c(name, kind, n_img, K, T, V, a=1.0, b=0.0, row0=0, msum=0.0, n_glob=0.0, design=""):
    return Case(name, kind, n_img, K, T, V, a, b, row0, msum, n_glob, design)


# design words: "equal" = equal scores within an image; "s300" = log-prob sums 300 apart within an image
CASES = [
    _c("v53_1img_k2_t1", 1, 1, 2, 1, 53, a=1.0, b=0.01),                  # a tail that is no multiple of 4, ldl 64, one step
    _c("v1000_3img_k5_t5_a025", 1, 3, 5, 5, 1000, a=0.25, b=0.5),
    _c("v10102_2img_k8_t7_a4", 1, 2, 8, 7, 10102, a=4.0, b=0.01),          # the benchmark's width, ldl 10 112
    _c("v40003_2rows", 0, 2, 1, 2, 40003, b=0.5),                          # no cap on V
    _c("kind0_5img_k1_t4_b0", 0, 5, 1, 4, 1000, b=0.0),                    # icz_test_reinforce bit for bit
    _c("kind0_5img_k1_t4_b001", 0, 5, 1, 4, 1000, b=0.01),
    _c("kind0_5img_k1_t4_b05", 0, 5, 1, 4, 1000, b=0.5),
    _c("big_8img_k5_t7", 1, 8, 5, 7, 53, a=1.0, b=0.01),                   # rows T = 280 > 256: the strided sums wrap
    _c("merged_4img_row0_4", 0, 4, 1, 5, 1000, b=0.5, row0=4),             # Bs = 8: evaluation-mode rows (draw -1, NaN) in front
    _c("merged_b0", 0, 4, 1, 5, 53, b=0.0, row0=4),
    _c("risk_equal_scores", 1, 3, 5, 5, 53, a=1.0, b=0.01, design="equal"),
    _c("risk_s300_a1", 1, 2, 3, 6, 53, a=1.0, b=0.5, design="s300"),       # the shift: exp(-300) beside 1
    _c("risk_b0", 1, 3, 5, 5, 1000, a=1.0, b=0.0),                         # reinforce_dlogits_kernel behind scst_risk_kernel
    _c("risk_globals", 1, 3, 5, 5, 53, a=1.0, b=0.5, msum=123.0, n_glob=7.0),
    _c("kind0_mask_sum_global", 0, 5, 1, 4, 53, b=0.5, msum=61.0),
    _c("risk_n_img_global_only", 1, 2, 2, 3, 53, a=0.25, b=0.01, n_glob=5.0),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def pad_vocab(V):
    return (V + 63) & ~63


def inputs(c):
    """The device's inputs of a case (numpy, fp32 unless noted), dead rows and pad columns NaN-filled"""
    rs = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    B, T, V, ldl = c.n_img * c.K, c.T, c.V, pad_vocab(c.V)
    Bs = c.row0 + B if c.row0 else 0
    stride = Bs or B
    n_on = rs.randint(1, T + 1, size=B)        # mask-on steps per row
    n_on[0] = 1                                # a row that ends at step 1
    n_on[B - 1] = T                            # ... and one that never ends
    if B > 2:
        n_on[1] = 1
    seq = np.zeros((B, T), dtype=np.int64)
    for r in range(B):
        k = T if (r == B - 1) else n_on[r] - 1
        seq[r, :k] = rs.randint(3, V, size=k)
        if 0 < k < T and r % 2:
            seq[r, k - 1] = 2                  # <end> is a token above 0: the step behind it is still on
    mask = np.ones((B, T), dtype=bool)
    mask[:, 1:] = seq[:, :-1] > 0
    x = np.full((T * stride, ldl), np.nan, dtype=np.float32)
    lse = np.full(T * stride, np.nan, dtype=np.float32)
    draw = np.full(T * stride, -1, dtype=np.int32)
    logp = np.zeros((B, T), dtype=np.float32)
    live = 0
    for t in range(T):
        for r in range(B):
            row = t * stride + c.row0 + r
            draw[row] = rs.randint(0, V)       # dead rows of the rollout keep a valid draw: the mask alone must stop them
            if not mask[r, t]:
                continue
            if live % 5 == 3:                  # one logit 80 above the rest: H near 0, p underflows to 0 elsewhere
                v = rs.randn(V).astype(np.float32)
                v[rs.randint(0, V)] += 80.0
            elif live % 5 == 4:                # near uniform: H near log V
                v = (rs.randn(V) * 1e-3).astype(np.float32)
            else:
                v = (rs.randn(V) * 2.0).astype(np.float32)
            live += 1
            x[row, :V] = v
            v64 = v.astype(np.float64)
            m = v64.max()
            lse[row] = np.float32(m + np.log(np.exp(v64 - m).sum()))
            logp[r, t] = np.float32(v[draw[row]]) - lse[row]
    reward = (rs.randn(B, 1) * np.ones((1, T))).astype(np.float32)
    scores = rs.rand(B) * 3.0
    if c.design == "equal":
        scores = np.repeat(rs.rand(c.n_img) * 3.0, c.K)
    if c.design == "s300":
        logp[np.arange(0, B, c.K), 0] -= np.float32(300.0)
    return {"seq": seq, "logp": logp, "reward": reward, "scores": scores, "x": x, "lse": lse, "draw": draw, "Bs": Bs, "ldl": ldl}


def risk_terms(logp, mask, scores, K, a, N):
    """float64 statement of the risk term -> (obj, coef [B, T], L [images], Q [B]) with the bounds (e_obj, e_coef)"""
    B, T = logp.shape
    n_img = B // K
    lp = logp.astype(np.float64) * mask
    s = np.zeros(B)
    for t in range(T):
        s = s + lp[:, t]
    es = T * U64 * np.abs(lp).sum(1)
    c = -scores.astype(np.float64)
    coef, ecoef = np.zeros((B, T)), np.zeros((B, T))
    Ls, eLs, Qs = np.zeros(n_img), np.zeros(n_img), np.zeros(B)
    for i in range(n_img):
        sl = slice(i * K, (i + 1) * K)
        as_ = a * s[sl]
        jm = int(np.argmax(as_))
        d = as_ - as_[jm]
        ed = a * (es[sl] + es[sl][jm]) + U64 * (np.abs(as_) + abs(as_[jm]) + np.abs(d))
        e = np.exp(d)
        ee = e * (np.expm1(ed) + E_EXP64 * U64) + TINY64
        Z = 0.0
        for j in range(K):
            Z += e[j]
        eZ = ee.sum() + K * U64 * Z
        Q = e / Z
        eQ = (ee + Q * eZ) / Z + U64 * Q
        L = 0.0
        for j in range(K):
            L += Q[j] * c[sl][j]
        eL = (eQ * np.abs(c[sl])).sum() + (K + 1) * U64 * np.abs(Q * c[sl]).sum()
        Ls[i], eLs[i], Qs[sl] = L, eL, Q
        cf = a * Q * (c[sl] - L) / N
        ecf = a / N * (eQ * np.abs(c[sl] - L) + Q * (eL + U64 * np.abs(c[sl] - L))) + (4 * U64 + U) * np.abs(cf) + 2.0 ** -149
        coef[sl] = cf[:, None] * mask[sl]
        ecoef[sl] = ecf[:, None] * mask[sl]
    obj = Ls.sum() / N
    eobj = (eLs.sum() + (-(-n_img // 256) + 8) * U64 * np.abs(Ls).sum()) / N + U * abs(obj)
    return obj, coef, eobj, ecoef, Ls, Qs


def row_entropy(x, lse):
    """H and its bound of one stored row x [V] with its log-sum-exp, and (d, p, ep) for the gradient"""
    d = x.astype(np.float64) - float(lse)
    p = np.exp(d)
    ep = p * (U * np.abs(d) + 2 * E_EXP * U) + TINY
    pd = np.where(p > 0, p * d, 0.0)
    H = -pd.sum()
    eH = (ep * np.abs(d) + 2 * U * np.abs(pd) + TINY).sum() + (-(-x.size // 1024) + 16) * U64 * np.abs(pd).sum() + U * abs(H)
    return H, eH, d, p, ep


def ref(c, inp):
    """The statement and its bounds for a case (or anything with the fields kind, K, T, V, a, b, row0, msum, n_glob) and its inputs"""
    seq, logp = inp["seq"], inp["logp"]
    B, T = seq.shape
    V, Bs = c.V, inp["Bs"]
    stride = Bs or B
    mask = np.ones((B, T))
    mask[:, 1:] = seq[:, :-1] > 0
    ms = mask.sum()
    M = float(np.float32(c.msum)) if c.msum else ms
    if c.kind == 0:
        terms = -logp.astype(np.float64) * inp["reward"].astype(np.float64) * mask
        obj = terms.sum() / M
        eobj = (-(-B * T // 256) + 15) * U * np.abs(terms).sum() / M
        coef = -inp["reward"].astype(np.float64) * mask / M
        ecoef = 2 * U * np.abs(coef)
    else:
        N = float(np.float32(c.n_glob)) if c.n_glob else float(B // c.K)
        obj, coef, eobj, ecoef, _, _ = risk_terms(logp, mask, inp["scores"], c.K, float(np.float32(c.a)), N)
    b = float(np.float32(c.b))
    w = b / M
    H, eH = np.zeros((B, T)), np.zeros((B, T))
    g, gb = np.zeros((T * stride, V)), np.zeros((T * stride, V))
    zero = np.ones(T * stride, dtype=bool)
    for t in range(T):
        for r in range(B):
            row = t * stride + c.row0 + r
            if not mask[r, t] or inp["draw"][row] < 0:
                continue
            cc = coef[r, t]
            if b == 0.0 and cc == 0.0:
                continue
            zero[row] = False
            h, eh, d, p, ep = row_entropy(inp["x"][row, :V], inp["lse"][row])
            ind = (np.arange(V) == inp["draw"][row]).astype(np.float64)
            t1 = cc * (ind - p)
            e1 = abs(cc) * (ep + U * np.abs(ind - p)) + ecoef[r, t] * np.abs(ind - p)
            t2, e2 = 0.0, 0.0
            if b > 0.0:
                H[r, t], eH[r, t] = h, eh
                t2 = np.where(p > 0, w * p * (d + h), 0.0)
                e2 = abs(w) * (ep * np.abs(d + h) + p * (U * np.abs(d) + eh + U * np.abs(d + h))) + 4 * U * np.abs(t2)
            g[row] = t1 + t2
            gb[row] = e1 + e2 + 3 * U * (np.abs(t1) + np.abs(t2)) + 2 * TINY
    ent = (mask * H).sum() / M
    eent = (mask * eH).sum() / M + (-(-B * T // 256) + 10) * U64 * np.abs(H).sum() / M + U * abs(ent)
    loss = obj - b * ent
    eloss = eobj + b * eent + U * abs(b * ent) + U * abs(loss)
    return {"mask": mask, "ms": ms, "coef": coef, "coef_bound": ecoef, "obj": obj, "obj_bound": eobj, "H": H * mask, "H_bound": eH, "ent": ent,
            "ent_bound": eent, "loss": loss, "loss_bound": eloss, "g": g, "g_bound": gb, "zero_rows": zero}


def loss_of(c, inp):
    """the scalar loss alone (central differences)"""
    return ref(c, inp)["loss"]
