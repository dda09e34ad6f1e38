"""XE training on K captions per image (include/icz.h: icz_butd_xe_forward_n, icz_test_xe_group_loss) stated through the oracle, and the
case tables of tests/test_gpu_xe_group_loss_step.py and tests/test_gpu_xe_grouped.py.  Plain numpy / torch, not collected by pytest.

The handle's statement (run): decoder row r = img * K + k of the grouped forward is row r of an ordinary XE batch over the features
repeated K times.  The oracle wants that batch sorted by decreasing length, so the rows are sorted (stably), the explicit dropout masks
[T, B K, ...] permuted with them, oracle.butd.forward_xe and label_smoothing_loss run in float64 under autograd, and the per-row results
are mapped back to img * K + k.  With per-image region counts every image is a batch of its own over feats[i, :count]; the per-image
sums of the loss are added and divided by the token count of the whole batch.

The kernel's statement (loss_ref): LabelSmoothingLoss over logits [T rows, ldl] with the mask t < len[row].  An active row goes through
the arithmetic of xe_loss_dlogits_kernel, so its bounds are the counted ones of tests/_token_choice.py (row_bounds with n_add_xe, the XE
gradient / row loss / loss lines of its docstring), taken over as they stand; an inactive (row, t) and the pad columns are exactly 0.
"""
import collections
import math
import zlib

import numpy as np
import torch

import _token_choice as tc
from oracle import butd as ob

U = tc.U


# ---- the handle's statement ---------------------------------------------------------------------------------------------------------
def sorted_rows(lengths):
    """the stable sort by decreasing length: position in the sorted batch -> row img * K + k"""
    return sorted(range(len(lengths)), key=lambda r: -int(lengths[r]))


class _float64:
    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.old)


def _rows(feats_rows, caps, lengths, p, masks, smoothing):
    """One sorted XE batch over the rows given (any order) -> (logits [n, T, V] detached, zero behind a row's end; the sum of the rows'
    KL terms, under autograd; alphas [n, T, R] detached, zero behind a row's end).  masks: None or (em, am, om) laid out [T, n, ...]."""
    order = sorted_rows(lengths)
    ls = [int(lengths[r]) for r in order]
    T, n = max(ls), len(ls)
    f = feats_rows[order]
    c = torch.as_tensor(np.asarray(caps)[order])
    m = [None if masks is None or x is None else np.asarray(x)[:T, order] for x in (masks or (None, None, None))]
    trace = {}
    packed = ob.forward_xe(f, c, ls, p, m[0], m[1], m[2], trace=trace)
    po = ob.packed_order(ls)
    tgt = torch.tensor([int(c[b, t + 1]) for b, t in po])
    kl_sum = ob.label_smoothing_loss(packed, tgt, smoothing) * len(po)
    V, R = packed.shape[1], f.shape[1]
    logits, alphas = np.zeros((n, T, V)), np.zeros((n, T, R))
    for i, (b, t) in enumerate(po):
        logits[order[b], t] = packed[i].detach().numpy()
    with torch.no_grad():
        for t in range(T):
            bt = sum(l > t for l in ls)
            am = None if m[1] is None else torch.as_tensor(m[1][t][:bt])
            _, al = ob.soft_attention(f[:bt], trace["h1"][t][:bt], p, am)
            for b in range(bt):
                alphas[order[b], t] = al[b].numpy()
    return logits, kl_sum, alphas


def run(sd_np, feats, captions, lengths, K, masks=None, smoothing=0.1, counts=None, n_tokens=None):
    """feats [B, R, D] fp32 numpy, captions [B K, L], lengths [B K] (= len - 1), masks None (evaluation mode) or (emb [T, B K, E], att
    [T, B K, R, A], out [T, B K, H]) keep flags; counts: None or the valid regions of every image; n_tokens: the loss normaliser (None:
    the sum of the lengths) -> {"logits" [B K, T, V], "alphas" [B K, T, R], "loss", "grads" {key: float64 numpy}, "active" [B K, T]}."""
    with _float64():
        p = {k: v.double().requires_grad_(True) for k, v in ob.to_params(sd_np).items()}
        lengths = [int(x) for x in lengths]
        B, T, N = feats.shape[0], max(lengths), float(n_tokens if n_tokens else sum(lengths))
        F = torch.as_tensor(np.asarray(feats), dtype=torch.float64)
        if counts is None:
            logits, kl, alphas = _rows(F.repeat_interleave(K, 0), captions, lengths, p, masks, smoothing)
        else:
            R = F.shape[1]
            logits, alphas, kl = None, np.zeros((B * K, T, R)), 0.0
            for i in range(B):
                c, sl = int(counts[i]), slice(i * K, (i + 1) * K)
                mi = None if masks is None else (masks[0][:, sl], masks[1][:, sl, :c], masks[2][:, sl])
                lg, kli, al = _rows(F[i:i + 1, :c].repeat_interleave(K, 0), np.asarray(captions)[sl], lengths[sl], p, mi, smoothing)
                if logits is None:
                    logits = np.zeros((B * K, T, lg.shape[2]))
                logits[sl, :lg.shape[1]] = lg
                alphas[sl, :al.shape[1], :c] = al
                kl = kl + kli
        loss = kl / N
        loss.backward()
        active = np.array([[t < l for t in range(T)] for l in lengths])
        return {"logits": logits, "alphas": alphas, "loss": float(loss.detach()), "active": active,
                "grads": {k: v.grad.numpy() for k, v in p.items()}}


def batch(rs, V, B, K, T, L=None, pattern=True):
    """Captions [B K, L] (L = T + 1 by default) and lengths (= len - 1) of a grouped batch: words 4..V-1, <sta> in front, <end> behind,
    zero padded.  pattern: row 0 has length 1 and row 1 length T (one image holds the shortest and the longest row), and, from two
    images on, every row of the LAST image is shorter than T; the rest are drawn from 1..T, in no order."""
    n = B * K
    lens = rs.randint(1, T + 1, size=n)
    if pattern:
        lens[0], lens[1] = 1, T
        if B >= 2 and T > 1:
            lens[(B - 1) * K:] = rs.randint(1, T, size=K)
    else:
        lens[rs.randint(0, n)] = T
    L = L or T + 1
    caps = np.zeros((n, L), dtype=np.int64)
    for r in range(n):
        caps[r, 0] = ob.STA
        caps[r, 1:lens[r]] = rs.randint(4, V, size=lens[r] - 1)
        caps[r, lens[r]] = ob.END
    return caps, [int(x) for x in lens]


def keep_masks(rs, T, rows, E, R, A, H):
    """explicit keep flags of a training-mode call, laid out for `rows` decoder rows"""
    return ((rs.rand(T, rows, E) < 0.5).astype(np.uint8), (rs.rand(T, rows, R, A) < 0.5).astype(np.uint8),
            (rs.rand(T, rows, H) < 0.5).astype(np.uint8))


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------
# n: how N is given -- "value" (n_tokens > 0), "dev" (a positive device scalar beside an n_tokens that must lose), "none" (n_tokens 0:
# the sum of the lengths)
Case = collections.namedtuple("Case", "name V n_img K T smoothing n")
CASES = [
    Case("v53_1x2_t1", 53, 1, 2, 1, 0.1, "none"),                 # ldl 64; the smallest: two rows, one step
    Case("v53_1x2_t7", 53, 1, 2, 7, 0.0, "value"),                # a row of length 1 beside one of length 7
    Case("v1000_3x5_t7", 1000, 3, 5, 7, 0.1, "dev"),              # ldl 1008
    Case("v1000_3x5_t1", 1000, 3, 5, 1, 0.0, "none"),
    Case("v10102_3x5_t7", 10102, 3, 5, 7, 0.1, "none"),           # the benchmark's width, ldl 10 112
    Case("v53_7x8_t7", 53, 7, 8, 7, 0.1, "value"),                # 56 rows x 7 steps = 392 (row, t) pairs > 256
    Case("v1000_7x8_t1", 1000, 7, 8, 1, 0.1, "dev"),
    Case("v10102_1x2_t7", 10102, 1, 2, 7, 0.0, "dev"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
GUARD = 8                     # guard words in front of and behind every output


def ldl_of(V):
    """the row stride of a case's logits: V rounded up to 16 floats (64 / 1008 / 10 112 for 53 / 1000 / 10 102)"""
    return (V + 15) & ~15


def lengths_of(c, sort=False):
    """per-row step counts, in no order: row 0 has 1 and row 1 has T; from two images on every row of the last image is below T; at
    T = 1 with more than two rows one row has 0 steps (the kernel alone takes that; the handle never passes it).  sort: descending."""
    rs = np.random.RandomState(zlib.crc32(("len/" + c.name).encode()) & 0x7FFFFFFF)
    rows = c.n_img * c.K
    lens = rs.randint(1, c.T + 1, size=rows)
    lens[0], lens[1] = 1, c.T
    if c.n_img >= 2 and c.T > 1:
        lens[(c.n_img - 1) * c.K:] = rs.randint(1, c.T, size=c.K)
    if c.T == 1 and rows > 2:
        lens[rows // 2] = 0
    lens = [int(x) for x in lens]
    return sorted(lens, reverse=True) if sort else lens


def inputs(c, sort=False):
    """The device's inputs of a case: lengths, captions [rows, T + 2] (targets 0 and V - 1 among them), logits x [T rows, ldl] fp32 with
    NaN in every inactive (row, t) and in the pad columns; every fifth active row has one logit 80 above the rest, every fifth is
    near uniform.  sort: the same case on lengths sorted descending (what icz_test_xe_loss takes)."""
    rs = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    rows, T, V, ldl = c.n_img * c.K, c.T, c.V, ldl_of(c.V)
    lens = lengths_of(c, sort)
    caps = rs.randint(0, V, size=(rows, T + 2)).astype(np.int64)
    longest = lens.index(T)
    caps[longest, 1] = 0                             # the targets 0 and V - 1, both at active steps
    caps[longest, T] = V - 1
    x = np.full((T * rows, ldl), np.nan, dtype=np.float32)
    live = 0
    for t in range(T):
        for r in range(rows):
            if lens[r] <= t:
                continue
            if live % 5 == 3:
                v = rs.randn(V).astype(np.float32)
                v[rs.randint(0, V)] += 80.0
            elif live % 5 == 4:
                v = (rs.randn(V) * 1e-3).astype(np.float32)
            else:
                v = (rs.randn(V) * 2.0).astype(np.float32)
            live += 1
            x[t * rows + r, :V] = v
    n_tokens = {"value": float(sum(lens)) + 3.0, "dev": 5.0, "none": 0.0}[c.n]
    n_dev = {"value": None, "dev": float(sum(lens)) * 2.0, "none": None}[c.n]
    return {"x": x, "caps": caps, "lengths": lens, "ldl": ldl, "n_tokens": n_tokens, "n_dev": n_dev}


def n_of(inp):
    if inp["n_dev"]:
        return float(np.float32(inp["n_dev"]))
    return float(np.float32(inp["n_tokens"])) if inp["n_tokens"] > 0 else float(sum(inp["lengths"]))


def loss_ref(c, inp):
    """(grad [T rows, V], its bound, loss_rows [T rows], their bounds, loss, its bound, active [T rows]); the formulas are
    _token_choice.xe_ref's with the mask t < len[row]"""
    rows, T, V, s, ldl = c.n_img * c.K, c.T, c.V, c.smoothing, inp["ldl"]
    lens, N = inp["lengths"], n_of(inp)
    conf, low = float(np.float32(1.0) - np.float32(s)), float(np.float32(s) / np.float32(V - 1))
    g, gb = np.zeros((T * rows, V)), np.zeros((T * rows, V))
    lr, rb, act = np.zeros(T * rows), np.zeros(T * rows), np.zeros(T * rows, dtype=bool)
    for t in range(T):
        for r in range(rows):
            if lens[r] <= t:
                continue
            i = t * rows + r
            act[i] = True
            x = inp["x"][i, :V]
            lpb = tc.row_bounds(x, tc.n_add_xe(V))[0]
            d64 = x.astype(np.float64) - float(x.max())
            lp = d64 - math.log(np.exp(d64).sum())
            tr = np.full(V, low)
            tr[inp["caps"][r, t + 1]] = conf
            p = np.exp(lp)
            g[i] = (p - tr) / N
            gb[i] = ((lpb + 2 * tc.E_EXP * U) * p + tc.TINY + 3 * U * (p + tr)) / N
            with np.errstate(divide="ignore", invalid="ignore"):
                ltr = np.where(tr > 0, np.log(np.where(tr > 0, tr, 1.0)), 0.0)
            term = np.where(tr > 0, tr * (ltr - lp), 0.0)
            lr[i] = term.sum()
            rb[i] = (-(-ldl // 256) + 14) * U * np.abs(term).sum() + lpb + 2 * tc.E_LOG * U * np.abs(ltr).max()
    loss = lr.sum() / N
    lb = ((-(-T * rows // 256) + 13) * U * np.abs(lr).sum() + rb.sum()) / N
    return g, gb, lr, rb, loss, lb, act
