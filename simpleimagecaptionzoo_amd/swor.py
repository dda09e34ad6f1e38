"""SCST on samples drawn without replacement (beyond the reference; include/icz.h "SCST on without-replacement samples",
csrc/swor_objective.hip): the n distinct captions per image of stochastic_beam.sample_distinct (temperature 1) train the decoder
through the importance-weighted estimators of Kool, van Hoof and Welling (2019; ICLR 2020).  Per image the last slot is only the
threshold kappa = G[n - 1]; the m = n - 1 slots in front of it are the samples, with CIDEr-D scores f:

    q_i = 1 - exp(-exp(phi_i - kappa)),  p_i = exp(phi_i),  w_i = p_i / q_i,  W = sum w_j,  Bu = sum w_j f_j
    estimator "normalised" (default):  c_i = w_i / (W - w_i + p_i) (f_i - Bu / W)        (biased, low variance)
    estimator "unbiased":              c_i = w_i (f_i (1 + w_i - p_i) - Bu)
    loss = -(1 / N_img) sum_img sum_i c_i logp_i

The weights use the sampler's evaluation-mode phi; logp_i and the gradient come from a training-mode xe_forward on the sampled
captions (swor_forward: dropout on, state kept for the backward pass), whose rows must be sorted by decreasing length: make_batch
sorts them and keeps the way back (perm).  Every row repeats its image's features and per-image prologue; a batch with per-image
region counts (RegionBatch) is refused.  The entry points are functions: the handles and captioners keep their public surface."""
import collections
import ctypes as C
import math
import numbers

import torch

from ._lib import IczError, SworOpts, check, lib, ptr, stream_ptr
from .handle import grad_args

ESTIMATORS = {"normalised": 0, "unbiased": 1}
MIN_N, MAX_N = 3, 8

# captions int64 (rows, max_len + 1) with <sta> in front, lengths = the steps of each row (a host list, decreasing), perm int32 (rows,)
# on the host: sorted row b is sample_distinct's row perm[b] = img * n + slot; rows_of_image int64 (images, n - 1): the sorted row of
# every (image, slot)
SworBatch = collections.namedtuple("SworBatch", "captions lengths perm rows_of_image")


def check_args(n=5, estimator="normalised", n_img_global=0.0):
    """ValueError, before any device work, for n not an integer in 3..8 (bools included), an estimator other than "normalised" /
    "unbiased", an n_img_global that is not a finite real >= 0 -> (n, estimator code, n_img_global)"""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not MIN_N <= int(n) <= MAX_N:
        raise ValueError("slots per image must be an integer in %d..%d (the last one is the threshold), got %r" % (MIN_N, MAX_N, n))
    if not isinstance(estimator, str) or estimator not in ESTIMATORS:
        raise ValueError("estimator %r is not one of %s" % (estimator, sorted(ESTIMATORS)))
    g = n_img_global
    if isinstance(g, bool) or not isinstance(g, numbers.Real) or not math.isfinite(float(g)) or float(g) < 0.0:
        raise ValueError("n_img_global must be a finite real >= 0, got %r" % (g,))
    return int(n), ESTIMATORS[estimator], float(g)


def make_batch(ids, lens, sta_id, n):
    """sample_distinct's (ids (B n, max_len), lens (B n,)) -> the teacher-forced batch of its samples: each image's threshold slot
    n - 1 dropped, <sta> prepended, the rows sorted by decreasing length with a stable sort -> SworBatch.  A <pad> (0) drawn inside a
    caption's length stays a token; a caption cut at max_len has no <end>.  ValueError for a bad n, a row count that is no multiple
    of n, or an image with an empty slot (lens == 0: fewer than n sequences exist, toy vocabularies only; its threshold is -inf)."""
    n, _, _ = check_args(n)
    total, T = int(ids.shape[0]), int(ids.shape[1])
    if total < n or total % n or tuple(lens.shape) != (total,):
        raise ValueError("%d caption rows with %s lengths are not images x n = %d slots" % (total, tuple(lens.shape), n))
    host = [int(x) for x in lens.tolist()]
    if min(host) <= 0:
        raise ValueError("image %d has an empty slot (fewer than %d sequences exist): no threshold to weigh its samples by" % (host.index(min(host)) // n, n))
    if max(host) > T:
        raise ValueError("a length of %d for captions of %d tokens" % (max(host), T))
    kept = [r for r in range(total) if r % n != n - 1]
    order = sorted(range(len(kept)), key=lambda i: -host[kept[i]])          # (sorted() is stable)
    perm = [kept[i] for i in order]
    rows_of_image = torch.empty(total // n, n - 1, dtype=torch.int64)
    for b, r in enumerate(perm):
        rows_of_image[r // n, r % n] = b
    sel = ids.index_select(0, torch.tensor(perm, dtype=torch.int64, device=ids.device)).to(torch.int64)
    captions = torch.cat([torch.full((len(perm), 1), int(sta_id), dtype=torch.int64, device=ids.device), sel], 1)
    return SworBatch(captions, [host[r] for r in perm], torch.tensor(perm, dtype=torch.int32), rows_of_image)


def _n_of(batch):
    return int(batch.rows_of_image.shape[1]) + 1


def swor_forward(handle, feats, batch, rng=None, want_logits=False):
    """xe_forward(train=True) of `handle` on the batch's captions, every row on its image's features (index-selected: the per-image
    prologue is repeated per row).  feats: the handle's per-image tensor (BUTD / AoA (B, R, D), NIC (B, E)); a RegionBatch (per-image
    region counts) raises ValueError."""
    if not torch.is_tensor(feats):
        raise ValueError("SCST on distinct samples takes one feature tensor per batch; per-image region counts are out of its scope")
    n = _n_of(batch)
    if int(feats.shape[0]) != int(batch.rows_of_image.shape[0]):
        raise ValueError("%d images of features for a batch of %d" % (feats.shape[0], batch.rows_of_image.shape[0]))
    img_of_row = (batch.perm.to(torch.int64) // n).to(feats.device)
    return handle.xe_forward(feats.index_select(0, img_of_row), batch.captions, batch.lengths, rng, train=True, want_logits=want_logits)


def _opts(batch, phi, G, scores, estimator, n_img_global, device):
    """icz_swor_opts over the step's tensors, checked on the host (icz_swor_check) -> (struct, rows, stats, what must stay alive)"""
    n, est, n_glob = check_args(_n_of(batch), estimator, n_img_global)
    rows = int(batch.perm.shape[0])
    total = rows // (n - 1) * n
    for t, what in ((phi, "phi"), (G, "G"), (scores, "scores")):
        if not torch.is_tensor(t) or tuple(t.shape) != (total,):
            raise IczError("%s must be a tensor (%d,): one entry per slot of sample_distinct" % (what, total))
    phi = phi.to(device=device, dtype=torch.float32).contiguous()
    G = G.to(device=device, dtype=torch.float64).contiguous()
    scores = scores.to(device=device, dtype=torch.float64).contiguous()
    perm_host = batch.perm.to(dtype=torch.int32, device="cpu").contiguous()
    perm = perm_host.to(device)
    stats = torch.zeros(total // n, 3, dtype=torch.float64, device=device)
    o = SworOpts(n, est, n_glob, phi.data_ptr(), G.data_ptr(), scores.data_ptr(), perm.data_ptr(), stats.data_ptr())
    lens = (C.c_int32 * rows)(*[int(x) for x in batch.lengths])
    check(lib().icz_swor_check(C.byref(o), rows, C.cast(perm_host.data_ptr(), C.POINTER(C.c_int32)), lens))
    return o, rows, stats, (phi, G, scores, perm)


def xe_backward_swor(handle, grads, phi, G, scores, batch, estimator="normalised", n_img_global=0.0, want_dfeats=False):
    """xe_backward of `handle` (holding swor_forward's stored pass) with the without-replacement SCST loss: phi, G (sample_distinct)
    and scores (CiderDReward.reward_loo(..., return_scores=True)), one entry per slot, row img * n + slot; fills `grads`; returns
    (loss2, stats): loss2 = (loss (1,), sum_i (-c_i / N) logp_i per image (images,)) as device tensors, stats (images, 3) float64 =
    {W, the baseline Bu / W, the effective sample size 1 / sum (w / W)^2}; a NicHandle with want_dfeats adds d features per ROW
    (rows, E), rows in the batch's sorted order.  N = n_img_global if > 0 (data-parallel: the all-reduced image count), else the
    batch's image count.  ValueError for a bad estimator or n_img_global before any device work; a refused call (IczError) queues
    nothing and leaves the stored forward usable."""
    o, rows, stats, keep = _opts(batch, phi, G, scores, estimator, n_img_global, handle.device)
    out = torch.zeros(1 + stats.shape[0], dtype=torch.float32, device=handle.device)
    ga, dfe = grad_args(handle, handle._grad_struct(grads), want_dfeats)
    check(handle._e.xe_backward_swor(handle._h, C.byref(o), rows, *ga, ptr(out), stream_ptr()))
    handle._swor_live = keep         # the kernels read phi, G, scores and perm in stream order
    res = ((out[0:1], out[1:]), stats)
    return res + (dfe,) if want_dfeats else res


def swor_loss(logits, V, batch, phi, G, scores, estimator="normalised", n_img_global=0.0):
    """icz_test_swor_objective, the kernels alone: logits (T B, ldl) fp32 with ldl = its row stride (a multiple of 4, 16-byte aligned
    rows), row t B + b, for the batch's captions and lengths (T = the longest).  The gradient is written over `logits`; returns
    (coef (images n,), loss_rows (T, B), loss_out (1 + images,), stats (images, 3))."""
    dev = logits.device
    o, B, stats, _keep = _opts(batch, phi, G, scores, estimator, n_img_global, dev)
    T = int(max(batch.lengths))
    rows_t = (C.c_int32 * T)(*[sum(1 for x in batch.lengths if x > t) for t in range(T)])
    caps = batch.captions.to(device=dev, dtype=torch.int64).contiguous()
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[0] != T * B or logits.stride(1) != 1 or logits.shape[1] < V:
        raise IczError("logits must be an fp32 tensor (%d, >= %d) with unit column stride" % (T * B, V))
    coef = torch.empty(stats.shape[0] * o.n, dtype=torch.float32, device=dev)
    loss_rows = torch.empty(T, B, dtype=torch.float32, device=dev)
    out = torch.empty(1 + stats.shape[0], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().icz_test_swor_objective(C.byref(o), ptr(logits), int(V), int(logits.stride(0)), ptr(caps), int(caps.shape[1]), B, T, rows_t,
                                            ptr(coef), ptr(loss_rows), ptr(out), stream_ptr()))
    return coef, loss_rows, out, stats


__all__ = ["make_batch", "swor_forward", "xe_backward_swor", "swor_loss", "check_args", "SworBatch", "ESTIMATORS", "MIN_N", "MAX_N"]
