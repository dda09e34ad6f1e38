"""SCST objectives beyond RewardCriterion (beyond the reference; include/icz.h "SCST objectives", csrc/scst_objective.hip): what turns
the sampled captions of a handle's stored rollout into a gradient, in the place of the loss of its sample_backward.

    objective term   "reinforce": obj = -sum(logp reward mask) / M            (today's form; reward (rows, T))
                     "risk":      obj = mean_img sum_k Q_k c_k,  Q = softmax_k(risk_alpha sum_t mask logp),  c = -scores
                                  (minimum-risk training over the K = 2..8 samples of an image; scores (rows,) float64, the CIDEr-D
                                  of every sample: CiderDReward.reward_loo(..., return_scores=True))
    entropy term     loss = obj - entropy_weight * sum(mask H) / M,  H = the entropy of the word distribution a token was drawn from

Rows are img * K + k, as multisample.sample_n lays them out.  The entry points are functions: the handles and captioners keep their
public surface."""
import ctypes as C
import math
import numbers

import torch

from ._lib import IczError, ScstObjective, check, lib, ptr, stream_ptr
from .handle import grad_args

KINDS = {"reinforce": 0, "risk": 1}
MAX_K = 8


def _real(x, what, positive):
    if isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(float(x)) or (float(x) <= 0.0 if positive else float(x) < 0.0):
        raise ValueError("%s must be a finite real %s, got %r" % (what, "> 0" if positive else ">= 0", x))
    return float(x)


class Objective:
    """The checked arguments of one objective (make_objective); with_data() attaches the step's reward / scores."""

    def __init__(self, kind, K, risk_alpha, entropy_weight, n_img_global, reward=None, scores=None):
        self.kind, self.K, self.risk_alpha, self.entropy_weight, self.n_img_global = kind, K, risk_alpha, entropy_weight, n_img_global
        self.reward, self.scores = reward, scores

    def with_data(self, reward=None, scores=None, n_img_global=None):
        return make_objective(self.kind, self.K, self.risk_alpha, self.entropy_weight,
                              n_img_global=self.n_img_global if n_img_global is None else n_img_global, reward=reward, scores=scores)

    def struct(self, device, rows, T):
        """icz_scst_objective over this step's tensors -> (the struct, what must stay alive while the call is queued)"""
        reward = scores = None
        if self.kind == "reinforce":
            if self.reward is None:
                raise IczError("objective 'reinforce' needs reward (rows, T)")
            reward = self.reward.to(device=device, dtype=torch.float32).contiguous()
            if tuple(reward.shape) != (rows, T):
                raise IczError("reward has shape %s for a rollout of (%d, %d)" % (tuple(reward.shape), rows, T))
        elif self.scores is not None:      # (a risk term without scores is refused by the library, in its documented order)
            scores = self.scores.to(device=device, dtype=torch.float64).contiguous()
            if tuple(scores.shape) != (rows,):
                raise IczError("scores has shape %s for a rollout of %d rows" % (tuple(scores.shape), rows))
        o = ScstObjective(KINDS[self.kind], self.K, self.risk_alpha, self.entropy_weight, self.n_img_global,
                          None if reward is None else reward.data_ptr(), None if scores is None else scores.data_ptr())
        return o, (reward, scores)


def make_objective(kind="reinforce", K=1, risk_alpha=1.0, entropy_weight=0.0, *, n_img_global=0.0, reward=None, scores=None):
    """kind "reinforce" (K = 1..8 rows per image) or "risk" (K = 2..8), risk_alpha finite > 0, entropy_weight finite >= 0,
    n_img_global finite >= 0 (0: the call's image count; data-parallel: the all-reduced one), reward (rows, T) / scores (rows,)
    tensors or None (attached later by with_data) -> Objective.  ValueError for a bad argument, before anything touches a device."""
    if kind not in KINDS:
        raise ValueError("objective kind %r is not one of %s" % (kind, sorted(KINDS)))
    lo = 2 if kind == "risk" else 1
    if isinstance(K, bool) or not isinstance(K, numbers.Integral) or not lo <= int(K) <= MAX_K:
        raise ValueError("K must be an integer in %d..%d for objective %r, got %r" % (lo, MAX_K, kind, K))
    risk_alpha = _real(risk_alpha, "risk_alpha", True)
    entropy_weight = _real(entropy_weight, "entropy_weight", False)
    n_img_global = _real(n_img_global, "n_img_global", False)
    for t, what in ((reward, "reward"), (scores, "scores")):
        if t is not None and not torch.is_tensor(t):
            raise ValueError("%s must be a tensor or None" % what)
    return Objective(kind, int(K), risk_alpha, entropy_weight, n_img_global, reward, scores)


def objective_check(objective, rows, T):
    """icz_scst_objective_check on an Objective with its tensors attached (host only): IczError in the library's documented order"""
    dev = objective.reward.device if objective.reward is not None else objective.scores.device if objective.scores is not None else "cpu"
    o, _keep = objective.struct(dev, rows, T)
    check(lib().icz_scst_objective_check(C.byref(o), int(rows), int(T)))


def sample_backward_objective(handle, objective, grads, mask_sum_global=0.0, *, want_entropy=False, want_dfeats=False):
    """sample_backward of `handle` (a ButdHandle, AoaHandle or NicHandle holding a rollout: sample, rollouts or sample_n) with
    `objective` (make_objective, its reward / scores attached) in the place of RewardCriterion; fills `grads`; returns
    (loss3, mask_sum[, entropy][, dfeats]): loss3 = [loss, obj, ent] as a 3-element device tensor, the local mask sum as a 1-element
    one, entropy = mask * H (rows, T) with want_entropy, d features per image with want_dfeats (NicHandle only).  Kind "reinforce"
    with entropy_weight 0 is sample_backward bit for bit.  A refused call (IczError) queues nothing and leaves the rollout stored."""
    seq = handle._live[2]
    rows, T = int(seq.shape[0]), int(seq.shape[1])
    o, keep = objective.struct(handle.device, rows, T)
    out3 = handle._buf("obj_loss3", (3,), torch.float32)
    msum = handle._buf("obj_msum", (1,), torch.float32)
    ent = handle._buf("obj_ent", (rows, T), torch.float32) if want_entropy else None
    ga, dfe = grad_args(handle, handle._grad_struct(grads), want_dfeats)
    check(handle._e.sample_backward_objective(handle._h, C.byref(o), *ga, ptr(out3), ptr(ent), ptr(msum), float(mask_sum_global), stream_ptr()))
    handle._objective_live = keep     # the kernels read the reward / scores in stream order
    res = (out3, msum)
    if want_entropy:
        res += (ent,)
    if want_dfeats:
        res += (dfe,)
    return res


def objective_loss(objective, logp, seq, logits, V, draw, lse, *, mask_sum_global=None, Bs=0, row0=0, want_entropy=True):
    """icz_test_scst_objective, the kernels alone: logp / seq (B, T), logits (T Bs', ldl) fp32 with ldl = its row stride, draw int32 /
    lse fp32 (T Bs',) (Bs' = Bs or B); Bs > 0: Bs rows per step of which [row0, row0 + B) are the rollout's; mask_sum_global a
    1-element device tensor or None.  The gradient is written over `logits`; returns (coef (B, T), loss3 (3,), mask_sum (1,),
    entropy (B, T) or None)."""
    B, T = int(seq.shape[0]), int(seq.shape[1])
    dev = logits.device
    o, _keep = objective.struct(dev, B, T)
    coef = torch.empty(B, T, dtype=torch.float32, device=dev)
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    msum = torch.empty(1, dtype=torch.float32, device=dev)
    ent = torch.empty(B, T, dtype=torch.float32, device=dev) if want_entropy else None
    with torch.cuda.device(dev):
        check(lib().icz_test_scst_objective(C.byref(o), ptr(logp), ptr(seq), B, T, ptr(mask_sum_global), ptr(coef), ptr(out3), ptr(ent), ptr(msum),
                                            ptr(logits), int(V), int(logits.stride(0)), ptr(draw), ptr(lse), int(Bs), int(row0), stream_ptr()))
    return coef, out3, msum, ent


__all__ = ["make_objective", "objective_check", "sample_backward_objective", "objective_loss", "Objective", "KINDS", "MAX_K"]
