"""The float64 oracle of the distillation loss (include/icz.h: icz_distill_opts; csrc/distill.hip), in numpy, with a torch twin for
autograd through a decoder oracle, the kernel-alone cases of tests/test_gpu_distill.py and the dropout compensation that makes a
teacher's evaluation-mode forward equal a student's training-mode forward under all-ones keep masks.

For a row with student logits s, teachers z_m, normalised weights w, target c, smoothing sigma, mixing alpha, temperature tau:
    q = sum_m w_m softmax(z_m / tau);  hard = sum_v true_v (log true_v - log_softmax(s)_v), true = 1 - sigma at c, sigma / (V - 1) elsewhere
    kd = tau^2 sum_v q_v (log q_v - log_softmax(s / tau)_v)  (terms with q_v = 0 are 0);  loss = ((1 - alpha) sum hard + alpha sum kd) / N
    d s = ((1 - alpha) (softmax(s) - true) + alpha tau (softmax(s / tau) - q)) / N"""
import numpy as np
import torch


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def norm_weights(weights, M):
    w = np.ones(M) if weights is None else np.asarray(weights, np.float64)
    return w / w.sum()


def teacher_q(teachers, weights, tau):
    """q [rows, V]; a member of weight 0 is not read (it may hold NaNs)"""
    w = norm_weights(weights, len(teachers))
    return sum(w[m] * np.exp(log_softmax(np.asarray(z, np.float64) / tau)) for m, z in enumerate(teachers) if w[m] > 0)


def smoothed_targets(V, targets, sigma):
    true = np.full((len(targets), V), sigma / (V - 1))
    true[np.arange(len(targets)), np.asarray(targets)] = 1.0 - sigma
    return true


def terms(s, teachers, weights, targets, sigma, alpha, tau, n):
    """-> (loss, sum hard / n, sum kd / n, d loss / d s), float64"""
    s = np.asarray(s, np.float64)
    V = s.shape[1]
    q = teacher_q(teachers, weights, tau)
    true = smoothed_targets(V, targets, sigma)
    lp1, lpT = log_softmax(s), log_softmax(s / tau)
    with np.errstate(divide="ignore", invalid="ignore"):
        hard = np.where(true > 0, true * (np.log(true) - lp1), 0.0).sum()
        kd = tau * tau * np.where(q > 0, q * (np.log(q) - lpT), 0.0).sum()
    ds = ((1 - alpha) * (np.exp(lp1) - true) + alpha * tau * (np.exp(lpT) - q)) / n
    return ((1 - alpha) * hard + alpha * kd) / n, hard / n, kd / n, ds


def loss_torch(logits, teachers, weights, targets, sigma, alpha, tau, n):
    """the same loss over a float64 torch tensor of student logits with an autograd graph -> (loss, hard / n, kd / n)"""
    V = logits.shape[1]
    q = torch.from_numpy(teacher_q(teachers, weights, tau))
    true = torch.from_numpy(smoothed_targets(V, targets, sigma))
    lp1, lpT = torch.log_softmax(logits, 1), torch.log_softmax(logits / tau, 1)
    hard = torch.where(true > 0, true * (torch.log(true.clamp_min(1e-300)) - lp1), torch.zeros_like(lp1)).sum()
    kd = tau * tau * torch.where(q > 0, q * (torch.log(q.clamp_min(1e-300)) - lpT), torch.zeros_like(lpT)).sum()
    return ((1 - alpha) * hard + alpha * kd) / n, hard / n, kd / n


# ---- the kernel-alone cases ------------------------------------------------------------------------------------------------------
VOCABS, ROWS, TAUS, ALPHAS, SIGMAS = (53, 1000, 10102), (1, 5), (0.25, 1.0, 2.0), (0.5, 1.0), (0.0, 0.1)
WEIGHT_KINDS = ("uniform", "unequal", "zero")
# row stride of a tensor of V columns: "tight" = V, "pad4" = the next multiple of 4 above V (16-byte rows), "odd" = an odd stride above
# V, "shift" = pad4 rows from a base pointer that is off 16 bytes by one float (aligned stride, unaligned pointer)
LD_KINDS = ("tight", "pad4", "odd", "shift")


def stride_of(kind, V):
    return {"tight": V, "pad4": (V + 4) // 4 * 4, "odd": V + 3 + V % 2, "shift": (V + 4) // 4 * 4}[kind]


def kernel_cases():
    """every V x rows x M once (24 cases); the other factors cycle at strides that give every V each value of each"""
    out, i = [], 0
    for V in VOCABS:
        for M in (1, 2, 3, 4):
            for rows in ROWS:
                kind = WEIGHT_KINDS[(i + i // 8) % 3]
                if kind == "zero" and M == 1:
                    kind = "uniform"
                out.append(dict(V=V, M=M, rows=rows, tau=TAUS[i % 3], alpha=ALPHAS[(i // 3) % 2], sigma=SIGMAS[(i // 2 + i // 8) % 2], weights=kind,
                                ld_s=LD_KINDS[i % 4], ld_t=LD_KINDS[(i // 2) % 4], ld_out=LD_KINDS[(i + 1 + i // 4) % 4], seed=1000 + i))
                i += 1
    # the rows the issue names, at the temperature that needs the shift: a spike of +80 in a teacher at tau = 0.25 with 5 rows, per V
    for V in VOCABS:
        out.append(dict(V=V, M=2, rows=5, tau=0.25, alpha=1.0, sigma=0.1, weights="unequal", ld_s="pad4", ld_t="pad4", ld_out="pad4", seed=2000 + V))
    return out


def case_id(c):
    return "V%d-r%d-M%d-t%g-a%g-s%g-%s-%s.%s.%s" % (c["V"], c["rows"], c["M"], c["tau"], c["alpha"], c["sigma"], c["weights"], c["ld_s"], c["ld_t"],
                                                    c["ld_out"])


def case_inputs(c):
    """fp32 inputs of a case: student [rows, V], teachers M x [rows, V], weights (None or list), targets [rows].  Row 0 (every case):
    a teacher logit +80 above the rest and target 0; with 5 rows, row 2: a near-uniform first teacher, row 4: target V - 1.  A member
    of weight 0 is all NaN."""
    rs = np.random.RandomState(c["seed"])
    V, M, rows = c["V"], c["M"], c["rows"]
    s = (rs.randn(rows, V) * 2.0).astype(np.float32)
    t = [(rs.randn(rows, V) * 2.0).astype(np.float32) for _ in range(M)]
    targets = rs.randint(0, V, size=rows).astype(np.int64)
    t[0][0, int(rs.randint(0, V))] += 80.0
    targets[0] = 0
    if rows >= 5:
        t[0][2] = (rs.randn(V) * 1e-3).astype(np.float32)
        targets[4] = V - 1
    w = None
    if c["weights"] == "unequal":
        w = [float(x) for x in (0.5, 1.5, 0.25, 3.0)[:M]]
    elif c["weights"] == "zero":
        w = [float(x) for x in (1.0, 0.0, 2.0, 0.5)[:M]]
        t[1][:] = np.nan
    return s, t, w, targets


# ---- a teacher whose evaluation-mode forward is the student's training-mode forward under all-ones keep masks --------------------------
def undo_full_keep_dropout(family, sd, dims):
    """A training-mode forward scales what every dropout keeps by 1 / (1 - p), so under all-ones keep masks it is NOT the
    evaluation-mode forward of the same weights.  Each dropout of the three decoders sits in front of a linear map (or behind a
    positively homogeneous one), so the factors fold into the weights: -> a copy of the state dict `sd` (reference keys, torch
    tensors) whose evaluation-mode logits equal, up to fp32 rounding, the training-mode logits of `sd` with every keep mask all ones.
    dims: BUTD (H, D, E), AoA (Hd, E), NIC: unused."""
    sd = {k: v.detach().clone() for k, v in sd.items()}
    if family == "nic":                 # NIC_Model.py: one dropout (p = 0.5) in front of predict
        sd["decoder.predict.weight_g"] *= 2.0
    elif family == "butd":              # BUTD_Model.py: the embedding, the attention's relu, the language LSTM's output (p = 0.5 each)
        H, D, E = dims
        sd["decoder.TD_atten.weight_ih"][:, H + D:H + D + E] *= 2.0
        sd["decoder.atten.affine.weight_g"] *= 2.0
        sd["decoder.predict.weight_g"] *= 2.0
    else:                               # AoA_Model.py
        Hd, E = dims
        sd["img_feats_porjection.0.weight"] *= 2.0           # relu(W x + b) dropped at 0.5
        sd["img_feats_porjection.0.bias"] *= 2.0
        for l in range(6):
            pre = "aoa_refine.aoa_layers.%d.aoa_block." % l
            sd[pre + "linear_V.weight"] /= 0.9               # the attention probabilities dropped at 0.1 (their rows sum to 1)
            sd[pre + "linear_V.bias"] /= 0.9
            sd[pre + "aoa_module.0.weight"] /= 0.7           # cat[x, query] dropped at 0.3
            sd[pre + "aoa_module.0.weight"][:Hd] /= 0.9      # the GLU's linear half: the sublayer output dropped at 0.1
            sd[pre + "aoa_module.0.bias"][:Hd] /= 0.9
        sd["decoder.lstm.weight_ih"][:, :E] *= 2.0           # the embedding dropped at 0.5
        sd["decoder.aoa_block.linear_V.weight"] /= 0.9       # the decoder's attention probabilities dropped at 0.1
        sd["decoder.aoa_block.linear_V.bias"] /= 0.9
        sd["decoder.aoa_block.aoa_module.0.weight"][:Hd] *= 2.0     # ctx is dropped at 0.5 at both of its uses (the LSTM input, predict)
        sd["decoder.aoa_block.aoa_module.0.bias"][:Hd] *= 2.0
    return sd
