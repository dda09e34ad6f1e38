"""Host oracle of the sampling decode (include/icz.h: icz_sample_opts), not collected by pytest: the temperature / top-k / nucleus
filter and the inverse-CDF draw in float64 exactly as icz.h defines them, and the decode loop over the per-model step closures of
tests/_beam_opts_oracle.py (or one batched BUTD closure for the full-width test)."""
import numpy as np
import torch

import _beam_opts_oracle as bo
from oracle import butd as ob

STA, END = 1, 2


def filter_masses(x, temperature=1.0, top_k=0, top_p=1.0, dtype=np.float64, info=None):
    """x [V] fp32 logits -> the survivors' unnormalised masses [V] (`dtype`; 0 = filtered).  temperature and top_p are the fp32
    values the C struct carries.  info (a dict) receives the margins the full-width excuse rules look at."""
    t, p = dtype(np.float32(temperature)), dtype(np.float32(top_p))
    V = x.shape[0]
    y = x.astype(dtype) / t
    order = np.lexsort((np.arange(V), -y))                    # y descending, ties to the lowest index
    k = top_k if top_k > 0 else V
    surv = order[:k]
    m = np.exp(y[surv] - y[surv[0]])
    if info is not None:
        info["topk_margin"] = float(x[order[k - 1]] - x[order[k]]) if k < V else np.inf
        info["nucleus_margin"] = np.inf
    if p < 1:
        q = m / m.sum(dtype=dtype)
        before = np.concatenate([np.zeros(1, dtype), np.cumsum(q, dtype=dtype)[:-1]])
        keep = before < p
        keep[0] = True
        if info is not None:
            info["nucleus_margin"] = float(np.abs(before[1:] - p).min()) if len(before) > 1 else np.inf
        surv, m = surv[keep], m[keep]
    out = np.zeros(V, dtype)
    out[surv] = m
    return out


def draw(masses, u):
    """oracle.butd.inverse_cdf_draw on one row of masses"""
    return int(ob.inverse_cdf_draw(torch.from_numpy(np.asarray(masses, np.float64)).unsqueeze(0), [float(np.float32(u))])[0])


def cdf_margin(masses, u):
    """distance of the draw's target from the nearest CDF edge, in units of the total mass"""
    c = np.cumsum(np.asarray(masses, np.float64))
    return float(np.abs(c / c[-1] - float(np.float32(u))).min())


def sample_row(x, u, temperature=1.0, top_k=0, top_p=1.0, info=None):
    """-> (token, log_softmax(x)[token] in float64, keep mask)"""
    m = filter_masses(x, temperature, top_k, top_p, info=info)
    tok = draw(m, u)
    if info is not None:
        info["cdf_margin"] = cdf_margin(m, u)
    x64 = x.astype(np.float64)
    lse = x64.max() + np.log(np.exp(x64 - x64.max()).sum())
    return tok, float(x64[tok] - lse), m > 0


def decode(step, state, rows, u, T, temperature=1.0, top_k=0, top_p=1.0, trace=None):
    """step(prev (rows,), state) -> (logits (rows, V), state).  u [T, rows].  Returns ids [rows, T] int64 (the drawn <end>, 0 behind
    it) and log-probs [rows, T] float64 (0 behind <end>).  trace (a list) receives per step the fp32 logits [rows, V]."""
    prev = torch.full((rows,), STA, dtype=torch.long)
    fin = np.zeros(rows, bool)
    ids, lps = np.zeros((rows, T), np.int64), np.zeros((rows, T), np.float64)
    with torch.no_grad():
        for t in range(T):
            if fin.all():
                break
            logits, state = step(prev, state)
            x = logits.numpy()
            if trace is not None:
                trace.append(x.copy())
            nxt = np.zeros(rows, np.int64)
            for r in range(rows):
                if fin[r]:
                    continue
                tok, lp, _ = sample_row(x[r], u[t, r], temperature, top_k, top_p)
                ids[r, t], lps[r, t] = tok, lp
                fin[r] = tok == END
                nxt[r] = 0 if fin[r] else tok
            prev = torch.from_numpy(nxt)
    return ids, lps


def decode_model(model, feats, p, n, u, T, temperature=1.0, top_k=0, top_p=1.0, counts=None):
    """feats [n_img, ...] (CPU); rows img * n + j use u[:, img * n + j].  counts: AoA region counts per image."""
    ids, lps = [], []
    for i in range(feats.shape[0]):
        f1 = feats[i:i + 1] if counts is None else feats[i:i + 1, :counts[i]]
        with torch.no_grad():
            step, state, _ = bo.CLOSURES[model](f1, p, n)
        a, b = decode(step, state, n, u[:, i * n:(i + 1) * n], T, temperature, top_k, top_p)
        ids.append(a)
        lps.append(b)
    return np.concatenate(ids), np.concatenate(lps)


def butd_batched_closure(feats_rows, p):
    """one BUTD closure over all decoder rows (feats_rows [rows, R, D]: the image's features repeated per sample), hoisted"""
    H = p["TD_atten.weight_hh"].shape[1]
    pre = ob.hoist(feats_rows, p)
    mean = feats_rows.mean(1)

    def step(prev, st):
        logits, _, s = ob.step(feats_rows, mean, prev, st, p, pre=pre)
        return logits, tuple(s)
    return step, ob.zero_state(feats_rows.shape[0], H)
