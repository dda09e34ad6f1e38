"""Host oracle of scoring given captions (include/icz.h: icz_*_score_captions), not collected by pytest: teacher forcing through
the per-model step closures of tests/_beam_opts_oracle.py (as _sampling_oracle.decode_model decodes through them), the float64
log_softmax of the closures' fp32 logits, the length rule of the contract written out token by token, per-image region counts for
AoA, and for an ensemble the float64 log of the weighted mean of the members' softmaxes."""
import numpy as np
import torch

import _beam_opts_oracle as bo

STA, END = 1, 2


def length(row, V=None):
    """scored tokens of one caption: through the first <end> if it comes before any 0, else up to the first 0, else all of it; an
    id outside [0, V) ends the row as a 0 does"""
    for t, c in enumerate(row):
        c = int(c)
        if c == END:
            return t + 1
        if c == 0 or c < 0 or (V is not None and c >= V):
            return t
    return len(row)


def lengths(ids, V=None):
    return np.array([length(r, V) for r in np.asarray(ids)], np.int64)


def _force(steps, logw, states, ids, V):
    """teacher forcing of ids [rows, T] through the members' closures -> log-probs [rows, T] float64 (0 behind the length)"""
    rows, T = ids.shape
    lens = lengths(ids, V)
    out = np.zeros((rows, T), np.float64)
    prev = torch.full((rows,), STA, dtype=torch.long)
    with torch.no_grad():
        for t in range(T):
            live = t < lens
            if not live.any():
                break
            terms = []
            for m, step in enumerate(steps):
                logits, states[m] = step(prev, states[m])
                assert logits.dtype == torch.float32
                terms.append(torch.log_softmax(logits.double(), 1) + logw[m])
            lp = terms[0] if len(terms) == 1 and logw[0] == 0.0 else torch.log(torch.exp(torch.stack(terms)).sum(0))
            nxt = np.zeros(rows, np.int64)
            for r in range(rows):
                if live[r]:
                    out[r, t] = float(lp[r, int(ids[r, t])])
                    nxt[r] = int(ids[r, t]) if t + 1 < lens[r] else 0
            prev = torch.from_numpy(nxt)
    return out


def score_model(model, feats, p, n, ids, counts=None):
    """feats [n_img, ...] (CPU); rows img * n + j of ids [n_img n, T] are image img's captions.  counts: AoA region counts per
    image.  -> log-probs [n_img n, T] float64"""
    return score_ensemble([(model, p, feats)], None, n, ids, counts)


def score_ensemble(members, weights, n, ids, counts=None):
    """members: [(model, CPU parameters, CPU feats [n_img, ...])]; weights None = uniform.  log( sum_m w_m softmax(logits_m)[c] )
    in float64 of the members' fp32 logits -> [n_img n, T] float64"""
    ids = np.asarray(ids)
    w = np.asarray(weights if weights is not None else [1.0] * len(members), np.float64)
    with np.errstate(divide="ignore"):
        logw = np.log(w / w.sum())
    out = []
    for i in range(members[0][2].shape[0]):
        steps, states, V = [], [], None
        for model, p, feats in members:
            f1 = feats[i:i + 1, :counts[i]] if model == "aoa" and counts is not None else feats[i:i + 1]
            with torch.no_grad():
                step, state, V = bo.CLOSURES[model](f1, p, n)
            steps.append(step)
            states.append(state)
        out.append(_force(steps, logw, states, ids[i * n:(i + 1) * n], V))
    return np.concatenate(out)


def row_logp(x, tok):
    """float64 log_softmax(x)[tok] of one fp32 row"""
    x64 = np.asarray(x).astype(np.float64)
    return float(x64[tok] - (x64.max() + np.log(np.exp(x64 - x64.max()).sum())))


def ensemble_row_logp(xs, weights, tok):
    """float64 log( sum_m w_m softmax(x_m)[tok] ) of the members' fp32 rows"""
    w = np.asarray(weights if weights is not None else [1.0] * len(xs), np.float64)
    w = w / w.sum()
    p = 0.0
    for x, wm in zip(xs, w):
        x64 = np.asarray(x).astype(np.float64)
        e = np.exp(x64 - x64.max())
        p += wm * e[tok] / e.sum()
    return float(np.log(p))
