"""Host oracle of the beam-search options (include/icz.h: icz_beam_opts), not collected by pytest: one generic beam search -- the
reference's (BUTD_Model.py:236-318, shrinking k, ties of the top-k as torch orders them) -- written against a per-model step
closure, plus n-gram blocking, the length penalty and the n-best ranking.  With the default options its rank 0 is what
oracle.{butd,aoa,nic}.beam_search return."""
import numpy as np
import torch

from oracle import aoa as oa
from oracle import butd as ob
from oracle import nic as on

STA, END = 1, 2


def banned_tokens(prefix, n):
    """tokens v the prefix y_0..y_s may not take: (y_{s-n+2}, ..., y_s, v) already occurs in it"""
    s = len(prefix) - 1
    if n == 0 or s < n - 1:
        return []
    tail = prefix[s - n + 2:]
    return sorted({prefix[i + n - 1] for i in range(s - n + 2) if prefix[i:i + n - 1] == tail})


def lp_norm(score, tokens, kind, alpha):
    """the device's fp32 length penalty (kind 0 none, 1 avg, 2 wu)"""
    s, a = np.float32(score), np.float32(alpha)
    if kind == 1:
        return np.float32(s / np.power(np.float32(tokens), a))
    if kind == 2:
        return np.float32(s / np.power(np.float32(5 + tokens) / np.float32(6), a))
    return s


def beam_nbest(step, state, k, V, max_steps, block_ngram=0, lp_kind=0, lp_alpha=0.0):
    """step(prev (rows,), state) -> (logits (rows, V), state); state: tuple of tensors indexed by row.  Returns all k hypotheses
    of the image ranked as icz_beam_opts specifies: [(token list, raw score, finished)]."""
    prev = torch.full((k,), STA, dtype=torch.long)
    seqs = prev.view(k, 1)
    run = torch.zeros(k, 1)
    done = []
    live = True
    for stp in range(1, max_steps + 1):
        logits, state = step(prev, state)
        lsm = torch.log_softmax(logits, dim=1)
        if block_ngram and stp > 1:
            for r in range(seqs.shape[0]):
                ban = banned_tokens(seqs[r].tolist(), block_ngram)
                if ban:
                    lsm[r, ban] = -float("inf")
        sc = run.expand(-1, V) + lsm
        top, idx = (sc[0] if stp == 1 else sc.reshape(-1)).topk(k, 0, True, True)
        src, nxt = torch.div(idx, V, rounding_mode="floor"), idx % V
        seqs = torch.cat([seqs[src], nxt.view(-1, 1)], 1)
        keep = [j for j in range(len(nxt)) if int(nxt[j]) != END]
        for j in range(len(nxt)):
            if int(nxt[j]) == END:
                done.append((seqs[j].tolist(), float(top[j]), True))
        k -= len(nxt) - len(keep)
        if k == 0:
            live = False
            break
        seqs = seqs[keep]
        sel = src[keep]
        state = tuple(s[sel] for s in state)
        run = top[keep].view(-1, 1)
        prev = nxt[keep]
    hyps = done + ([(seqs[j].tolist(), float(run[j, 0]), False) for j in range(seqs.shape[0])] if live else [])
    order = sorted(range(len(hyps)), key=lambda e: (not hyps[e][2], -lp_norm(hyps[e][1], len(hyps[e][0]) - 1, lp_kind, lp_alpha), e))
    return [hyps[e] for e in order]


# ---- per-model step closures (one image; the state tensors carry every per-row input) ---------------------------------
def butd_closure(feats1, p, k):
    H = p["TD_atten.weight_hh"].shape[1]
    feats = feats1.expand(k, -1, -1)
    pre = ob.hoist(None, p)

    def step(prev, st):
        f, mean = st[0], st[1]
        logits, _, s = ob.step(f, mean, prev, st[2:], p, pre=pre)
        return logits, (f, mean) + tuple(s)
    return step, (feats, feats.mean(1)) + ob.zero_state(k, H), p["predict.bias"].shape[0]


def aoa_closure(feats1, p, k):
    enc1 = oa.refine(feats1, p)
    enc = enc1.expand(k, -1, -1)
    meanf = oa.masked_mean(enc1, None).expand(k, -1)

    def step(prev, st):
        logits, _, s = oa.dec_step(prev, st[2:], st[0], st[1], p)
        return logits, (st[0], st[1]) + tuple(s)
    Hd = enc.shape[2]
    return step, (enc, meanf) + tuple(torch.zeros(k, Hd) for _ in range(3)), p["decoder.predict.bias"].shape[0]


def nic_closure(feats1, p, k):
    h, c = on.init_state(feats1.expand(k, -1), p)

    def step(prev, st):
        logits, h, c = on.step(prev, st[0], st[1], p)
        return logits, (h, c)
    return step, (h, c), p["predict.bias"].shape[0]


CLOSURES = {"butd": butd_closure, "aoa": aoa_closure, "nic": nic_closure}


def nbest(model, feats1, p, k, max_steps, block_ngram=0, lp_kind=0, lp_alpha=0.0):
    with torch.no_grad():
        step, state, V = CLOSURES[model](feats1, p, k)
        return beam_nbest(step, state, k, V, max_steps, block_ngram, lp_kind, lp_alpha)


def repeats_ngram(tokens, n):
    """True if some n-gram occurs twice in the token list"""
    grams = [tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1)]
    return len(grams) != len(set(grams))
