"""Host oracle of diverse beam search (include/icz.h: icz_beam_diversity), not collected by pytest: one image at a time, in plain
torch, on the step closures of tests/_beam_opts_oracle.py.  The beam of B rows splits into G groups of kg = B / G (rows
group-major).  Every step runs the decoder over all live rows; then the groups select in order, group g ranking its candidates
run + log_softmax by key = score - fp32(lambda * c), c = how often groups 0 .. g-1 picked the token at this step.  A pick keeps
its raw score; ties go to the lower flat index r * V + v within the group (written out here, not left to torch.topk)."""
import numpy as np
import torch

import _beam_opts_oracle as bo

STA, END = bo.STA, bo.END


def _top(key, n):
    """flat indices of the n largest finite keys, ties -> lower index (key: float32 numpy array)"""
    order = np.lexsort((np.arange(key.size), -key.astype(np.float64)))
    return [int(i) for i in order[:n] if np.isfinite(key[i])]


def diverse_nbest(step, state, B, G, lam, V, max_steps, block_ngram=0, lp_kind=0, lp_alpha=0.0):
    """step / state as bo.beam_nbest.  Returns the image's B hypotheses ranked as icz_beam_opts specifies:
    [(token list, raw score, finished)]."""
    kg = B // G
    lam32 = np.float32(lam)
    # live beams per group: lists of (prefix, raw score); the state holds the rows of all live beams, group-major
    groups = [[([STA], np.float32(0)) for _ in range(kg)] for _ in range(G)]
    prev = torch.full((B,), STA, dtype=torch.long)
    done = []
    for stp in range(1, max_steps + 1):
        logits, state = step(prev, state)
        lsm = torch.log_softmax(logits, dim=1)
        rows = [b for grp in groups for b in grp]
        for i, (seq, _) in enumerate(rows):
            if block_ngram and stp > 1:
                ban = bo.banned_tokens(seq, block_ngram)
                if ban:
                    lsm[i, ban] = -float("inf")
        run = torch.tensor([float(r[1]) for r in rows], dtype=torch.float32)
        sc = (run.view(-1, 1) + lsm).numpy()                                 # fp32: run + log_softmax
        cnt = np.zeros(V, np.float32)
        new_groups, sel = [], []
        base = 0
        for grp in groups:
            na = len(grp)
            if na == 0:
                new_groups.append([])
                continue
            nr = 1 if stp == 1 else na
            s = sc[base:base + nr]
            key = (s - lam32 * cnt[None, :]).astype(np.float32)            # product rounded on its own, then the subtraction
            picks = _top(key.reshape(-1), na)
            keep = []
            for f in picks:
                r, v = divmod(f, V)
                raw = np.float32(s[r, v])
                seq = grp[r][0] + [v]
                cnt[v] += 1
                if v == END:
                    done.append((seq, float(raw), True))
                else:
                    keep.append((seq, raw))
                    sel.append(base + r)
            new_groups.append(keep)
            base += na
        groups = new_groups
        if not sel:
            break
        idx = torch.tensor(sel, dtype=torch.long)
        state = tuple(x[idx] for x in state)
        prev = torch.tensor([b[0][-1] for grp in groups for b in grp], dtype=torch.long)
    hyps = done + [(b[0], float(b[1]), False) for grp in groups for b in grp]
    order = sorted(range(len(hyps)), key=lambda e: (not hyps[e][2], -bo.lp_norm(hyps[e][1], len(hyps[e][0]) - 1, lp_kind, lp_alpha), e))
    return [hyps[e] for e in order]


def nbest(model, feats1, p, B, G, lam, max_steps, block_ngram=0, lp_kind=0, lp_alpha=0.0):
    with torch.no_grad():
        step, state, V = bo.CLOSURES[model](feats1, p, B)
        return diverse_nbest(step, state, B, G, lam, V, max_steps, block_ngram, lp_kind, lp_alpha)
