"""Host oracle of constrained beam search (include/icz.h: icz_beam_constraints), not collected by pytest: the specification, one
image at a time, in plain torch / numpy on the step closures of tests/_beam_opts_oracle.py -- and the case tables and float64
statement of one constrained step on given logits, in the style of tests/_beam_step.py.

The search.  An image has c <= C constraints (lists of alternative word ids); a hypothesis's state is the bit mask of the constraints
it has satisfied, S = 2^C states of `beam` slots each.  Every step scores all live rows (run + log_softmax, fp32, a banned token
-inf); candidate (state s, slot j, token v) has target s | bit(v); the targets select in ascending order, target t taking its best
cap[t] finite candidates, ties to the lower flat index (s * beam + j) * V + v; <end> retires (and lowers cap[t]), everything else is
compacted into t's slots in pick order.  Every selection logs the smallest gap between neighbouring candidates it met, the first
rejected one included: a (config, image) pair whose smallest gap is below GAP_MIN is not comparable token for token, because the
device's and torch's log-softmax sum in different orders."""
import collections

import numpy as np
import torch

import _beam_opts_oracle as bo
import _beam_step as bs

STA, END = bo.STA, bo.END
GAP_MIN = 6e-5                   # the separation tests/test_gpu_beam_diverse.py keeps its configs above
MAX_LEFT_OUT = 0.10              # share of (config, image) pairs that may fall below it
SLOTS, MAX_A = 12, 4             # force_val slots per row: constraint c, alternative a -> c * 4 + a

Hyp = collections.namedtuple("Hyp", "tokens score finished state")


def bit_table(cons, V):
    """int array [V]: the bit of the constraint that holds token v (0: none)"""
    bits = np.zeros(V, dtype=np.int64)
    for c, alts in enumerate(cons):
        for w in alts:
            bits[w] = 1 << c
    return bits


def popcount(s):
    return bin(int(s)).count("1")


def rank(hyps, lp_kind, lp_alpha):
    """hyps in order (retirements, then live beams in (state, slot) order) -> ranked"""
    order = sorted(range(len(hyps)), key=lambda e: (-popcount(hyps[e].state), not hyps[e].finished,
                                                    -bo.lp_norm(hyps[e].score, len(hyps[e].tokens) - 1, lp_kind, lp_alpha), e))
    return [hyps[e] for e in order]


def select(keys, flats, n, gaps):
    """positions of the n best finite keys by (key descending, flat ascending); logs the gaps between neighbours up to the first
    rejected candidate"""
    keys = np.asarray(keys, dtype=np.float32)
    flats = np.asarray(flats, dtype=np.int64)
    fin = np.nonzero(np.isfinite(keys))[0]
    order = fin[np.lexsort((flats[fin], -keys[fin].astype(np.float64)))]
    for a, b in zip(order[:n], order[1:n + 1]):
        gaps.append(float(keys[a]) - float(keys[b]))
    return [int(i) for i in order[:n]]


def constrained_nbest(step, state, beam, C, cons, V, max_steps, block_ngram=0, lp_kind=0, lp_alpha=0.0, gaps=None):
    """step / state as bo.beam_nbest (the state's first row is used).  cons: the image's constraints (len(cons) <= C).  Returns all
    hypotheses of the image ranked as icz_beam_constraints specifies: [Hyp(tokens, raw score, finished, state)]."""
    gaps = [] if gaps is None else gaps
    S = 1 << C
    bits = bit_table(cons, V)
    cap = [beam] * S
    live = [[] for _ in range(S)]                 # per state: [(tokens, fp32 score)]
    live[0] = [([STA], np.float32(0))]
    state = tuple(x[:1] for x in state)
    done = []
    for stp in range(1, max_steps + 1):
        rows = [(s, j, b) for s in range(S) for j, b in enumerate(live[s])]
        if not rows:
            break
        prev = torch.tensor([b[0][-1] for _, _, b in rows], dtype=torch.long)
        logits, state = step(prev, state)
        lsm = torch.log_softmax(logits, dim=1)
        for i, (_, _, b) in enumerate(rows):
            if block_ngram and stp > 1:
                ban = bo.banned_tokens(b[0], block_ngram)
                if ban:
                    lsm[i, ban] = -float("inf")
        run = torch.tensor([float(b[1]) for _, _, b in rows], dtype=torch.float32)
        sc = (run.view(-1, 1) + lsm).numpy()                                  # fp32: run + log_softmax
        target = np.stack([s | bits for s, _, _ in rows])                     # [rows, V]
        flat = np.stack([(s * beam + j) * V + np.arange(V, dtype=np.int64) for s, j, _ in rows])
        new_live, sel = [[] for _ in range(S)], []
        for t in range(S):
            if cap[t] == 0:
                continue
            m = target == t
            if not m.any():
                continue
            ri, vi = np.nonzero(m)
            for p in select(sc[ri, vi], flat[ri, vi], cap[t], gaps):
                r, v = int(ri[p]), int(vi[p])
                tokens, score = rows[r][2][0] + [v], np.float32(sc[r, v])
                if v == END:
                    done.append(Hyp(tokens, float(score), True, t))
                    cap[t] -= 1
                else:
                    new_live[t].append((tokens, score))
                    sel.append(r)
        live = new_live
        if sel:
            idx = torch.tensor(sel, dtype=torch.long)
            state = tuple(x[idx] for x in state)
    hyps = done + [Hyp(b[0], float(b[1]), False, s) for s in range(S) for b in live[s]]
    return rank(hyps, lp_kind, lp_alpha)


def nbest(model, feats1, p, beam, C, cons, max_steps, block_ngram=0, lp_kind=0, lp_alpha=0.0, gaps=None):
    with torch.no_grad():
        step, state, V = bo.CLOSURES[model](feats1, p, 1)
        return constrained_nbest(step, state, beam, C, cons, V, max_steps, block_ngram, lp_kind, lp_alpha, gaps)


def contains(tokens, alts):
    return any(w in tokens[1:] for w in alts)


def earned_state(tokens, cons):
    """the state a token list has earned: bit c set iff it holds a word of constraint c"""
    return sum(1 << c for c, alts in enumerate(cons) if contains(tokens, alts))


# ---- whole-search configurations (tests/test_gpu_beam_constrained.py; tests/test_cpu_beam_constrained.py asserts their share of
# comparable pairs on the oracle alone).  A set gives the constraints of image 0; image i takes the set rotated by i, so one batch
# holds images of different counts.
SETS = [[[5]], [[7, 9]], [[5], [11, 12]], [[6], [8], [13, 14, 15]]]
BEAMS = (2, 3, 4)
VARIANTS = [(0, None), (3, ("wu", 0.9))]                                  # (block_ngram, length penalty)


def batch_constraints(set_index, n_img):
    return [SETS[(set_index + i) % len(SETS)] for i in range(n_img)]


def configs():
    """(beam, set index, block_ngram, length penalty)"""
    return [(b, si, blk, lp) for b in BEAMS for si in range(len(SETS)) for blk, lp in VARIANTS]


_GOLDEN, _PAIRS = {}, {}


def golden_case(golden_dir, name, regime):
    """-> (model, CPU parameters, CPU features of up to 3 images): what test_gpu_beam_opts._setup binds, without a device"""
    import os
    from oracle import butd as ob
    from synth import feats_from_seed
    from test_gpu_beam_opts import _regime
    key = (name, regime)
    if key not in _GOLDEN:
        g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
        sd = {k[3:]: v for k, v in g.items() if k.startswith("sd.")}
        if name.startswith("butd"):
            model, sd, feats = "butd", _regime(ob.strip_prefix(sd), g, regime, ""), torch.tensor(g["feats"])
        elif name.startswith("aoa"):
            B, R, D = [int(x) for x in g["dims"][:3]]
            model, sd, feats = "aoa", _regime(sd, g, regime, "decoder."), torch.from_numpy(feats_from_seed(int(g["feats_seed"]), B, R, D))
        else:
            model, sd, feats = "nic", _regime(sd, g, regime, ""), torch.tensor(g["feats"])
        p = {k: torch.tensor(np.asarray(v), dtype=torch.float32) for k, v in sd.items()}
        _GOLDEN[key] = (model, p, feats[:min(3, feats.shape[0])].contiguous())
    return _GOLDEN[key]


def oracle_pair(golden_dir, name, regime, cfg, img):
    """the oracle's full ranked list of one (config, image) pair and the smallest gap of its selections; computed once per process"""
    key = (name, regime, cfg, img)
    if key not in _PAIRS:
        from test_gpu_beam_opts import LP
        model, p, feats = golden_case(golden_dir, name, regime)
        beam, si, block, lp = cfg
        cons = batch_constraints(si, feats.shape[0])
        C = max(len(c) for c in cons)
        gaps = []
        hyps = nbest(model, feats[img:img + 1], p, beam, C, cons[img], 50, block, *LP[lp], gaps=gaps)
        _PAIRS[key] = (hyps, min(gaps) if gaps else float("inf"))
    return _PAIRS[key]


# ---- AoA on per-image region counts (golden aoa_adaptive, regime "track"; tests/test_gpu_beam_constrained.py).  20 steps, the
# handles' usual caption length, not 50: along this golden's longest hypotheses (50 tokens, still live at the limit, scores near
# -73) the fp32 recurrence drifts away from the float64 one from about step 40 on -- teacher-forced on the oracle's own tokens, the
# fp32 oracle's log-prob of single late steps is up to 6.7e-5 off the float64 oracle's and its 50-step score 1.5e-4, more than the
# 1e-4 a device score is held to.  At 20 steps the fp32 oracle stays within OWN_ERROR_MAX of float64 on every hypothesis compared;
# the CPU test asserts that (oracle_own_error), so the reference is good to a fifth of the tolerance it is used at.
AOA_ADAPTIVE_STEPS = 20
AOA_ADAPTIVE_CONFIGS = [(3, 2, 0, None), (2, 3, 3, ("wu", 0.9)), (4, 0, 0, None), (3, 1, 3, ("wu", 0.9))]
OWN_ERROR_MAX = 2e-5
_AOA = {}


def aoa_adaptive_case(golden_dir):
    """-> (golden arrays, state dict of regime "track", CPU parameters, padded CPU features, region counts)"""
    if "case" not in _AOA:
        import os
        from test_gpu_aoa import regime_sd
        from test_gpu_aoa_adaptive import counts_of, padded_feats
        g = dict(np.load(os.path.join(golden_dir, "aoa_adaptive.npz")))
        sd = regime_sd(g, "track")
        p = {k: torch.tensor(np.asarray(v), dtype=torch.float32) for k, v in sd.items()}
        _AOA["case"] = (g, sd, p, torch.from_numpy(padded_feats(g)), counts_of(g))
    return _AOA["case"]


def aoa_adaptive_pair(golden_dir, cfg, img):
    """the oracle's ranked list of image `img` on its unpadded features and the smallest gap of its selections; once per process"""
    if (cfg, img) not in _AOA:
        from test_gpu_beam_opts import LP
        _, _, p, f, counts = aoa_adaptive_case(golden_dir)
        beam, si, block, lp = cfg
        cons = batch_constraints(si, 3)
        gaps = []
        hyps = nbest("aoa", f[img:img + 1, :counts[img]], p, beam, max(len(c) for c in cons), cons[img], AOA_ADAPTIVE_STEPS, block, *LP[lp],
                     gaps=gaps)
        _AOA[(cfg, img)] = (hyps, min(gaps) if gaps else float("inf"))
    return _AOA[(cfg, img)]


def oracle_own_error(model, feats1, p, tokens, score):
    """|score - the float64 oracle's summed log-probability of `tokens`|, teacher-forced on parameters and features cast to float64:
    what the fp32 oracle's own arithmetic contributes to a score it reports"""
    with torch.no_grad():
        step, state, _ = bo.CLOSURES[model](feats1.double(), {k: v.double() for k, v in p.items()}, 1)
        state = tuple(x.double() for x in state)
        total = 0.0
        for a, b in zip(tokens[:-1], tokens[1:]):
            logits, state = step(torch.tensor([a]), state)
            total += float(torch.log_softmax(logits, 1)[0, b])
    return abs(score - total)


# ======================================================================================================================
# One constrained step on given logits (icz_test_beam_rowtopk_constrained / icz_test_beam_constrained_step), float64, on the row
# scores, bounds and tie classes of tests/_beam_step.py.  Every deciding comparison is a tie by construction or separated by
# bs.MARGIN x the score bound (the CPU test asserts it for every case).
ConsCase = collections.namedtuple("ConsCase", "name n_img beam C A V ldl step compact ngram words n_act cap rows run prefix routes hyp_cnt purpose")


def _ccase(name, n_img, beam, C, A, V, words, n_act, cap=None, rows=("ap",), step=3, compact=0, ngram=0, run=None, prefix=None, routes=None,
           hyp_cnt=None, **purpose):
    ldl = bs.round4(V)
    routes = tuple(r for r in (0, 1, 2, 3) if bs.fits(r, V, ldl, 0)) if routes is None else tuple(routes)
    cap = [[beam] * (1 << C)] * n_img if cap is None else cap
    return ConsCase(name, n_img, beam, C, A, V, ldl, step, compact, ngram, words, n_act, cap, rows, run, prefix, routes, hyp_cnt, purpose)


def words_array(c):
    w = np.full((c.n_img, c.C, c.A), -1, dtype=np.int32)
    for img, cons in enumerate(c.words):
        for q, alts in enumerate(cons):
            w[img, q, :len(alts)] = alts
    return w


def cons_inputs(c):
    """logits [rows, V] (NaN: not scored), run [rows] (NaN: not read), seqs [rows, L], n_act / cap [n_img, S], words, L"""
    rs = bs.seeded(c.name)
    S, K = 1 << c.C, (1 << c.C) * c.beam
    rows, L = c.n_img * K, c.step + 2
    n_act = np.asarray(c.n_act, dtype=np.int32).reshape(c.n_img, S)
    cap = np.asarray(c.cap, dtype=np.int32).reshape(c.n_img, S)
    logits = np.full((c.n_img if c.compact else rows, c.V), np.nan, dtype=np.float32)
    run = np.full(rows, np.nan, dtype=np.float32)
    seqs = np.full((rows, L), bs.CANARY, dtype=np.int32)
    made = {}
    for row in range(rows):
        img, r = divmod(row, K)
        s, j = divmod(r, c.beam)
        if j >= n_act[img, s]:
            continue
        spec = c.rows.get(row, ("ap",)) if isinstance(c.rows, dict) else c.rows[row % len(c.rows)] if isinstance(c.rows, list) else c.rows
        x = made[spec[1]] if spec[0] == "same" else bs.make_row(c.V, spec, rs)
        made[row] = x
        logits[img if c.compact else row] = x
        if c.step > 1:
            dflt = -6.0 * rs.rand()
            run[row] = dflt if c.run is None else c.run.get(row, dflt) if isinstance(c.run, dict) else c.run[row % len(c.run)]
    for row in range(rows):
        if c.prefix is None:
            p = [STA] + [0] * (c.step - 2) + [c.V - 1] if c.step > 1 else [STA]
        else:
            p = c.prefix.get(row) if isinstance(c.prefix, dict) else c.prefix
            p = [STA] + [0] * (c.step - 2) + [c.V - 1] if p is None else p
        assert len(p) == c.step, (c.name, len(p), c.step)
        seqs[row, :c.step] = p
    return {"logits": logits, "run": run, "seqs": seqs, "n_act": n_act, "cap": cap, "words": words_array(c), "L": L}


def cons_scored_rows(c, inp):
    """row -> (scores float64 [V] with the n-gram bans at -inf, bound, exact, run/row tie class, logits row)"""
    S, K = 1 << c.C, (1 << c.C) * c.beam
    out, classes = {}, {}
    for row in range(c.n_img * K):
        img, r = divmod(row, K)
        s, j = divmod(r, c.beam)
        if j >= inp["n_act"][img, s]:
            continue
        x = inp["logits"][img if c.compact else row]
        rn = np.float32(0.0) if c.step == 1 else inp["run"][row]
        ban = [v for v in bo.banned_tokens(inp["seqs"][row, :c.step].tolist(), c.ngram) if 0 <= v < c.V] if c.ngram else []
        sc, bound, exact = bs.row_scores(x, rn, ban)
        cls = classes.setdefault(x.tobytes(), len(classes))
        out[row] = (sc, bound, exact, (bs._bits(rn), cls), x, None)
    return out


def cons_rowtopk_ref(c, inp, log):
    """row -> (cand idx [cap], cand val [cap], force [12], bound): the row's best cap[state] over the tokens that are no constraint word
    of its image (an empty slot: SENT, -inf) and the score of every constraint word (-inf: banned or an empty slot)"""
    K = (1 << c.C) * c.beam
    res = {}
    for row, e in cons_scored_rows(c, inp).items():
        img, r = divmod(row, K)
        s = r // c.beam
        n = int(inp["cap"][img, s])
        sc = e[0].copy()
        force = np.full(SLOTS, -np.inf)
        for q, alts in enumerate(c.words[img]):
            for a, w in enumerate(alts):
                force[q * MAX_A + a] = e[0][w]
                sc[w] = -np.inf
        pick = bs.top_n([bs.Cand(sc[v], sc[v], v, bs._tie(e, v), e[1]) for v in bs.head(sc, n)], n, log, "%s row %d" % (c.name, row))
        idx = [p.flat for p in pick] + [bs.SENT] * (n - len(pick))
        val = [p.score for p in pick] + [-np.inf] * (n - len(pick))
        res[row] = (np.asarray(idx, dtype=np.int64), np.asarray(val), force, e[1])
    return res


def cons_new_state(c, inp):
    S, K = 1 << c.C, (1 << c.C) * c.beam
    rows, L = c.n_img * K, inp["L"]
    rs = bs.seeded("state " + c.name)
    st = {"n_act": inp["n_act"].copy(), "cap": inp["cap"].copy(), "run": inp["run"].astype(np.float64), "seqs_in": inp["seqs"].copy(),
          "seqs_out": np.full((rows, L), bs.CANARY, dtype=np.int32), "src_row": np.full(rows, bs.CANARY, dtype=np.int32),
          "it_next": np.full(rows, bs.CANARY, dtype=np.int64), "n_live": 0,
          "hyp_seq": np.full((rows, L), bs.CANARY, dtype=np.int32), "hyp_score": np.full(rows, bs.FILL), "hyp_len": np.full(rows, bs.CANARY, dtype=np.int32),
          "hyp_state": np.full(rows, bs.CANARY, dtype=np.int32), "hyp_cnt": np.zeros(c.n_img, dtype=np.int32)}
    for img in range(c.n_img):
        n = c.hyp_cnt[img] if c.hyp_cnt else 0
        st["hyp_cnt"][img] = n
        for h in range(n):
            st["hyp_seq"][img * K + h, :2] = (STA, END)
            st["hyp_score"][img * K + h] = float(np.float32(-1.0 - h - rs.rand()))
            st["hyp_len"][img * K + h] = 2
            st["hyp_state"][img * K + h] = 0
    return st


def cons_step_ref(c, inp, st, log):
    """One constrained step on the state (in place): every target's search over all (live row, token) pairs of its image."""
    S, K, V, beam, step = 1 << c.C, (1 << c.C) * c.beam, c.V, c.beam, c.step
    sr = cons_scored_rows(c, inp)
    st["max_bound"] = max([e[1] for e in sr.values()] + [0.0])
    for img in range(c.n_img):
        row0 = img * K
        bits = bit_table(c.words[img], V)
        na0, cap0 = st["n_act"][img].copy(), st["cap"][img].copy()
        live = 0
        for t in range(S):
            tr0 = row0 + t * beam
            cands = []
            for s in range(S):
                for j in range(int(na0[s])):
                    e = sr[row0 + s * beam + j]
                    tok = np.nonzero(((s | bits) == t) & (e[0] > -np.inf))[0]
                    keep = tok[np.argsort(-e[0][tok], kind="stable")[:int(cap0[t]) + 1]] if len(tok) else tok
                    # a row's ties beyond cap + 1 entries cannot matter: the stable sort keeps the lower tokens first
                    for v in keep:
                        cands.append(bs.Cand(e[0][v], e[0][v], (s * beam + j) * V + int(v), bs._tie(e, int(v)), e[1]))
            keep = []
            ends = 0
            for p in bs.top_n(cands, int(cap0[t]), log, "%s image %d target %d" % (c.name, img, t)):
                r, tok = divmod(p.flat, V)
                if tok == END:
                    ends += 1
                    if st["hyp_cnt"][img] < K:
                        h = row0 + st["hyp_cnt"][img]
                        st["hyp_cnt"][img] += 1
                        st["hyp_score"][h], st["hyp_len"][h], st["hyp_state"][h] = p.score, step + 1, t
                        st["hyp_seq"][h, :step] = st["seqs_in"][row0 + r, :step]
                        st["hyp_seq"][h, step] = END
                else:
                    keep.append((row0 + r, tok, p.score, p.bound))
            st["n_act"][img, t] = len(keep)
            st["cap"][img, t] = int(cap0[t]) - ends
            live += len(keep)
            bs._compact_rows(st, tr0, beam, keep, step, np.zeros(c.n_img * K))
        st["n_live"] += live > 0
    return st


W1, W2, W3 = [[5]], [[5], [11, 12]], [[6], [8], [13, 14, 15]]
_OH = lambda tok, base=0.0: ("onehot", tok, base)      # noqa: E731


def _cons_cases():
    cs = []
    # S = 2, 4, 8 with beam 4, 3, 2: every state live, a later step, all vocabularies of the three routes and their thresholds
    for V in (53, 3072, 3073, 10102, 10300):
        for beam, C, words in ((4, 1, W1), (3, 2, W2), (2, 3, W3)):
            S = 1 << C
            cs.append(_ccase("v%d_b%dc%d" % (V, beam, C), 2, beam, C, max(len(a) for a in words), V, [words, words[:C - 1] if C > 1 else []],
                             [[min(beam, 1 + (s % beam)) for s in range(S)], [beam] + [0] * (S - 1)], shapes=True))
    # 8 x 4 rows: the largest image
    cs.append(_ccase("rows32", 2, 4, 3, 3, 257, [W3, W3], [[4, 3, 2, 1, 4, 0, 2, 4], [1, 0, 0, 0, 0, 0, 0, 4]], shapes=True))
    # step 1: only state 0, slot 0 is live; compact logits
    cs.append(_ccase("step1", 2, 3, 2, 2, 53, [W2, W1], [[1, 0, 0, 0], [1, 0, 0, 0]], step=1, step1=True))
    cs.append(_ccase("step1_compact", 2, 3, 2, 2, 53, [W2, W1], [[1, 0, 0, 0], [1, 0, 0, 0]], step=1, compact=1, step1=True))
    # empty states beside full ones, a state at capacity 0 (all its beams retired earlier), capacity below beam
    cs.append(_ccase("empty_full_cap0", 2, 3, 2, 2, 53, [W2, W2], [[3, 0, 2, 0], [0, 0, 0, 3]], cap=[[3, 0, 2, 1], [3, 3, 0, 3]],
                     hyp_cnt=[4, 3], cap0=True))
    # constraint words that are n-gram-banned: word 5 (constraint 0) and 11 (constraint 1) banned in every row, 12 stays
    pb = bs.ban_prefix(2, [5, 11])
    cs.append(_ccase("banned_words", 1, 3, 2, 2, 53, [W2], [[2, 1, 1, 0]], ngram=2, step=len(pb), prefix=pb, banned_words=[5, 11]))
    pb2 = bs.ban_prefix(3, [5, 11, 30])
    cs.append(_ccase("banned_words_top", 1, 2, 2, 2, 3073, [W2], [[2, 1, 1, 1]], rows=("top", [5, 30, 11, 12, 7, 9, 10]), ngram=3, step=len(pb2),
                     prefix=pb2, banned_words=[5, 11]))
    # the row's best tokens are constraint words: they leave the ordinary list and arrive as forced candidates; rows of state 1
    # (constraint 0 satisfied) re-use word 5 and stay in state 1
    cs.append(_ccase("reuse_word", 1, 3, 2, 2, 53, [W2], [[2, 2, 0, 1]], rows=("top", [5, 12, 7, 11, 9, 10, 13]), reuse=True))
    # <end> retires in two states in one step
    cs.append(_ccase("end_two_states", 2, 2, 1, 1, 53, [W1, W1], [[2, 2], [1, 2]],
                     rows={0: _OH(END), 1: _OH(7), 2: _OH(END, 1.0), 3: _OH(9), 4: _OH(END), 6: _OH(END), 7: _OH(END, 0.5)},
                     run={0: -1.0, 1: -2.0, 2: -1.5, 3: -2.5, 4: -1.0, 6: -3.0, 7: -2.0}, step=4, hyp_cnt=[0, 1], ends_states=2))
    # ties by construction.  Equal logit bits: identical rows with identical run in states 0 and 1 -- state 0's forced word 5 and state
    # 1's re-used word 5 both target state 1 with equal scores, the lower flat index (state 0's row) first.
    cs.append(_ccase("tie_across_states", 1, 2, 1, 1, 53, [W1], [[1, 1]], rows={0: ("top", [5, 7, 9]), 2: ("same", 0)}, run={0: -1.5, 2: -1.5},
                     tie="states"))
    # exact rows: a forced candidate (state 0 row, word 5 at score -1.0) ties an ordinary one of target 1 (state 1 row, token 4 at -1.0):
    # flat index (0 * 2 + 0) * V + 5 < (1 * 2 + 0) * V + 4, the forced one first
    cs.append(_ccase("tie_forced_ordinary", 1, 2, 1, 1, 53, [W1], [[1, 1]], cap=[[2, 1]], rows={0: _OH(5), 2: _OH(4)}, run={0: -1.0, 2: -1.0},
                     tie="forced"))
    return cs


CONS_CASES = _cons_cases()


# finalize cases: name -> state dict (scores are given fp32 data: every output is compared exactly)
def _cfin(name, n_img, beam, C, steps_done, n_act, hyp_cnt, n_best, lp_kind, lp_alpha, hyp_state=None, hyp_score=None, hyp_len=None, run=None):
    rs = bs.seeded("cfin " + name)
    S = 1 << C
    K = S * beam
    L, rows = steps_done + 2, n_img * K
    f = {"n_img": n_img, "beam": beam, "C": C, "L": L, "steps_done": steps_done, "n_best": n_best, "lp_kind": lp_kind, "lp_alpha": lp_alpha,
         "n_act": np.asarray(n_act, dtype=np.int32).reshape(n_img, S), "run": (-1.0 - 8.0 * rs.rand(rows)).astype(np.float32),
         "seqs": rs.randint(3, 30, (rows, L)).astype(np.int32), "hyp_cnt": np.asarray(hyp_cnt, dtype=np.int32),
         "hyp_score": (-1.0 - 8.0 * rs.rand(rows)).astype(np.float32), "hyp_len": rs.randint(2, L, rows).astype(np.int32),
         "hyp_state": rs.randint(0, S, rows).astype(np.int32), "hyp_seq": rs.randint(3, 30, (rows, L)).astype(np.int32)}
    for key, upd in (("run", run), ("hyp_score", hyp_score), ("hyp_len", hyp_len), ("hyp_state", hyp_state)):
        for i, v in (upd or {}).items():
            f[key][i] = v
    return f


def cons_finalize_ref(f):
    n_img, beam, S, L, nb = f["n_img"], f["beam"], 1 << f["C"], f["L"], f["n_best"]
    K = S * beam
    out = np.zeros((n_img, nb, L), dtype=np.float32)
    lens = np.zeros((n_img, nb), dtype=np.int32)
    scores = np.zeros((n_img, nb), dtype=np.float32)
    sat = np.zeros((n_img, nb), dtype=np.int32)
    for img in range(n_img):
        nf = int(f["hyp_cnt"][img])
        ents = [(True, f["hyp_score"][img * K + h], int(f["hyp_len"][img * K + h]), f["hyp_seq"][img * K + h], int(f["hyp_state"][img * K + h]))
                for h in range(nf)]
        ents += [(False, f["run"][img * K + s * beam + j], f["steps_done"] + 1, f["seqs"][img * K + s * beam + j], s)
                 for s in range(S) for j in range(int(f["n_act"][img, s]))]
        ents = ents[:K]
        ns = [bo.lp_norm(e[1], e[2] - 1, f["lp_kind"], f["lp_alpha"]) for e in ents]
        order = sorted(range(len(ents)), key=lambda e: (-popcount(ents[e][4]), not ents[e][0], -float(ns[e]), e))
        for m in range(nb):
            if m < len(order):
                _, sc, ln, src, stt = ents[order[m]]
                out[img, m, :ln] = src[:ln]
                lens[img, m], scores[img, m], sat[img, m] = ln, sc, stt
            else:
                scores[img, m] = -np.inf
    return out, lens, scores, sat


def _cfin_cases():
    cs = collections.OrderedDict()
    for kind, alpha in ((0, 0.0), (1, 0.7), (2, 0.7)):
        # image 0: a live full-state beam outranks finished ones of fewer bits; 1: two finished tied in score, length and state;
        # 2: nothing at all (length 0, -inf); 3: a full list and live beams in several states
        cs["c2_lp%d" % kind] = _cfin("c2", 4, 3, 2, 5, [[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 2]], [3, 2, 0, 6], 3, kind, alpha,
                                     hyp_state={0: 0, 1: 1, 2: 2, 12: 1, 13: 1}, hyp_score={12: -3.5, 13: -3.5}, hyp_len={12: 4, 13: 4})
        cs["c3_lp%d" % kind] = _cfin("c3", 2, 2, 3, 4, [[1, 0, 2, 0, 1, 0, 0, 2], [0] * 8], [5, 16], 2, kind, alpha)
        cs["c1_lp%d" % kind] = _cfin("c1", 2, 4, 1, 6, [[2, 1], [0, 3]], [3, 4], 4, kind, alpha)
    return cs


CFIN_CASES = _cfin_cases()
