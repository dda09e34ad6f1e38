"""Case tables and float64 reference of the kernels of one beam-search step (csrc/beam_kernels.h), each on given logits and a given
search state (tests/test_cpu_beam_step.py holds every case to its stated purpose and the reference to independent statements;
tests/test_gpu_beam_step.py runs the tables through icz_test_beam_rowtopk / icz_test_beam_step / icz_test_beam_finalize).  Plain numpy,
not collected by pytest.

A case is name -> shape -> purpose; the purpose is data that the CPU test recomputes (which kernel route 0 takes, how many tokens tie
at the top and which threads own them, how long the ban list is, which slots stay empty).

The reference: score = float64(run) + log_softmax_float64(logits[:V]), a banned token (_beam_opts_oracle.banned_tokens) scores -inf,
top-n by (score descending, flat index r * V + v ascending), and the merge / group-merge / finalize rules of include/icz.h written out
slot by slot.  A grouped search ranks by _diverse_beam_oracle's key score - fp32(lambda * c).

How a selection can be compared exactly.  The device score rs + ((x - mx) - ls) is a monotone function of the logit x within a row, so
equal logit bits in one row give equal scores, and bitwise identical rows with identical run bits give equal scores across rows: ties
BY CONSTRUCTION.  A row with one maximum and every other logit at least 150 below it ("exact row") has se = 1 and ls = 0 on any device
whose expf(<= -150) is 0 and logf(1) is 0, so its scores are fp32(run + fp32(x - mx)) bit for bit: the reference states them in fp32 and
their bound is 0 -- that is how an <end> ties a stored best_score and how two diverse keys tie.  Every other comparison that decides a
selection or its order must be separated in the reference by MARGIN = 64 x the score bound; every top-n of the reference logs the
smallest (gap / bound) it met and test_cpu_beam_step.py asserts >= 64 for every case.  It is a condition on the inputs, not a tolerance.

The score bound (u = 2^-24, counted, never fitted to a device), for a row of range d = max - min, normaliser ls and running score run:
  three fp32 roundings of the score        u (d + (d + ls) + (|run| + d + ls))       x - mx, (.) - ls, rs + (.)
  the log-sum-exp, relative error of se    (n_add + 2 E_EXP + d) u                   n_add = max(ceil(V / 256), 40) + 8 additions on an
                                                                                     element's path (thread, 6 in the wave, 2 in the block),
                                                                                     expf within E_EXP ulp (<= 2 E_EXP u), its argument's rounding u d
  logf                                     2 E_LOG u ls
E_EXP = E_LOG = 4 ulp is ASSUMED: the HIP headers and documents installed with ROCm state no figure for expf / logf.
At V = 10300, logits over [-8, 8]: ~1.2e-5, margin ~7.6e-4, against gaps of 1.55e-3 between the neighbours of an arithmetic progression.
A chained search adds a step's bound to the bound its source row's running score already carries."""
import collections
import math
import zlib

import numpy as np

import _beam_opts_oracle as bo

U = 2.0 ** -24
E_EXP = E_LOG = 4
MARGIN = 64.0
SENT = 0x7fffffff
STA, END = 1, 2
CANARY = -7                      # fill of every integer slot a kernel has no business writing
FILL = 7.0                       # fill of every float slot a kernel has no business writing
CAND = 8                         # BEAM_MAX_K: candidate slots per row
CAP = 128                        # BEAM_CAND_CAP: the register kernels' candidate list
ROUTES = {1: ("reg3", 3072), 2: ("reg10", 10240), 3: ("sweep", None)}


def seeded(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def round4(v):
    return (v + 3) & ~3


def fits(route, V, ldl, off):
    """whether a forced route can take the shape (include/icz.h); off = floats between a 16-byte boundary and the logits"""
    if route in (1, 2):
        return ldl % 4 == 0 and ldl >= round4(V) and off % 4 == 0 and V <= ROUTES[route][1]
    return True


def owner(v):
    """thread of the register kernels that holds element v (and its register slot u, j)"""
    return (v >> 2) & 255, v >> 10, v & 3


# ======================================================================================================================
# logits rows.  spec:
#   ("ap",)                      a permutation of an arithmetic progression over [-8, 8]: all gaps equal
#   ("top", positions)           an arithmetic progression over [-8, 4], the given positions at 6.0 + 0.03 i: the row's top, in order
#   ("ties", positions)          an arithmetic progression over [-8, 4], the given positions all at 6.0: tied at the top
#   ("const",)                   every logit 0.5
#   ("onehot", tok, base)        an exact row: logit `base` at tok, the others a permutation of base - 200 - (0 .. 8)
#   ("same", r)                  the bits of the case's row r
def make_row(V, spec, rs):
    kind = spec[0]
    if kind == "ap":
        return rs.permutation(np.linspace(-8.0, 8.0, V)).astype(np.float32)
    if kind in ("top", "ties"):
        x = rs.permutation(np.linspace(-8.0, 4.0, V)).astype(np.float32)
        pos = np.asarray(spec[1], dtype=np.int64)
        x[pos] = 6.0 + (0.03 * (len(pos) - np.arange(len(pos))) if kind == "top" else 0.0)
        return x
    if kind == "const":
        return np.full(V, 0.5, dtype=np.float32)
    if kind == "onehot":
        base = spec[2] if len(spec) > 2 else 0.0
        x = (base - 200.0 - rs.permutation(np.linspace(0.0, 8.0, V))).astype(np.float32)
        x[spec[1]] = base
        return x
    raise ValueError(spec)


def is_exact_row(x):
    mx = x.max()
    return int((x == mx).sum()) == 1 and (x.size == 1 or np.partition(x, -2)[-2] <= mx - 150.0)


def row_scores(x, run, banned=()):
    """(float64 scores [V], bound, exact) of one row: x fp32 [V], run an fp32 value (0 at step 1)."""
    x = np.asarray(x, dtype=np.float32)
    run32 = np.float32(run)
    mx = x.max()
    if is_exact_row(x):
        sc = (run32 + (x - mx)).astype(np.float32).astype(np.float64)            # fp32, as the device forms it with ls = 0
        bound, exact = 0.0, True
    else:
        d64 = x.astype(np.float64) - float(mx)
        ls = math.log(np.exp(d64).sum())
        sc = float(run32) + (d64 - ls)
        d = float(mx) - float(x.min())
        n_add = max(-(-x.size // 256), 40) + 8
        bound = U * (d + (d + ls) + (abs(float(run32)) + d + ls)) + (n_add + 2 * E_EXP + d) * U + 2 * E_LOG * U * ls
        exact = False
    sc = sc.copy()
    if len(banned):
        sc[np.asarray(banned, dtype=np.int64)] = -np.inf
    return sc, bound, exact


Cand = collections.namedtuple("Cand", "key score flat tie bound")           # key: what ranks; score: what is kept; tie: by-construction class


def head(keys, n):
    """flat indices of the n + 1 largest finite keys by (key descending, index ascending): all a top-n and its margin need"""
    keys = np.asarray(keys, dtype=np.float64)
    order = np.lexsort((np.arange(keys.size), -keys))[:n + 1]
    return [int(i) for i in order if keys[i] > -np.inf]


def top_n(cands, n, log, what):
    """The first n of the finite candidates by (key descending, flat ascending).  Every adjacent pair up to the first one left out is
    either a by-construction tie (equal tie class) or logs gap / bound."""
    c = sorted((c for c in cands if c.key > -np.inf), key=lambda c: (-c.key, c.flat))
    for a, b in zip(c[:n], c[1:n + 1]):
        if a.tie == b.tie:
            continue
        bd = max(a.bound, b.bound)
        gap = a.key - b.key
        log.append((what, gap / bd if bd > 0 else (np.inf if gap > 0 else 0.0)))
    return c[:n]


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def row_cands_count(n_act_img, r, k, groups, step):
    """candidates the row top-k emits for slot r of an image (n_act_img: int, or the image's per-group list): beam_row_cands"""
    if groups == 1:
        na = int(n_act_img)
        return na if r < (1 if step == 1 else na) else 0
    if step == 1:
        return k if r == 0 else 0
    kg = k // groups
    g = r // kg
    return min(k, int(sum(n_act_img[:g + 1]))) if (r % kg) < n_act_img[g] else 0


# ======================================================================================================================
# one step's inputs: logits rows, running scores, prefixes
StepCase = collections.namedtuple("StepCase", "name n_img k V ldl off step compact ngram groups lam n_act rows run prefix routes listed "
                                              "has_complete best_score hyp_cnt purpose")


def _case(name, n_img, k, V, n_act, rows=("ap",), ldl=None, off=0, step=3, compact=0, ngram=0, groups=1, lam=0.0, run=None, prefix=None,
          routes=None, listed=True, has_complete=None, best_score=None, hyp_cnt=None, **purpose):
    ldl = round4(V) if ldl is None else ldl
    routes = tuple(r for r in (0, 1, 2, 3) if fits(r, V, ldl, off)) if routes is None else tuple(routes)
    return StepCase(name, n_img, k, V, ldl, off, step, compact, ngram, groups, lam, n_act, rows, run, prefix, routes, listed, has_complete,
                    best_score, hyp_cnt, purpose)


def ban_prefix(ngram, tokens, step=None):
    """A prefix (its length is the step) that bans every token of `tokens`: <sta>, <pad> filler up to `step`, then (tail, b) for every
    b, then the tail again, the tail being ngram - 1 times <sta>.  (The leading <sta> in front of a tail bans <sta> as well; the
    reference reads the bans off the prefix, whatever they are.)"""
    tail = [STA] * (ngram - 1)
    body = []
    for b in tokens:
        body += tail + [int(b)]
    body += tail
    n = 1 + len(body)
    step = n if step is None else step
    assert step >= n
    fill = [0] * (step - n)                       # <pad>: never part of the tail
    return [STA] + fill + body


def periodic_prefix(step, period):
    """<sta> then tokens 3, 4, .. cycling with the given period: a ban list with many and duplicate entries"""
    return [STA] + [3 + (i % period) for i in range(step - 1)]


def case_inputs(c):
    """-> dict: logits [rows_l, V] fp32 (rows not scored: NaN), run [rows] fp32 (NaN where it is not read), seqs [rows, L] int32 (the
    prefixes, CANARY behind them), n_act (int32 [n_img] or [n_img, groups]), L."""
    rs = seeded(c.name)
    rows = c.n_img * c.k
    L = c.step + 2
    n_act = np.asarray(c.n_act, dtype=np.int32).reshape((c.n_img,) if c.groups == 1 else (c.n_img, c.groups))
    rows_l = c.n_img if c.compact else rows
    logits = np.full((rows_l, c.V), np.nan, dtype=np.float32)
    run = np.full(rows, np.nan, dtype=np.float32)
    seqs = np.full((rows, L), CANARY, dtype=np.int32)
    made = {}
    for row in range(rows):
        img, r = divmod(row, c.k)
        if row_cands_count(n_act[img], r, c.k, c.groups, c.step) == 0:
            continue
        spec = c.rows.get(row, ("ap",)) if isinstance(c.rows, dict) else c.rows[row % len(c.rows)] if isinstance(c.rows, list) else c.rows
        x = made[spec[1]] if spec[0] == "same" else make_row(c.V, spec, rs)
        made[row] = x
        logits[img if c.compact else row] = x
        if c.step > 1:
            dflt = -6.0 * rs.rand()
            run[row] = dflt if c.run is None else c.run.get(row, dflt) if isinstance(c.run, dict) else c.run[row % len(c.run)]
    for row in range(rows):
        if c.prefix is None:
            p = [STA] + list(3 + rs.randint(0, max(1, c.V - 3), c.step - 1)) if c.V > 3 else [STA] * c.step
        else:
            p = c.prefix.get(row) if isinstance(c.prefix, dict) else c.prefix[row % len(c.prefix)] if isinstance(c.prefix[0], list) else c.prefix
            p = [STA] + [0] * (c.step - 2) + [c.V - 1] if p is None else p          # no token twice at the end: no ban
        assert len(p) == c.step, (c.name, len(p), c.step)
        seqs[row, :c.step] = p
    return {"logits": logits, "run": run, "seqs": seqs, "n_act": n_act, "L": L}


def banned_of(c, inp, row):
    if not c.ngram:
        return []
    return [v for v in bo.banned_tokens(inp["seqs"][row, :c.step].tolist(), c.ngram) if 0 <= v < c.V]


def scored_rows(c, inp, log=None):
    """row -> (scores float64 [V], bound, tie class of token v as a function, n candidates)"""
    out = {}
    classes = {}
    for row in range(c.n_img * c.k):
        img, r = divmod(row, c.k)
        n = row_cands_count(inp["n_act"][img], r, c.k, c.groups, c.step)
        if n == 0:
            continue
        x = inp["logits"][img if c.compact else row]
        rn = np.float32(0.0) if c.step == 1 else inp["run"][row]
        sc, bound, exact = row_scores(x, rn, banned_of(c, inp, row))
        bound += inp.get("run_bound", np.zeros(c.n_img * c.k))[row]
        cls = classes.setdefault(x.tobytes(), len(classes))
        out[row] = (sc, bound, exact, (_bits(rn), cls), x, n)
    return out


def _tie(entry, v):
    sc, bound, exact, rc, x, _ = entry
    return ("x", _bits(sc[v])) if exact and bound == 0.0 else ("g", rc, _bits(x[v]))


def rowtopk_ref(c, inp, log):
    """row -> (idx [n], val float64 [n], bound): the row's best n by (score descending, token ascending); a slot without an admissible
    token is (SENT, -inf).  Rows that are not scored are absent: their slots keep the fill."""
    res = {}
    for row, e in scored_rows(c, inp).items():
        sc, bound, n = e[0], e[1], e[5]
        pick = top_n([Cand(sc[v], sc[v], v, _tie(e, v), bound) for v in head(sc, n)], n, log, "%s row %d" % (c.name, row))
        idx = [p.flat for p in pick] + [SENT] * (n - len(pick))
        val = [p.score for p in pick] + [-np.inf] * (n - len(pick))
        res[row] = (np.asarray(idx, dtype=np.int64), np.asarray(val), bound)
    return res


# ======================================================================================================================
# the search state and the merge rules
def new_state(c, inp):
    """The state a step reads, as the case gives it (numpy; floats float64 except where the device's fp32 bits matter)."""
    rows, L, k = c.n_img * c.k, inp["L"], c.k
    rs = seeded("state " + c.name)
    st = {
        "n_act": inp["n_act"].copy(), "run": inp["run"].astype(np.float64), "run_bound": np.zeros(rows),
        "seqs_in": inp["seqs"].copy(), "seqs_out": np.full((rows, L), CANARY, dtype=np.int32),
        "src_row": np.full(rows, CANARY, dtype=np.int32), "it_next": np.full(rows, CANARY, dtype=np.int64),
        "best_score": np.full(c.n_img, -np.inf), "best_len": np.full(c.n_img, CANARY, dtype=np.int32),
        "best_seq": np.full((c.n_img, L), CANARY, dtype=np.int32), "has_complete": np.zeros(c.n_img, dtype=np.int32),
        "n_live": 0, "hyp": None,
    }
    for img in range(c.n_img):
        if c.has_complete and c.has_complete[img]:
            st["has_complete"][img] = 1
            st["best_score"][img] = float(np.float32(c.best_score[img]))
            st["best_len"][img] = 2
            st["best_seq"][img, :2] = (STA, END)
    if c.listed:
        hyp = {"seq": np.full((rows, L), CANARY, dtype=np.int32), "score": np.full(rows, FILL), "len": np.full(rows, CANARY, dtype=np.int32),
               "cnt": np.zeros(c.n_img, dtype=np.int32)}
        for img in range(c.n_img):
            n = c.hyp_cnt[img] if c.hyp_cnt else 0
            hyp["cnt"][img] = n
            for h in range(n):
                hyp["seq"][img * k + h, :2] = (STA, END)
                hyp["score"][img * k + h] = float(np.float32(-1.0 - h - rs.rand()))
                hyp["len"][img * k + h] = 2
        st["hyp"] = hyp
    return st


def _retire(st, img, slot_seq, score, step, k, listed_only):
    """one <end> pick of image img: the best hypothesis (plain search only) and the n-best list"""
    if not listed_only and (not st["has_complete"][img] or score > st["best_score"][img]):
        st["has_complete"][img] = 1
        st["best_score"][img] = score
        st["best_len"][img] = step + 1
        st["best_seq"][img, :step] = slot_seq[:step]
        st["best_seq"][img, step] = END
    hyp = st["hyp"]
    if hyp is not None and hyp["cnt"][img] < k:
        s = img * k + hyp["cnt"][img]
        hyp["cnt"][img] += 1
        hyp["score"][s] = score
        hyp["len"][s] = step + 1
        hyp["seq"][s, :step] = slot_seq[:step]
        hyp["seq"][s, step] = END


def _compact_rows(st, first, slots, keep, step, bounds):
    """survivors `keep` = [(source row, token, score, bound)] into rows first .. first + slots - 1"""
    for j in range(slots):
        if j < len(keep):
            src, tok, score, bd = keep[j]
            st["seqs_out"][first + j, :step] = st["seqs_in"][src, :step]
            st["seqs_out"][first + j, step] = tok
            st["run"][first + j] = score
            bounds[first + j] = bd
            st["src_row"][first + j] = src
            st["it_next"][first + j] = tok
        else:
            st["src_row"][first + j] = first + j
            st["it_next"][first + j] = 0


def step_ref(c, inp, st, log, logits=None, step=None):
    """One step on the state (in place): the search over all (live row, token) pairs of an image, not over the per-row lists.
    logits / step override the case's (a chained search)."""
    step = c.step if step is None else step
    k, V, G = c.k, c.V, c.groups
    cc = c._replace(step=step)
    ii = dict(inp, logits=inp["logits"] if logits is None else logits, run=st["run"].astype(np.float32), seqs=st["seqs_in"], n_act=st["n_act"],
              run_bound=st["run_bound"])
    sr = scored_rows(cc, ii)
    # the reference's running score is float64: put it in place of its fp32 rounding (an exact row states fp32 itself)
    for row, e in sr.items():
        if not e[2] and step > 1:
            sc = e[0] + (st["run"][row] - float(np.float32(st["run"][row])))
            sr[row] = (sc,) + e[1:]
    bounds = st["run_bound"].copy()
    st["max_bound"] = max([e[1] for e in sr.values()] + [st.get("max_bound", 0.0)])      # of every score formed so far
    lam32 = np.float32(c.lam)
    for img in range(c.n_img):
        row0 = img * k
        if G == 1:
            na = int(st["n_act"][img])
            if na == 0:
                _compact_rows(st, row0, k, [], step, bounds)
                continue
            nr = 1 if step == 1 else na
            ent = [sr[row0 + r] for r in range(nr)]
            cands = [Cand(ent[f // V][0][f % V], ent[f // V][0][f % V], f, _tie(ent[f // V], f % V), ent[f // V][1])
                     for f in head(np.concatenate([e[0] for e in ent]), na)]
            keep = []
            for p in top_n(cands, na, log, "%s step %d image %d" % (c.name, step, img)):
                src, tok = divmod(p.flat, V)
                if tok == END:
                    _retire(st, img, st["seqs_in"][row0 + src], p.score, step, k, False)
                else:
                    keep.append((row0 + src, tok, p.score, p.bound))
            st["n_act"][img] = len(keep)
            st["n_live"] += len(keep) > 0
            _compact_rows(st, row0, k, keep, step, bounds)
            continue
        kg = k // G
        cnt = collections.Counter()
        live = 0
        for g in range(G):
            na, gr0 = int(st["n_act"][img, g]), row0 + g * kg
            if na == 0:
                _compact_rows(st, gr0, kg, [], step, bounds)
                continue
            nr = 1 if step == 1 else na
            pen = np.zeros(V, dtype=np.float32)
            for v, n_picked in cnt.items():
                pen[v] = lam32 * np.float32(n_picked)                             # the product rounded on its own
            ent = [sr[row0 if step == 1 else gr0 + r] for r in range(nr)]
            # an exact row: the device's fp32 key; any other: float64
            keys = [(e[0].astype(np.float32) - pen).astype(np.float64) if e[2] and e[1] == 0.0 else e[0] - pen.astype(np.float64) for e in ent]
            cands = []
            for f in head(np.concatenate(keys), na):
                r, v = divmod(f, V)
                e, key = ent[r], float(keys[r][v])
                if e[2] and e[1] == 0.0:
                    cands.append(Cand(key, e[0][v], f, ("x", _bits(key)), 0.0))
                else:
                    cands.append(Cand(key, e[0][v], f, (_tie(e, v), cnt[v]), e[1] + U * abs(key)))
            keep = []
            for p in top_n(cands, na, log, "%s step %d image %d group %d" % (c.name, step, img, g)):
                src, tok = divmod(p.flat, V)
                cnt[tok] += 1
                srow = gr0 + src                 # step 1: the scores are row 0's, the state that continues is the group's own first row's
                if tok == END:
                    _retire(st, img, st["seqs_in"][srow], p.score, step, k, True)
                else:
                    keep.append((srow, tok, p.score, ent[src][1]))
            st["n_act"][img, g] = len(keep)
            live += len(keep)
            _compact_rows(st, gr0, kg, keep, step, bounds)
        st["n_live"] += live > 0
    st["run_bound"] = bounds
    return st


def next_step(st):
    """what BeamBuf::search does between two steps: the sequences written become the ones read"""
    st["seqs_in"], st["seqs_out"] = st["seqs_out"], st["seqs_in"]
    return st


# ======================================================================================================================
# final selection
def live_rows(n_act_img, img, k, groups):
    if groups == 1:
        return [img * k + q for q in range(int(n_act_img))]
    kg = k // groups
    return [img * k + g * kg + q for g in range(groups) for q in range(int(n_act_img[g]))]


def lp_bound(ns):
    """fp32 normalised score: powf within 4 ulp (assumed), the quotient in it and the division: 10 u relative"""
    return 10 * U * abs(float(ns))


def finalize_ref(form, f, log):
    """f: dict of the state (n_img, k, L, steps_done, groups, n_act, run fp32, seqs, has_complete, best_score fp32, best_len, best_seq,
    hyp_cnt, hyp_score fp32, hyp_len, hyp_seq, n_best, lp_kind, lp_alpha) -> (out [n_img, n_best, L] float32, lens, scores float32)."""
    n_img, k, L, nb = f["n_img"], f["k"], f["L"], f["n_best"]
    out = np.zeros((n_img, nb, L), dtype=np.float32)
    lens = np.zeros((n_img, nb), dtype=np.int32)
    scores = np.zeros((n_img, nb), dtype=np.float32)
    for img in range(n_img):
        if form == 0:
            if f["has_complete"][img]:
                src, ln, sc = f["best_seq"][img], int(f["best_len"][img]), f["best_score"][img]
            else:
                bi, bv = 0, np.float32(-np.inf)
                for j in range(int(f["n_act"][img])):
                    if f["run"][img * k + j] > bv:
                        bv, bi = f["run"][img * k + j], j
                src, ln, sc = f["seqs"][img * k + bi], f["steps_done"] + 1, bv
            out[img, 0, :ln] = src[:ln]
            lens[img, 0], scores[img, 0] = ln, sc
            continue
        nf = int(f["hyp_cnt"][img])
        ents = [(True, f["hyp_score"][img * k + h], int(f["hyp_len"][img * k + h]), f["hyp_seq"][img * k + h]) for h in range(nf)]
        ents += [(False, f["run"][r], f["steps_done"] + 1, f["seqs"][r]) for r in live_rows(f["n_act"][img], img, k, f["groups"])]
        ents = ents[:k]
        ns = [bo.lp_norm(e[1], e[2] - 1, f["lp_kind"], f["lp_alpha"]) for e in ents]
        order = sorted(range(len(ents)), key=lambda e: (not ents[e][0], -float(ns[e]), e))
        for a, b in zip(order, order[1:]):
            if ents[a][0] != ents[b][0] or (_bits(ents[a][1]) == _bits(ents[b][1]) and ents[a][2] == ents[b][2]):
                continue                                                        # finished before live, or tied by construction
            bd = max(lp_bound(ns[a]), lp_bound(ns[b])) if f["lp_kind"] else 0.0
            gap = float(ns[a]) - float(ns[b])
            log.append(("finalize image %d" % img, gap / bd if bd > 0 else (np.inf if gap > 0 else 0.0)))
        for m in range(nb):
            if m < len(order):
                _, sc, ln, src = ents[order[m]]
                out[img, m, :ln] = src[:ln]
                lens[img, m], scores[img, m] = ln, sc
            else:
                scores[img, m] = -np.inf
    return out, lens, scores


# ======================================================================================================================
# row top-k cases (icz_test_beam_rowtopk): every route that fits the shape, and route 0.  purpose keys (test_cpu_beam_step.py):
#   route0       the kernel route 0 takes (asked of icz_beam_rowtopk_route_for)
#   wide_ld      ldl above V rounded up to 4
#   n_acts       the per-image n_act values present
#   scored       the rows that are scored
#   ties / list_cnt / threads    T tokens tied at the top; entries the register kernels' list receives; how many threads own the ties
#                ("min": at least that many, "max": at most)
#   path / rounds   the register kernels' path ("list": at most 128 entries, "overflow": more); rounds (at least) tau takes
#   banned / ban_entries / best_banned / slot_classes / admissible   tokens banned in row 0's prefix; ban-list entries, duplicates
#                counted (at least); the row's best token is banned; the (u, j) register slots the banned tokens cover; tokens left
#   no_ban       blocking is on but the step is below ngram or nothing matches
ROUTE0_AT = {3: 1, 7: 1, 255: 1, 256: 1, 257: 1, 1023: 1, 1025: 1, 2047: 1, 2048: 1, 2049: 1, 3071: 1, 3072: 1, 3073: 2, 10101: 2, 10102: 2,
             10240: 2, 10241: 3, 10300: 3}


def reg_list(x, na):
    """(entries the register kernels' candidate list receives, rounds tau took) for a row of scores x and na candidates"""
    t = np.full(256, -np.inf)
    for v in range(x.size):
        t[owner(v)[0]] = max(t[owner(v)[0]], x[v])
    taken = rounds = 0
    tau = -np.inf
    while rounds < CAND:
        tau = t.max()
        hit = (t == tau) & (tau > -np.inf)
        taken += int(hit.sum())
        t[hit] = -np.inf
        rounds += 1
        if taken >= na or tau == -np.inf:
            break
    return int(((x >= tau) & (x > -np.inf)).sum()), rounds


def _spread(T, V):
    return sorted((79 * i + 5) % V for i in range(T))


def _few(T, threads, nv4):
    return sorted(4 * (t + 256 * u) + j for t in range(threads) for u in range(nv4) for j in range(4))[:T]


def _rt_cases():
    cs = []
    for i, V in enumerate(sorted(ROUTE0_AT)):
        k = (1, 5, 8)[i % 3]
        cs.append(_case("v%d" % V, 3, k, V, [0, 1, k], ldl=round4(V) + (8 if i % 2 else 0), route0=ROUTE0_AT[V], wide_ld=bool(i % 2),
                        n_acts=sorted({0, 1, k})))
    cs += [
        _case("step1", 3, 5, 257, [5, 5, 5], step=1, scored=[0, 5, 10], route0=1),
        _case("step1_compact", 3, 5, 257, [5, 5, 5], step=1, compact=1, scored=[0, 5, 10], route0=1),
        _case("step1_sweep_compact", 2, 8, 10241, [8, 8], step=1, compact=1, scored=[0, 8], route0=3),
        _case("odd_ldl", 2, 5, 255, [5, 2], ldl=257, route0=3),
        _case("base_off4", 2, 5, 256, [5, 2], ldl=260, off=1, route0=3),
        _case("odd_ldl_big", 1, 5, 10102, [5], ldl=10103, route0=3),
    ]
    for T in (127, 128, 129, 200):
        cs.append(_case("ties%d_v1000" % T, 1, 8, 1000, [8], rows=("ties", _spread(T, 1000)), ties=T, list_cnt=T, threads=("min", 8), route0=1,
                        path="list" if T <= CAP else "overflow"))
        cs.append(_case("ties%d_v10101" % T, 1, 8, 10101, [8], rows=("ties", _spread(T, 10101)), ties=T, list_cnt=T, threads=("min", 8),
                        route0=2, path="list" if T <= CAP else "overflow"))
    cs += [
        _case("ties129_4threads", 2, 8, 10240, [8, 5], rows=("ties", _few(129, 4, 10)), ties=129, threads=("max", 4), route0=2, path="overflow", rounds=2),
        _case("ties129_11threads", 1, 8, 3072, [8], rows=("ties", _few(129, 11, 3)), ties=129, threads=("max", 11), route0=1, path="overflow"),
        _case("ties24_2threads", 1, 5, 3072, [5], rows=("ties", _few(24, 2, 3)), ties=24, threads=("max", 2), route0=1, path="list", rounds=2),
        _case("const600", 2, 5, 600, [5, 3], rows=("const",), ties=600, list_cnt=600, route0=1, path="overflow"),
        _case("const100", 1, 5, 100, [5], rows=("const",), ties=100, list_cnt=100, route0=1, path="list"),
        _case("ties_special_ids", 1, 5, 50, [3], rows=("ties", [0, 1, 2, 3, 9]), ties=5, path="list", route0=1),
    ]
    for n in (2, 3, 4):
        p = ban_prefix(n, [40, 150])
        cs.append(_case("ban_best_n%d" % n, 2, 5, 300, [5, 3], rows=("top", [40, 41, 150, 7, 299, 8, 9, 10]), ngram=n, step=len(p), prefix=p,
                        banned=[40, 150], best_banned=True, route0=1))
        cs.append(_case("ban_step_eq_n%d" % n, 1, 5, 300, [3], rows=("top", [1, 5, 6, 7]), ngram=n, step=n, prefix=[STA] * n, banned=[1],
                        best_banned=True, route0=1))
        if n > 2:
            cs.append(_case("ban_step_below_n%d" % n, 1, 5, 300, [3], rows=("top", [1, 5, 6, 7]), ngram=n, step=n - 1, prefix=[STA] * (n - 1),
                            no_ban=True, route0=1))
    slots3 = [1024 * u + 4 * (5 + u) + j for u in range(3) for j in range(4)]
    slots10 = [1024 * u + 4 * (5 + u) + j for u in range(10) for j in range(4)]
    cs += [
        _case("ban_periodic_200", 1, 5, 300, [4], rows=("top", list(range(3, 12))), ngram=2, step=200, prefix=periodic_prefix(200, 7),
              ban_entries=20, route0=1),
        _case("ban_periodic_256", 1, 5, 300, [4], rows=("top", list(range(3, 12))), ngram=4, step=256, prefix=periodic_prefix(256, 5),
              ban_entries=40, route0=1),
        _case("ban_many_200", 1, 8, 300, [8], rows=("top", [50, 3, 100, 101, 99, 102, 4, 103, 104, 105, 106, 107]), ngram=2, step=200,
              prefix=ban_prefix(2, range(3, 101), step=200), banned=list(range(3, 101)), ban_entries=98, best_banned=True, route0=1),
        _case("ban_many_sweep", 1, 8, 10300, [8], rows=("top", [50, 3, 100, 10299, 99, 102, 4, 103, 104, 105, 106, 107]), ngram=2, step=200,
              prefix=ban_prefix(2, range(3, 101), step=200), banned=list(range(3, 101)), ban_entries=98, best_banned=True, route0=3),
        _case("ban_slots_reg3", 1, 5, 3072, [5], rows=("top", slots3 + [9, 2000, 3071, 1, 0]), ngram=2, step=26, prefix=ban_prefix(2, slots3),
              banned=slots3, slot_classes=12, best_banned=True, route0=1),
        _case("ban_slots_reg10", 1, 5, 10240, [5], rows=("top", slots10 + [9, 2000, 10239, 1, 0]), ngram=2, step=82, prefix=ban_prefix(2, slots10),
              banned=slots10, slot_classes=40, best_banned=True, route0=2),
        _case("ban_tiny", 1, 5, 7, [5], ngram=2, step=10, prefix=ban_prefix(2, [3, 4, 5, 6]), banned=[1, 3, 4, 5, 6], admissible=2, route0=1),
    ]
    per = periodic_prefix(9, 3)
    for k, G, na in ((4, 2, [[2, 1], [0, 2]]), (6, 3, [[2, 0, 1], [1, 2, 2]]), (8, 4, [[2, 0, 2, 1], [0, 0, 0, 2]]), (8, 8, [[1, 0, 1, 1, 0, 0, 1, 1], [1] * 8])):
        cs.append(_case("grouped_k%dg%d" % (k, G), 2, k, 300, na, groups=G, step=9, route0=1, empty_middle=True))
        cs.append(_case("grouped_k%dg%d_ban" % (k, G), 2, k, 300, na, groups=G, step=9, ngram=3, prefix=per, rows=("top", [5, 3, 4, 6, 7, 8, 9, 10, 11]),
                        ban_entries=2, best_banned=True, route0=1, empty_middle=True))
    cs.append(_case("grouped_step1", 2, 6, 300, [[2, 2, 2], [2, 2, 2]], groups=3, step=1, scored=[0, 6], route0=1))
    cs.append(_case("grouped_sweep_route0", 1, 6, 10241, [[2, 0, 1]], groups=3, step=9, ngram=3, prefix=per,
                    rows=("top", [5, 3, 4, 6, 7, 8, 9, 10, 11]), ban_entries=2, route0=3, empty_middle=True))
    cs.append(_case("grouped_sweep_route0_no_ban", 1, 6, 10241, [[2, 0, 1]], groups=3, step=9, route0=3, empty_middle=True))
    return cs


RT_CASES = _rt_cases()
# refused (route, V, ldl, off): a register route on a vocabulary beyond it, on an odd ldl, on a misaligned base, on ldl below V rounded up
RT_REFUSED = [(1, 3073, 3076, 0), (2, 10241, 10244, 0), (1, 255, 257, 0), (2, 256, 260, 1), (1, 255, 255, 0), (3, 300, 299, 0), (0, 300, 299, 0)]


# ======================================================================================================================
# whole-step cases (icz_test_beam_step).  purpose keys:
#   end          per image how an <end> pick meets the stored best hypothesis: "wins", "loses", "ties"
#   ends         <end> picks per image;  listed_after  the n-best counts after the step;  n_act_after / n_live_after
#   vanish       beams of image 0 that end unfinished and unlisted (no admissible candidate)
#   copy         the prefix length the lane-strided copy moves
#   cross_tie    the picks of image 0 are the same token from rows 0, 1, .. in that order
#   c_of_token   (token, c): the count the last group sees for the token;  key_tie  the fused key would fall below the unfused one
A_, Y_ = 5, 9
R0_ = float(np.float32(-2.0 - 14 * 0.0371))
P5_ = np.float32(np.float32(0.3) * np.float32(5))
R1_ = float(np.float32(np.float32(R0_) - P5_))
_OH_END, _OH5, _OH7 = ("onehot", END), ("onehot", 5), ("onehot", 7)


def _step_cases():
    cs = [
        _case("end_vs_best", 3, 3, 23, [2, 2, 2], rows=[_OH_END, _OH5, ("ap",)], run=[-1.0, -3.0, 0.0], step=4, has_complete=[1, 1, 1],
              best_score=[-2.0, -0.5, -1.0], end=["wins", "loses", "ties"], n_live_after=3),
        _case("several_ends", 3, 4, 23, [3, 3, 3], rows=[_OH_END, _OH_END, _OH7, ("ap",)], run=[-1.0, -2.0, -3.0, 0.0], step=5,
              hyp_cnt=[0, 3, 4], ends=[2, 2, 2], listed_after=[2, 4, 4], n_act_after=[1, 1, 1]),
        _case("several_ends_no_list", 3, 4, 23, [3, 3, 3], rows=[_OH_END, _OH_END, _OH7, ("ap",)], run=[-1.0, -2.0, -3.0, 0.0], step=5,
              listed=False, ends=[2, 2, 2], n_act_after=[1, 1, 1]),
        _case("all_retire", 3, 3, 23, [2, 1, 0], rows=[_OH_END, ("onehot", END, 1.0), ("ap",)], run=[-1.0, -1.5, 0.0], step=3, ends=[2, 1, 0],
              n_act_after=[0, 0, 0], n_live_after=0),
        _case("dead_beside_live", 3, 5, 40, [3, 0, 1], step=6, n_live_after=2),
        _case("cross_row_tie", 1, 3, 40, [3], rows={0: ("ap",), 1: ("same", 0), 2: ("same", 0)}, run=[-1.5], step=4, cross_tie=True),
        _case("vanish", 1, 5, 7, [3], ngram=2, step=14, rows=("top", [0, 2, 4]),
              prefix={0: ban_prefix(2, [0, 2, 3, 4, 5, 6]), 1: ban_prefix(2, [0, 2, 3, 4, 5, 6]), 2: ban_prefix(2, [3, 4, 5, 6], step=14)},
              vanish=1, n_act_after=[1], ends=[1]),
    ]
    for s in (1, 64, 65, 130):
        cs.append(_case("copy_step%d" % s, 2, 5, 40, [5, 5] if s == 1 else [5, 3], step=s, copy=s))
    cs.append(_case("copy_step1_compact", 2, 5, 40, [5, 5], step=1, compact=1, copy=1))
    for k, G, na in ((4, 2, [[2, 1], [0, 2]]), (6, 3, [[2, 0, 1], [1, 2, 2]]), (8, 4, [[2, 0, 2, 1], [0, 0, 0, 2]]), (8, 8, [[1, 0, 1, 1, 0, 0, 1, 1], [1] * 8])):
        for lam in (0.0, 0.5, 0.3):
            cs.append(_case("grouped_k%dg%d_lam%g" % (k, G, lam), 2, k, 40, na, groups=G, lam=lam, step=4, empty_middle=True))
    cs += [
        _case("grouped_step1_lam0.5", 2, 6, 40, [[2, 2, 2], [2, 2, 2]], groups=3, lam=0.5, step=1, repeated_token=True),
        _case("grouped_step1_compact", 2, 8, 40, [[2, 2, 2, 2], [2, 2, 2, 2]], groups=4, lam=0.3, step=1, compact=1, repeated_token=True),
        _case("grouped_ban", 2, 6, 40, [[2, 0, 1], [1, 2, 2]], groups=3, lam=0.5, step=9, ngram=3, prefix=periodic_prefix(9, 3),
              rows=("top", [5, 3, 4, 6, 7, 8, 9, 10, 11]), ban_entries=2),
        _case("grouped_unfused_key", 1, 8, 23, [[2, 2, 1, 2]], groups=4, lam=0.3, step=3,
              rows={0: ("onehot", A_), 1: ("onehot", A_), 2: ("onehot", A_), 3: ("onehot", A_), 4: ("onehot", A_), 6: ("onehot", A_),
                    7: ("onehot", Y_)},
              run={0: -1.0, 1: -1.25, 2: -1.5, 3: -1.75, 4: -2.0, 6: R0_, 7: R1_}, c_of_token=(A_, 5), key_tie=True),
    ]
    return cs


STEP_CASES = _step_cases()

# chained searches: (name, k, groups, lambda, ngram); six steps of icz_test_beam_step on given logits [step][row]
CHAIN_STEPS, CHAIN_V, CHAIN_IMG = 6, 40, 2
CHAIN_CASES = [("chain_plain", 5, 1, 0.0, 0), ("chain_plain_ban2", 5, 1, 0.0, 2), ("chain_grouped", 6, 3, 0.5, 0), ("chain_grouped_ban3", 6, 3, 0.5, 3)]


def chain_case(name, k, G, lam, ngram):
    na = [k] * CHAIN_IMG if G == 1 else [[k // G] * G] * CHAIN_IMG
    return _case(name, CHAIN_IMG, k, CHAIN_V, na, groups=G, lam=lam, ngram=ngram, step=1)


def chain_logits(name, k):
    """[CHAIN_STEPS][rows, V]: permuted progressions with tokens 3 and 4 on top (so that n-grams repeat) and <end> near the top in
    about a third of the rows (so that beams retire)."""
    rs = seeded("chain " + name)
    out = []
    for s in range(CHAIN_STEPS):
        x = np.stack([rs.permutation(np.linspace(-8.0, 8.0, CHAIN_V)) for _ in range(CHAIN_IMG * k)])
        x[:, 3] = 8.6 + 0.3 * rs.rand(CHAIN_IMG * k)
        x[:, 4] = 8.2 + 0.3 * rs.rand(CHAIN_IMG * k)
        x[:, END] = np.where(rs.rand(CHAIN_IMG * k) < 0.35, 8.0 + 0.15 * rs.rand(CHAIN_IMG * k), x[:, END])
        out.append(x.astype(np.float32))
    return out


def chain_ref(name, k, G, lam, ngram, log):
    """the reference run as a whole search -> the state after every step (copies)"""
    c = chain_case(name, k, G, lam, ngram)
    L = CHAIN_STEPS + 1
    rows = CHAIN_IMG * k
    inp = {"logits": None, "run": np.zeros(rows, dtype=np.float32), "seqs": np.full((rows, L), CANARY, dtype=np.int32),
           "n_act": np.asarray(c.n_act, dtype=np.int32), "L": L}
    inp["seqs"][:, 0] = STA
    st = new_state(c, inp)
    lg = chain_logits(name, k)
    states = []
    for s in range(1, CHAIN_STEPS + 1):
        step_ref(c, inp, st, log, logits=lg[s - 1], step=s)
        states.append({key: (dict((a, b.copy()) for a, b in v.items()) if isinstance(v, dict) else v.copy() if hasattr(v, "copy") else v)
                       for key, v in st.items()})
        next_step(st)
    return c, inp, lg, states


# ======================================================================================================================
# finalize cases: name -> (form, state dict).  Scores are given fp32 data, so every output is compared exactly.
def _fin_state(name, n_img, k, steps_done, groups, n_act, hyp_cnt, n_best, lp_kind, lp_alpha, has_complete=None, run=None, hyp_score=None,
               hyp_len=None):
    rs = seeded("fin " + name)
    L, rows = steps_done + 2, n_img * k
    f = {"n_img": n_img, "k": k, "L": L, "steps_done": steps_done, "groups": groups, "n_best": n_best, "lp_kind": lp_kind, "lp_alpha": lp_alpha,
         "n_act": np.asarray(n_act, dtype=np.int32), "run": (-1.0 - 8.0 * rs.rand(rows)).astype(np.float32),
         "seqs": rs.randint(3, 30, (rows, L)).astype(np.int32), "has_complete": np.asarray(has_complete or [0] * n_img, dtype=np.int32),
         "best_score": (-1.0 - 8.0 * rs.rand(n_img)).astype(np.float32), "best_len": rs.randint(2, L, n_img).astype(np.int32),
         "best_seq": rs.randint(3, 30, (n_img, L)).astype(np.int32), "hyp_cnt": np.asarray(hyp_cnt, dtype=np.int32),
         "hyp_score": (-1.0 - 8.0 * rs.rand(rows)).astype(np.float32), "hyp_len": rs.randint(2, L, rows).astype(np.int32),
         "hyp_seq": rs.randint(3, 30, (rows, L)).astype(np.int32)}
    for key, upd in (("run", run), ("hyp_score", hyp_score), ("hyp_len", hyp_len)):
        for i, v in (upd or {}).items():
            f[key][i] = v
    return f


def _fin_cases():
    cs = collections.OrderedDict()
    # image 0: a finished best; 1: nothing finished, run ties (first beam wins); 2: nothing finished, no beam; 3: the last beam is best
    cs["best"] = (0, _fin_state("best", 4, 3, 4, 1, [2, 3, 0, 3], [0] * 4, 1, 0, 0.0, has_complete=[1, 0, 0, 0],
                                run={3: -1.5, 4: -1.5, 5: -2.5, 9: -3.0, 10: -2.0, 11: -1.0}))
    for kind, alpha in ((0, 0.0), (1, 0.7), (2, 0.7)):
        # image 0: two finished before two live, one of them better; 1: two finished tied in score and length; 2: two hypotheses for
        # n_best 4 (length 0, -inf); 3: a full list beside live beams
        cs["nbest_lp%d" % kind] = (1, _fin_state("nbest", 4, 4, 5, 1, [2, 1, 1, 2], [2, 3, 1, 4], 4, kind, alpha, run={0: -0.25},
                                                 hyp_score={4: -3.5, 5: -3.5}, hyp_len={4: 4, 5: 4}))
        # grouped live rows with holes: an empty middle group, an empty image, all groups live
        cs["grouped_lp%d" % kind] = (2, _fin_state("grouped", 3, 6, 5, 3, [[1, 0, 2], [0, 0, 0], [2, 2, 2]], [2, 1, 0], 6, kind, alpha,
                                                   run={0: -2.5, 4: -2.5}))
    return cs


FIN_CASES = _fin_cases()
