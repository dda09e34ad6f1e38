"""Host oracle of stochastic beam search (include/icz.h: icz_*_sample_distinct; Kool et al., ICML 2019), not collected by pytest:
the search stated in float64 numpy, one image at a time, over the step closures of tests/_beam_opts_oracle.py; the Philox uniforms
restated on the host; and a trace of every deciding margin -- per row the g gaps inside the emitted list and at the emission cut, per
image and step the G~ gaps between neighbouring survivors and at the merge cut.  A case whose smallest margin is below GAP_MIN is
not comparable token for token: the device scores g in fp32 (within OWN_ERROR_MAX of float64)."""
import collections

import numpy as np
import torch

import _beam_opts_oracle as bo

STA, END = 1, 2
GAP_MIN = 6e-5                   # the separation tests/_beam_constrained.py keeps: three times OWN_ERROR_MAX
OWN_ERROR_MAX = 2e-5             # fp32 scores against float64
MIN_SHARE = 0.90                 # share of images a whole-decode config must keep above GAP_MIN
RNG_GUMBEL = 8                   # csrc/rng.h
SLOT_STRIDE = 8                  # csrc/sbs_kernels.h: SBS_MAX_N

Hyp = collections.namedtuple("Hyp", "tokens phi G frozen")


# ---- noise ---------------------------------------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of csrc/rng.h on uint32 arrays (counters and keys broadcast against each other) -> four uint64 arrays"""
    M0, M1, W0, W1, MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = np.asarray(k0, dtype=np.uint64), np.asarray(k1, dtype=np.uint64)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def bits_to_uniform(r):
    """u = ((r >> 9) + 0.5) * 2^-23: exact in fp32, strictly inside (0, 1)"""
    return ((np.asarray(r, dtype=np.uint64) >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def _key(seed):
    seed = np.asarray(seed, dtype=np.uint64)
    return seed & np.uint64(0xFFFFFFFF), seed >> np.uint64(32)


def philox_row(seed, step, img, slot, V):
    """the uniforms of tokens 0 .. V-1 of (image, slot) at `step`: counter {v >> 2, img * 8 + slot, step, RNG_GUMBEL}, word v & 3"""
    q = np.arange((V + 3) // 4, dtype=np.uint64)
    k0, k1 = _key(seed)
    r = philox(q, np.full(q.shape, img * SLOT_STRIDE + slot), np.full(q.shape, step), np.full(q.shape, RNG_GUMBEL), k0, k1)
    return bits_to_uniform(np.stack(r, 1).reshape(-1)[:V])


def philox_root(seed, img):
    """the root's uniform: step 0, slot 0, v = 0 (seed and img broadcast)"""
    k0, k1 = _key(seed)
    img = np.asarray(img, dtype=np.uint64)
    z = np.zeros(np.broadcast(img, k0).shape, dtype=np.uint64)
    return bits_to_uniform(philox(z, img * np.uint64(SLOT_STRIDE) + z, z, z + np.uint64(RNG_GUMBEL), k0, k1)[0])


def philox_uniforms(seed, max_len, n_img, n, V):
    """what a Philox run draws, as the explicit arrays: uniforms [max_len, n_img, n, V] and root_uniforms [n_img], fp32"""
    u = np.stack([np.stack([np.stack([philox_row(seed, s, img, slot, V) for slot in range(n)]) for img in range(n_img)])
                  for s in range(1, max_len + 1)])
    return u, philox_root(seed, np.arange(n_img)).astype(np.float32)


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------
def gumbel(u):
    return -np.log(-np.log(np.asarray(u, dtype=np.float64)))


def log1mexp(a):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(a > -np.log(2.0), np.log(-np.expm1(a)), np.log1p(-np.exp(np.minimum(a, 0.0))))


def condition(Tp, g, Z):
    """G~ = -log(exp(-Tp) - exp(-Z) + exp(-g)) in its stable form, float64; g = Z maps to exactly Tp"""
    g = np.asarray(g, dtype=np.float64)
    w = Tp - g + log1mexp(g - Z)
    return Tp - np.maximum(0.0, w) - np.log1p(np.exp(-np.abs(w)))


def condition_naive(Tp, g, Z):
    return -np.log(np.exp(-Tp) - np.exp(-Z) + np.exp(-np.asarray(g, dtype=np.float64)))


def score_row(x, phi, u, T):
    """x [V] fp32 finished logits, u [V] fp32 -> (phi_c, g) float64: lp = x / T - lse(x / T), phi_c = phi + lp, g = phi_c + gumbel(u)"""
    y = x.astype(np.float64) / float(np.float32(T))
    m = y.max()
    lp = y - (m + np.log(np.exp(y - m).sum()))
    phi_c = float(phi) + lp
    with np.errstate(divide="ignore", invalid="ignore"):
        return phi_c, phi_c + gumbel(u)


def top_n(g, n):
    """-> (the at most n largest finite g by (g descending, v ascending), the first one rejected or None)"""
    V = g.shape[0]
    k = min(n + 1, V)
    part = np.argpartition(-g, k - 1)[:k] if k < V else np.arange(V)
    thr = g[part].min()
    pool = np.nonzero(g >= thr)[0]                            # everything tied with the partition's edge too
    pool = pool[np.isfinite(g[pool])]
    order = pool[np.lexsort((pool, -g[pool]))]
    return order[:n], (order[n] if len(order) > n else None)


def image_step(hyps, x, u, n, T, step, gaps=None):
    """One step of one image.  hyps: the occupied slots in order; x [len(hyps), V] fp32 logits (a frozen slot's row is not read);
    u [len(hyps), V] fp32.  Returns (new hyps in slot order, parent slot of each, rows) where rows[slot] = (idx, g, phi_c) of the
    live slot's emitted candidates.  gaps (a list) receives every deciding margin."""
    gaps = [] if gaps is None else gaps
    cands, rows = [], {}
    for slot, h in enumerate(hyps):
        if h.frozen:
            cands.append((h.G, slot, 0, h, True))
            continue
        phi_c, g = score_row(x[slot], h.phi, u[slot], T)
        idx, rejected = top_n(g, n)
        rows[slot] = (idx, g[idx], phi_c[idx])
        if len(idx) == 0:
            continue
        gaps.extend(np.diff(-g[idx]).tolist())
        if rejected is not None:
            gaps.append(float(g[idx[-1]] - g[rejected]))
        Gt = condition(h.G, g[idx], g[idx[0]])
        for v, gt, pc in zip(idx, Gt, phi_c[idx]):
            v = int(v)
            cands.append((float(gt), slot, v, Hyp(h.tokens + [v], float(pc), float(gt), v == END), False))
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))
    for a, b in zip(cands[:n], cands[1:n + 1]):
        if not (a[4] and b[4]):                               # two frozen hypotheses carry their G unchanged: an exact comparison
            gaps.append(a[0] - b[0])
    keep = cands[:n]
    return [c[3] for c in keep], [c[1] for c in keep], rows


def search(step, state, n, max_len, T, noise, u_root, gaps=None, all_steps=False):
    """step(prev (rows,), state) -> (logits (rows, V), state), state a tuple of tensors indexed by row (its first row is used).
    noise(s, slot) -> u [V] fp32 of this image at step s = 1 ..; u_root: the root's uniform.  Returns the image's hypotheses in slot
    order (G descending): [Hyp(tokens without <sta>, phi, G, frozen)].  The search ends once every hypothesis is frozen unless
    all_steps (the result is the same: the early-out of the device)."""
    hyps = [Hyp([], 0.0, float(gumbel(np.float32(u_root))), False)]
    state = tuple(x[:1] for x in state)
    with torch.no_grad():
        for s in range(1, max_len + 1):
            if all(h.frozen for h in hyps) and not all_steps:
                break
            prev = torch.tensor([0 if h.frozen else (h.tokens[-1] if h.tokens else STA) for h in hyps], dtype=torch.long)
            logits, state = step(prev, state)
            u = np.stack([noise(s, slot) for slot in range(len(hyps))])
            hyps, parents, _ = image_step(hyps, logits.numpy(), u, n, T, s, gaps)
            state = tuple(x[torch.tensor(parents, dtype=torch.long)] for x in state)
    return hyps


def search_model(model, feats1, p, n, max_len, T, noise, u_root, gaps=None):
    with torch.no_grad():
        step, state, _ = bo.CLOSURES[model](feats1, p, 1)
    return search(step, state, n, max_len, T, noise, u_root, gaps)


def explicit_noise(u, img):
    """noise() over explicit uniforms [max_len, n_img, n, V]"""
    return lambda s, slot: u[s - 1, img, slot]


def philox_noise(seed, img, V):
    return lambda s, slot: philox_row(seed, s, img, slot, V)


def outputs(hyps, n, max_len):
    """the device's outputs of one image: ids [n, max_len] int64, lens, finished, phi, G"""
    ids = np.zeros((n, max_len), np.int64)
    lens, fin = np.zeros(n, np.int32), np.zeros(n, np.int32)
    phi, G = np.full(n, -np.inf), np.full(n, -np.inf)
    for j, h in enumerate(hyps):
        ids[j, :len(h.tokens)] = h.tokens
        lens[j], fin[j], phi[j], G[j] = len(h.tokens), int(h.frozen), h.phi, h.G
    return ids, lens, fin, phi, G


# ---- a toy model with an exact answer: V = 4, <end> = 2, the logits a fixed table indexed by a hash of the prefix ------------------
TOY_V = 4
_TOY_TABLE = np.random.RandomState(7).uniform(-1.5, 1.5, (97, TOY_V)).astype(np.float32)


def toy_closure():
    def step(prev, st):
        h = (st[0] * 5 + prev + 1) % 97
        return torch.from_numpy(_TOY_TABLE[h.numpy()]), (h,)
    return step, (torch.zeros(1, dtype=torch.long),)


def toy_leaves(max_len, T=1.0):
    """every sequence the toy model can produce within max_len steps -> {tuple(tokens): probability}, float64"""
    step, state = toy_closure()
    out = {}

    def walk(tokens, st, logp):
        prev = torch.tensor([tokens[-1] if tokens else STA])
        logits, st2 = step(prev, st)
        y = logits.numpy()[0].astype(np.float64) / float(np.float32(T))
        lp = y - np.log(np.exp(y).sum())
        for v in range(TOY_V):
            t = tokens + [v]
            if v == END or len(t) == max_len:
                out[tuple(t)] = np.exp(logp + lp[v])
            else:
                walk(t, st2, logp + lp[v])
    walk([], state, 0.0)
    return out


# ---- the configurations of the GPU tests; tests/test_cpu_sample_distinct.py asserts their margins on the oracle alone -------------
# whole decodes at the golden dims (tests/test_gpu_sample_distinct.py): (golden, regime, n, temperature, seed of the explicit noise)
DECODE_LEN = 12
DECODE_GOLDENS = [("butd_dec_tiny", "nat"), ("aoa_tiny", "track"), ("nic_dec_tiny", "track")]
DECODE_NT = [(n, T) for n in (1, 3, 5, 8) for T in (1.0, 0.7)]


def decode_noise(seed, n_img, n, V, max_len=DECODE_LEN):
    """explicit uniforms of a whole-decode config, strictly inside (0, 1): (u [max_len, n_img, n, V], root [n_img]) fp32"""
    rs = np.random.RandomState(seed)
    u = bits_to_uniform(rs.randint(0, 2 ** 32, (max_len, n_img, n, V), dtype=np.uint64))
    return u, bits_to_uniform(rs.randint(0, 2 ** 32, n_img, dtype=np.uint64))


# ======================================================================================================================
# One step on a given state (icz_test_sbs_rowtopk / icz_test_sbs_step), float64.  Logits in [-16, 16], |phi| <= 16; rows the kernels
# must not read (frozen, unoccupied) hold NaN logits.  Every case's seed was searched on the CPU so that all its margins are above
# GAP_MIN (tests/test_cpu_sample_distinct.py asserts it): no comparison of the GPU test is excused.
StepCase = collections.namedtuple("StepCase", "name n_img n V ld nsplit step compact T special")
CANARY = -777


def pad64(V):
    return (V + 63) & ~63


def _step_cases():
    cs = []
    add = lambda *a, special=None: cs.append(StepCase(*a, special))      # noqa: E731
    # shapes: every vocabulary, padded and unpadded rows, 1 / 2 / 4 slabs, every n, every temperature; seeds filled in below
    add("v53_n1", 3, 1, 53, 53, 1, 4, 0, 1.0)
    add("v53_n2_pad_s2", 3, 2, 53, 64, 2, 3, 0, 0.5)
    add("v53_n5", 2, 5, 53, 53, 1, 5, 0, 2.0)
    add("v53_n8_s4", 2, 8, 53, 64, 4, 6, 0, 1.0)
    add("v1000_n5_pad", 3, 5, 1000, 1024, 1, 3, 0, 1.0)
    add("v1000_n2_s2", 2, 2, 1000, 1000, 2, 2, 0, 2.0)
    add("v1000_n8_s4", 2, 8, 1000, 1024, 4, 7, 0, 0.5)
    add("v10102_n5_s2", 2, 5, 10102, 10112, 2, 4, 0, 1.0)
    add("v10102_n8", 2, 8, 10102, 10102, 1, 3, 0, 0.5)
    add("v10102_n1_s4", 3, 1, 10102, 10112, 4, 9, 0, 2.0)
    # step 1: only slot 0 is occupied; one logits row per image (compact) or per decoder row
    add("step1_compact_n5", 3, 5, 1000, 1024, 2, 1, 1, 1.0, special="step1")
    add("step1_compact_n8", 2, 8, 53, 53, 1, 1, 1, 0.5, special="step1")
    add("step1_rows_n5", 2, 5, 53, 64, 1, 1, 0, 1.0, special="step1")
    # a row with only 3 finite logits at n = 5: fewer candidates, an empty slot downstream
    add("finite3", 2, 5, 53, 64, 1, 3, 0, 1.0, special="finite3")
    # <end> among the winners: the new hypothesis is frozen on entry
    add("end_wins", 3, 5, 1000, 1024, 1, 4, 0, 1.0, special="end")
    # an image whose rows are all frozen beside a live one
    add("all_frozen", 2, 5, 53, 53, 1, 5, 0, 1.0, special="all_frozen")
    # two frozen rows of equal G: resolved to the lower slot
    add("tie_frozen", 2, 5, 53, 64, 2, 5, 0, 1.0, special="tie_frozen")
    return cs


STEP_SEEDS = {}                  # name -> seed, filled at the bottom of this file


def step_inputs(c, seed=None):
    """the state before the step and its inputs, numpy: slabs [nsplit, R, ld] with bias [ld] (finished logits x [R, V] = the fp32 sum in
    slab order + bias), uniforms [n_img, n, V], occ, frozen, phi, G, len, seqs [rows, L]"""
    rs = np.random.RandomState((STEP_SEEDS[c.name] if seed is None else seed) + 1000 * (sum(map(ord, c.name)) % 997))
    rows, L = c.n_img * c.n, c.step + 2
    R = c.n_img if c.compact else rows
    occ = np.ones(c.n_img, np.int32) if c.step == 1 else rs.randint(1, c.n + 1, c.n_img).astype(np.int32)
    frozen = np.zeros(rows, np.uint8)
    phi = np.full(rows, np.nan, np.float32)
    G = np.full(rows, np.nan, np.float64)
    ln = np.full(rows, CANARY, np.int32)
    seqs = np.full((rows, L), CANARY, np.int32)
    if c.special == "all_frozen":
        occ[0] = c.n
    if c.special in ("tie_frozen", "finite3", "end"):
        occ[:] = np.maximum(occ, min(c.n, 3))
    if c.special == "finite3":
        occ[0] = 1                                             # image 0: one live row with 3 finite logits -> 3 occupied slots of 5
    for img in range(c.n_img):
        g = 1.0 - np.cumsum(rs.uniform(0.3, 1.5, c.n))
        for slot in range(int(occ[img])):
            row = img * c.n + slot
            G[row] = g[slot] if c.step > 1 else gumbel(bits_to_uniform(rs.randint(0, 2 ** 32, dtype=np.uint64)))
            phi[row] = 0.0 if c.step == 1 else np.float32(rs.uniform(-16.0, 0.0))
            fz = c.step > 2 and rs.rand() < 0.3
            if c.special == "all_frozen" and img == 0:
                fz = True
            if c.special == "tie_frozen" and slot in (1, 2):
                fz = True
                G[row] = G[img * c.n + 1]
            if c.special in ("finite3", "end") and slot == 0:
                fz = False
            frozen[row] = fz
            ln[row] = rs.randint(1, c.step - 1) if fz else c.step - 1
            seqs[row, :ln[row]] = rs.randint(3, c.V, ln[row])
            if fz:
                seqs[row, ln[row] - 1] = END
    slabs = rs.uniform(-16.0 / c.nsplit, 16.0 / c.nsplit, (c.nsplit, R, c.ld)).astype(np.float32)
    bias = rs.uniform(-0.5, 0.5, c.ld).astype(np.float32) if c.nsplit > 1 else np.zeros(c.ld, np.float32)
    if c.nsplit > 1:
        slabs *= np.float32(15.5 / 16.0)
    if c.special == "finite3":
        keep = rs.choice(np.arange(3, c.V), 3, replace=False)
        r0 = 0                                                 # image 0, slot 0
        for z in range(c.nsplit):
            row = slabs[z, r0].copy()
            slabs[z, r0] = -np.inf
            slabs[z, r0, keep] = row[keep]
    if c.special == "end":
        slabs[:, ::c.n] *= np.float32(0.25)                    # slot 0 of every image: <end> is by far its best token
        slabs[:, ::c.n, END] = 16.0 / c.nsplit
    x = slabs[0].copy()
    for z in range(1, c.nsplit):
        x = x + slabs[z]
    if c.nsplit > 1:
        x = x + bias
    for row in range(rows):                                    # rows the kernel must not read
        img, slot = divmod(row, c.n)
        if (slot >= occ[img] or frozen[row]) and not c.compact:
            slabs[:, row] = np.nan
            x[row] = np.nan
    u = bits_to_uniform(rs.randint(0, 2 ** 32, (c.n_img, c.n, c.V), dtype=np.uint64))
    return {"slabs": slabs, "bias": bias, "x": x[:, :c.V], "uniforms": u, "occ": occ, "frozen": frozen, "phi": phi, "G": G, "len": ln, "seqs": seqs,
            "L": L}


def step_ref(c, inp, gaps=None):
    """the state after the step, float64: cand {row: (idx, g, phi_c)} and the arrays the merge writes (CANARY / NaN: not written)"""
    rows, L = c.n_img * c.n, inp["L"]
    out = {"cand": {}, "occ": inp["occ"].copy(), "frozen": inp["frozen"].copy(), "phi": inp["phi"].astype(np.float64), "G": inp["G"].copy(),
           "len": inp["len"].copy(), "seqs_out": np.full((rows, L), CANARY, np.int32), "src_row": np.full(rows, CANARY, np.int32),
           "it_next": np.full(rows, CANARY, np.int64), "n_live": 0, "parent_rank": {}}
    for img in range(c.n_img):
        row0, oc = img * c.n, int(inp["occ"][img])
        hyps = [Hyp(inp["seqs"][row0 + s, :inp["len"][row0 + s]].tolist(), float(inp["phi"][row0 + s]), float(inp["G"][row0 + s]),
                    bool(inp["frozen"][row0 + s])) for s in range(oc)]
        x = inp["x"][img:img + 1] if c.compact else inp["x"][row0:row0 + oc]
        new, parents, cand = image_step(hyps, x, inp["uniforms"][img, :oc], c.n, c.T, c.step, gaps)
        for slot, e in cand.items():
            out["cand"][row0 + slot] = e
        out["occ"][img] = len(new)
        for j in range(c.n):
            row = row0 + j
            if j < len(new):
                h, par = new[j], parents[j]
                carried = hyps[par].frozen
                out["phi"][row], out["G"][row], out["frozen"][row], out["len"][row] = h.phi, h.G, h.frozen, len(h.tokens)
                out["seqs_out"][row, :len(h.tokens)] = h.tokens
                out["src_row"][row] = row0 + par
                out["it_next"][row] = 0 if h.frozen else h.tokens[-1]
                out["n_live"] += not h.frozen
                if not carried:
                    out["parent_rank"][row] = (row0 + par, int(np.nonzero(cand[par][0] == h.tokens[-1])[0][0]))
            else:
                out["src_row"][row], out["it_next"][row] = row, 0
    return out


STEP_CASES = _step_cases()
STEP_SEEDS.update({c.name: 0 for c in STEP_CASES})       # searched: seed 0 separates every case by more than 2 GAP_MIN


# ---- whole decodes: the oracle's hypotheses and smallest margin per (config, image), computed once per process ---------------------
DECODE_SEEDS = {}                # (golden, n, T) -> seed of the explicit noise; filled below
_DECODES = {}


def decode_pair(golden_dir, name, regime, n, T, img, seed=None):
    """-> (the oracle's hypotheses of image `img` under the config's explicit noise, the smallest of its margins)"""
    import _beam_constrained as bc
    seed = DECODE_SEEDS.get((name, n, T), 0) if seed is None else seed
    key = (name, regime, n, T, img, seed)
    if key not in _DECODES:
        model, p, feats = bc.golden_case(golden_dir, name, regime)
        V = bo.CLOSURES[model](feats[:1], p, 1)[2]
        u, root = decode_noise(seed, feats.shape[0], n, V)
        gaps = []
        hyps = search_model(model, feats[img:img + 1], p, n, DECODE_LEN, T, explicit_noise(u, img), root[img], gaps)
        _DECODES[key] = (hyps, min(gaps) if gaps else float("inf"))
    return _DECODES[key]


# searched on the CPU: with these seeds every image of every config keeps all its margins above 2 GAP_MIN (seed 0 elsewhere)
DECODE_SEEDS.update({("butd_dec_tiny", 8, 1.0): 3, ("nic_dec_tiny", 8, 1.0): 1})


def philox_pair(golden_dir, name, regime, n, T, img, seed):
    """decode_pair under the Philox noise of `seed` (image `img` of the batch)"""
    import _beam_constrained as bc
    key = ("philox", name, regime, n, T, img, seed)
    if key not in _DECODES:
        model, p, feats = bc.golden_case(golden_dir, name, regime)
        V = bo.CLOSURES[model](feats[:1], p, 1)[2]
        gaps = []
        hyps = search_model(model, feats[img:img + 1], p, n, DECODE_LEN, T, philox_noise(seed, img, V), philox_root(seed, img), gaps)
        _DECODES[key] = (hyps, min(gaps) if gaps else float("inf"))
    return _DECODES[key]


# Further comparisons of tests/test_gpu_sample_distinct.py that are token for token; searched on the CPU so that EVERY image keeps all
# its margins above 2 GAP_MIN (tests/test_cpu_sample_distinct.py asserts GAP_MIN), so each of them compares all three images:
PHILOX_SEEDS = {"butd_dec_tiny": 2, "aoa_tiny": 1, "nic_dec_tiny": 1}      # Philox runs at T = 1, n = 1, 3, 5, 8: the prefix property
BATCH_NT, BATCH_SEED = (3, 0.7), 100                                       # explicit noise: a batch = its images one by one
COPIES_NT, COPIES_SEEDS = (3, 1.0), {"butd_dec_tiny": 201, "aoa_tiny": 200, "nic_dec_tiny": 200}      # regime "nat": copies = the single model
