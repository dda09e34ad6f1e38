"""Case tables, float64 references and a-priori bounds of the kernels in csrc/lstm_kernels.h, each on its own: embed_kernel,
embed_steps_kernel, lstm_point_kernel, lstm_point_gw_kernel and lstm_bwd_point_kernel (tests/test_cpu_lstm_kernels.py holds every
case to its stated purpose and every reference to a scalar loop on the host; tests/test_gpu_lstm_kernels.py runs the tables through the
icz_test_* entries).  Plain numpy, no pytest, no torch; not collected by pytest.

A case is name -> shape -> purpose; the purpose is data written out by hand here (which slab loops of the gate-per-wave kernel run,
how many workgroups, how many lane-quads of the last one hold a unit, which kernel route 0 takes), so that the CPU test can recompute
it from the shape.

The embedding kernels and the dropped copy of h' are exact operations (gather, relu, keep, double): compared by value with ==.
Everything else has an a-priori bound, derived and never fitted (u = 2^-24, one rounding per fp32 operation on the element's path;
a contracted multiply-add rounds once where the bound counts two):
  p        the pre-activation gate, a sum: (additions + 2) u sum|addends|, the rule of tests/_support_kernels.py; additions = one per
           slab, one for pre, two for the biases
  expf, tanhf, the division in sigmoidf_   3, 5 and 2.5 ulp (the OpenCL-conformance limits), 1 ulp = 2 u relative: 6 u, 10 u, 5 u
  sig(p)   1 / (1 + e): 6 u (1 - sig) from e, u from the addition, 5 u from the division: 12 u relative, and e_p sig (1 - sig) from p
  tanh(p)  10 u relative and e_p (1 - tanh^2)
  c'       f c + i g: the gates' errors times their partners, and 2 u (|f c| + |i g|) for two products and a sum
  h'       o tanh(c'): e_o |tanh c'| + |o| (e_c' (1 - tanh^2 c') + 10 u |tanh c'|) + u |h'|
  dh       a sum again: one addition per slab of a present set, one to join each set, one for the dropped-output term
  dc, d gates, dc_prev   as tests/test_gpu_bptt_fused_step.py derives them: 1 - tanh^2 is off by 22 u absolutely, 1 - g^2 by 2 u, four
           resp. five roundings of the result's magnitude; where the gates and c' are themselves computed (the chained case) their
           bounds enter through the partial derivatives
All of it is first order; the second-order terms are below e times the first-order ones with e < 1e-4 the largest relative error in
play, and the factor SECOND = 1 + 2^-10 on every bound covers them.  Every reference returns (value, bound) pairs as float64 arrays."""
import collections

import numpy as np

from _philox import RNG_EMB, RNG_OUT, _keep_bits
from _support_kernels import GUARD, U, seeded  # noqa: F401

EXP_U, TANH_U, DIV_U = 6.0, 10.0, 5.0            # 3, 5 and 2.5 ulp
SIG_U = EXP_U + 1.0 + DIV_U
SECOND = 1.0 + 2.0 ** -10
MASK_BYTES = (0, 1, 2, 255)
SEED = 0x1234ABCD5678EF01
WIDE_OFF, WIDE_PAD = 5, 9                         # a wide slab set: rows of H + 9 floats read from column 5


def cdiv(a, b):
    return -(-a // b)


# ======================================================================================================================
# dropout: which elements a kernel keeps.  -1 = passes unchanged (mode 0, rows in front of row0), 0 = dropped, 1 = kept and doubled
def keep_flags(mode, mask, seed, stream, step, n):
    if mode == 1:
        return (np.asarray(mask[:n]) != 0).astype(np.int8)
    return _keep_bits(seed, stream, step, n).astype(np.int8)


def row_keep(mode, row0, rows, width, mask, seed, stream, step, at_row=False):
    """[rows, width]; at_row: the WRONG index row * width + j for the rows behind row0 (the backward's index used by the forward)"""
    k = np.full((rows, width), -1, dtype=np.int8)
    if mode == 0:
        return k
    flags = keep_flags(mode, mask, seed, stream, step, rows * width).reshape(rows, width)
    for r in range(row0, rows):
        k[r] = flags[r if at_row else r - row0]
    return k


def apply_keep(x, k):
    """x doubled where kept, zero where dropped, itself where it passes (exact in any binary format)"""
    return np.where(k < 0, x, np.where(k > 0, x * 2, x * 0))


# ======================================================================================================================
# embed_kernel / embed_steps_kernel
EMB_V, EMB_ROWS = 7, 5
EMB_TOKENS = (0, EMB_V - 1, 3, 3, 0)              # the first and the last table row, and repeats
EMB_E = (4, 12, 1020, 1024, 1028, 2052)
# E -> (workgroups per row, 16-byte groups in the last one): 1024 columns per workgroup
EMB_GEOMETRY = {4: (1, 1), 12: (1, 3), 1020: (1, 255), 1024: (1, 256), 1028: (2, 1), 2052: (3, 1)}
EMB_STEP = 3
EmbCase = collections.namedtuple("EmbCase", "name E relu mode row0 live purpose")


def _emb_cases():
    out = []
    for relu in (0, 1):                            # the full table at the smallest width
        for mode in (0, 1, 2):
            for row0 in (0, 2):
                for live in (None, 1, 0):
                    out.append(EmbCase("E4_relu%d_mode%d_row0%d_live%s" % (relu, mode, row0, live), 4, relu, mode, row0, live, {"wgs": 1, "last": 1}))
    for E in EMB_E[1:]:                            # the wider rows: what the width exists for, and one case per mode
        wgs, last = EMB_GEOMETRY[E]
        out.append(EmbCase("E%d_philox" % E, E, 1, 2, 2, None, {"wgs": wgs, "last": last}))
        out.append(EmbCase("E%d_mask" % E, E, 0, 1, 0, 1, {"wgs": wgs, "last": last}))
        out.append(EmbCase("E%d_dead" % E, E, 1, 0, 0, 0, {"wgs": wgs, "last": last}))
    return out


EMB_CASES = _emb_cases()
# (E, rows, table offset in floats, emb offset in floats, null): refused on the host
EMB_REFUSED = [(0, 5, 0, 0, None), (2, 5, 0, 0, None), (6, 5, 0, 0, None), (8, 0, 0, 0, None), (8, -1, 0, 0, None), (8, 5, 1, 0, None), (8, 5, 0, 1, None),
               (8, 5, 0, 0, "table"), (8, 5, 0, 0, "it"), (8, 5, 0, 0, "emb")]


def emb_table(E):
    """[V, E] fp32 with both signs in every row, row 0 included"""
    t = seeded("emb table %d" % E).standard_normal((EMB_V, E)).astype(np.float32)
    t[:, 0], t[:, 1] = np.abs(t[:, 0]) + 0.5, -np.abs(t[:, 1]) - 0.5
    return t


def emb_mask(name, n):
    return seeded("emb mask " + name).choice(MASK_BYTES, size=n).astype(np.uint8)


def embed_ref(table, tok, relu, keep):
    """fp32, exact: gather, relu, then x 2 where kept, else 0"""
    x = table[np.asarray(tok)]
    if relu:
        x = np.maximum(x, np.float32(0))
    return apply_keep(x, keep).astype(np.float32)


StepsCase = collections.namedtuple("StepsCase", "name T B E rows_t mode purpose")
ST_B = 5
ST_CASES = [StepsCase("T%d_E%d_mode%d" % (T, E, mode), T, ST_B, E, rows_t, mode, {"wgs": EMB_GEOMETRY[E][0], "last_t": T - 1, "ragged": ragged})
            for T, rows_t, ragged in ((1, (5,), False), (4, (5, 5, 3, 1), True), (128, (5,) * 40 + (3,) * 60 + (1,) * 28, True))
            for E in ((4, 1028) if T == 4 else (4,))
            for mode in (0, 1, 2)]
# (T, B, rows_t): refused on the host
ST_REFUSED = [(0, 5, ()), (129, 5, (5,) * 129), (2, 5, (5, 6)), (2, 5, (6, 5)), (3, 5, (3, 4, 1)), (2, 5, (3, -1)), (2, 0, (0, 0))]


def steps_tokens(c):
    tok = seeded("steps tok " + c.name).randint(0, EMB_V, size=(c.T, c.B)).astype(np.int64)
    tok[0, 0], tok[0, 1], tok[-1, 0] = 0, EMB_V - 1, 0           # the first and the last table row, in rows that every step keeps
    return tok


def steps_keep(c, mask, t):
    """keep of step t: the slice t of a mask [T, B, E] / Philox step t, element b E + e"""
    return row_keep(c.mode, 0, c.B, c.E, None if mask is None else mask[t].reshape(-1), SEED, RNG_EMB, t)


def steps_ref(c, table, tok, mask):
    """[T, B, E] fp32 with GUARD in the rows b >= rows_t[t], which the kernel leaves alone"""
    out = np.full((c.T, c.B, c.E), GUARD, dtype=np.float32)
    for t in range(c.T):
        n = c.rows_t[t]
        out[t, :n] = embed_ref(table, tok[t], 1, steps_keep(c, mask, t))[:n]
    return out


# ======================================================================================================================
# the forward LSTM kernels
FWD_H = (4, 20, 252, 256, 260, 516)               # one quad, a partial wave, the last lane-quad of a workgroup, one workgroup, a second
FWD_H_ROUTE1 = (5, 255, 257)                      # workgroup of one quad (twice); the one-unit kernel alone: no whole groups of 4
FWD_NS = (1, 3, 4, 5, 8, 12, 13, 16, 29)
# ns -> trips of the gate-per-wave kernel's three slab loops (eight, four, one at a time)
NS_LOOPS = {1: (0, 0, 1), 3: (0, 0, 3), 4: (0, 1, 0), 5: (0, 1, 1), 8: (1, 0, 0), 12: (1, 1, 0), 13: (1, 1, 1), 16: (2, 0, 0), 29: (3, 1, 1)}
# H -> (workgroups per row, threads of the last one that hold a hidden unit, lane-quads per wave of the last one that do)
H_GEOMETRY = {4: (1, 4, 1), 5: (1, 5, 0), 20: (1, 20, 5), 252: (1, 252, 63), 255: (1, 255, 0), 256: (1, 256, 64), 257: (2, 1, 0), 260: (2, 4, 1),
              516: (3, 4, 1)}
FWD_STEP = 6
GATHER_ROWS, GATHER_N_PRE = (2, 0, 2, 1, 0), 3     # pre_row of five decoder rows: three parents, two of them twice
FwdCase = collections.namedtuple("FwdCase", "name rows H ns pre gates_out hdrop_out mode row0 live routes purpose")


def _fwd(name, rows, H, ns, pre=None, gates_out=True, hdrop_out=True, mode=0, row0=0, live=None):
    wgs, units, quads = H_GEOMETRY[H]
    routes = (1, 2) if H % 4 == 0 else (1,)
    return FwdCase(name, rows, H, ns, pre, gates_out, hdrop_out, mode, row0, live, routes,
                   {"loops": NS_LOOPS[ns], "wgs": wgs, "units": units, "quads": quads, "route0": 2 if H % 4 == 0 else 1})


def _fwd_cases():
    out = []
    for ns in FWD_NS:                              # every slab count x rows x pre at the smallest width
        for rows in (1, 5):
            for pre in (None, "identity", "gather"):
                if pre == "gather" and rows == 1:
                    continue
                out.append(_fwd("H4_ns%d_rows%d_%s" % (ns, rows, pre), rows, 4, ns, pre))
    for g, hd in ((True, True), (True, False), (False, True), (False, False)):      # the switches, crossed, at the smallest width
        for mode in (0, 1, 2):
            for row0 in (0, 2):
                for live in (None, 1, 0):
                    out.append(_fwd("H4_g%d_hd%d_mode%d_row0%d_live%s" % (g, hd, mode, row0, live), 5, 4, 5, "gather", g, hd, mode, row0, live))
    for H in FWD_H[1:] + FWD_H_ROUTE1:             # the widths: lanes and workgroups past H, with every loop, a gather, dropout, a dead step
        out.append(_fwd("H%d_one_slab" % H, 1, H, 1))
        out.append(_fwd("H%d_all_loops" % H, 5, H, 13, "gather", True, True, 2, 2, 1))
        out.append(_fwd("H%d_mask" % H, 5, H, 4, "identity", True, True, 1, 0, None))
        out.append(_fwd("H%d_dead" % H, 5, H, 8, None, True, True, 0, 0, 0))
        out.append(_fwd("H%d_dead_tail" % H, 1, H, 3, None, True, True, 0, 0, 0))
    return out


FWD_CASES = _fwd_cases()
FWD_BY_NAME = {c.name: c for c in FWD_CASES}
FWD_MUTATIONS = ("no_b_hh", "last_slab", "swap_fg", "c_prev_next", "pre_row_ignored", "keep_at_row")


def fwd_mutation_applies(c, mut):
    if c.live == 0:
        return False
    if mut == "pre_row_ignored":
        return c.pre == "gather"
    if mut == "keep_at_row":
        return c.mode != 0 and c.row0 > 0 and c.hdrop_out
    if mut == "c_prev_next":
        return c.H >= 2
    return True


def fwd_inputs(c):
    """fp32 operands: pre-activations of order one whatever the slab count (every addend is drawn at 1 / sqrt(addends))"""
    rs = seeded("fwd " + c.name)
    G = 4 * c.H
    n_add = c.ns + (1 if c.pre else 0) + 2
    sc = 1.0 / np.sqrt(n_add)
    n_pre = 0 if not c.pre else (GATHER_N_PRE if c.pre == "gather" else c.rows)
    d = {"slab": rs.standard_normal((c.ns, c.rows, G)) * sc, "b_ih": rs.standard_normal(G) * sc, "b_hh": rs.standard_normal(G) * sc,
         "c_prev": rs.standard_normal((c.rows, c.H))}
    if c.pre:
        d["pre"] = rs.standard_normal((n_pre, G)) * sc
    d = {k: v.astype(np.float32) for k, v in d.items()}
    if c.pre == "gather":
        assert c.rows == len(GATHER_ROWS)
        d["pre_row"] = np.asarray(GATHER_ROWS, dtype=np.int32)
    d["mask"] = rs.choice(MASK_BYTES, size=c.rows * c.H).astype(np.uint8)      # rows * H flags: the kernel reads the first (rows - row0) * H
    return d


def sigmoid_ref(p, e_p):
    s = 1.0 / (1.0 + np.exp(-p))
    return s, e_p * s * (1.0 - s) + SIG_U * U * s


def tanh_ref(p, e_p):
    t = np.tanh(p)
    return t, e_p * (1.0 - t * t) + TANH_U * U * np.abs(t)


def fwd_ref(c, d, mut=None):
    """float64 cell on the fp32 operands -> {"gates", "c", "h", "hdrop"}: (value, bound), and "keep" [rows, H] (row_keep)"""
    H, rows = c.H, c.rows
    slab = d["slab"].astype(np.float64)
    if mut == "last_slab":
        slab = slab[:-1] if c.ns > 1 else slab * 0
    terms = list(slab)
    if c.pre:
        pr = d["pre_row"] if c.pre == "gather" else np.arange(rows)
        if mut == "pre_row_ignored":
            pr = np.minimum(np.arange(rows), d["pre"].shape[0] - 1)
        terms.append(d["pre"].astype(np.float64)[pr])
    terms.append(np.broadcast_to(d["b_ih"].astype(np.float64), (rows, 4 * H)))
    if mut != "no_b_hh":
        terms.append(np.broadcast_to(d["b_hh"].astype(np.float64), (rows, 4 * H)))
    p = sum(terms)
    adds = c.ns + (1 if c.pre else 0) + 2
    e_p = (adds + 2) * U * sum(np.abs(t) for t in terms)
    q = [p[:, k * H:(k + 1) * H] for k in range(4)]
    e = [e_p[:, k * H:(k + 1) * H] for k in range(4)]
    if mut == "swap_fg":
        q[1], q[2], e[1], e[2] = q[2], q[1], e[2], e[1]
    gi, e_i = sigmoid_ref(q[0], e[0])
    gf, e_f = sigmoid_ref(q[1], e[1])
    gg, e_g = tanh_ref(q[2], e[2])
    go, e_o = sigmoid_ref(q[3], e[3])
    cp = d["c_prev"].astype(np.float64)
    if mut == "c_prev_next":
        cp = np.roll(cp, -1, axis=1)
    cn = gf * cp + gi * gg
    e_c = e_f * np.abs(cp) + e_i * np.abs(gg) + e_g * np.abs(gi) + 2 * U * (np.abs(gf * cp) + np.abs(gi * gg))
    tc = np.tanh(cn)
    hn = go * tc
    e_h = e_o * np.abs(tc) + np.abs(go) * (e_c * (1.0 - tc * tc) + TANH_U * U * np.abs(tc)) + U * np.abs(hn)
    keep = row_keep(c.mode, c.row0, rows, H, d["mask"], SEED, RNG_OUT, FWD_STEP, at_row=(mut == "keep_at_row"))
    out = {"gates": (np.concatenate([gi, gf, gg, go], 1), np.concatenate([e_i, e_f, e_g, e_o], 1) * SECOND), "c": (cn, e_c * SECOND),
           "h": (hn, e_h * SECOND), "hdrop": (apply_keep(hn, keep), np.where(keep < 0, 1.0, np.where(keep > 0, 2.0, 0.0)) * e_h * SECOND),
           "keep": keep}
    return out


# ======================================================================================================================
# lstm_bwd_point_kernel
BWD_H = (4, 20, 255, 257, 516)
BWD_ROWS = (1, 5, 65)
BWD_STEP = 6
FLAGS = ((None, None), (1, 1), (1, 0), (0, 1))     # (live, carry_live), the four of tests/test_gpu_bptt_fused_step.py
# the three slab sets of a case: per set None (absent) or (slabs, wide rows, fewer rows than the step)
BWD_SETS = collections.OrderedDict([
    ("a", ((1, False, False), None, None)),                                   # NIC's image step (with no dhdrop) and the language LSTM (with it)
    ("a4", ((4, False, True), None, None)),
    ("ab", ((5, False, True), (1, True, False), None)),
    ("abc_145", ((1, False, False), (4, True, False), (5, False, False))),
    ("abc_514", ((5, True, True), (1, False, False), (4, True, True))),
    ("abc_451", ((4, False, False), (5, True, True), (1, False, False))),
    ("bc", (None, (4, False, False), (1, True, False))),
    ("ac", ((1, True, False), None, (5, False, True))),
    ("c", (None, None, (4, False, False))),
])
BwdCase = collections.namedtuple("BwdCase", "name rows H sets dhdrop mode dc_in c_prev live carry_live purpose")
# dc_in: None (absent), "fewer" (dc_in_rows below rows), "all"


def _fewer(rows):
    return max(1, rows // 2)


def _bwd(name, rows, H, sets, dhdrop=False, mode=0, dc_in=None, c_prev=True, live=None, carry_live=None):
    wgs, units, _ = H_GEOMETRY[H]
    return BwdCase(name, rows, H, sets, dhdrop, mode, dc_in, c_prev, live, carry_live,
                   {"slabs": tuple(0 if s is None else s[0] for s in BWD_SETS[sets]), "wgs": wgs, "units": units})


def _bwd_cases():
    out = []
    for sets in BWD_SETS:                          # every arrangement of the sets x rows x flags at the smallest width
        for rows in BWD_ROWS:
            for i, (live, carry) in enumerate(FLAGS):
                dc_in = (None, "fewer", "all")[(i + rows) % 3] if sets != "a" else ("all" if i else None)
                out.append(_bwd("H4_%s_rows%d_live%s_carry%s" % (sets, rows, live, carry), rows, 4, sets, dhdrop=(i % 2 == 1), mode=0, dc_in=dc_in,
                                c_prev=(i != 2), live=live, carry_live=carry))
    for mode in (0, 1, 2):                          # dropout x c_prev x dc_in with all three sets present
        for c_prev in (True, False):
            for dc_in in (None, "fewer", "all"):
                out.append(_bwd("H4_drop_mode%d_cp%d_dc%s" % (mode, c_prev, dc_in), 5, 4, "abc_514", True, mode, dc_in, c_prev, 1, 1))
    for mode in (0, 1, 2):                          # the language LSTM's shape: set a and dhdrop only
        out.append(_bwd("H4_lm_mode%d" % mode, 5, 4, "a", True, mode, "all", True, None, None))
    out.append(_bwd("H4_nic_image", 5, 4, "a", False, 0, None, False, None, None))      # NIC's image step: set a only, no state in front
    for H in BWD_H[1:]:                            # the widths
        out.append(_bwd("H%d_lm_philox" % H, 5, H, "a4", True, 2, "fewer", True, 1, 1))
        out.append(_bwd("H%d_nic_image" % H, 1, H, "a", False, 0, None, False, None, None))
        out.append(_bwd("H%d_three_sets_mask" % H, 65, H, "abc_514", True, 1, "all", True, None, None))
        out.append(_bwd("H%d_carry_dead" % H, 5, H, "ab", True, 0, "all", True, 1, 0))
        out.append(_bwd("H%d_dead" % H, 5, H, "abc_145", True, 1, "all", True, 0, 1))
    return out


BWD_CASES = _bwd_cases()
BWD_BY_NAME = {c.name: c for c in BWD_CASES}
BWD_MUTATIONS = ("last_slab", "swap_fg", "c_prev_next", "dc_in_beyond", "g_deriv")


def bwd_sets(c):
    """per set None or (ns, lda, column offset, rows_x)"""
    return [None if s is None else (s[0], c.H + (WIDE_PAD if s[1] else 0), WIDE_OFF if s[1] else 0, _fewer(c.rows) if s[2] else c.rows)
            for s in BWD_SETS[c.sets]]


def bwd_dc_rows(c):
    return None if c.dc_in is None else (_fewer(c.rows) if c.dc_in == "fewer" else c.rows)


def bwd_mutation_applies(c, mut):
    if c.live == 0:
        return False
    sets = bwd_sets(c)
    carry = c.carry_live != 0
    if mut == "last_slab":                         # the last slab of the last set that is read
        return any(s is not None and (i or carry) for i, s in enumerate(sets))
    if mut == "dc_in_beyond":
        return c.dc_in == "fewer" and carry and _fewer(c.rows) < c.rows
    # (set a alone behind a dead carry and no dhdrop: no gradient arrives, every output is zero whatever the formula)
    arrives = c.dhdrop or (c.dc_in and carry) or any(s is not None and (i or carry) for i, s in enumerate(sets))
    if mut == "c_prev_next":
        return bool(c.c_prev and arrives)
    return bool(arrives)


def bwd_inputs(c):
    rs = seeded("bwd " + c.name)
    rows, H = c.rows, c.H
    sets = bwd_sets(c)
    n_add = sum(s[0] for s in sets if s) + (1 if c.dhdrop else 0)
    sc = 1.0 / np.sqrt(max(n_add, 1))
    d = {}
    for k, s in zip("abc", sets):
        if s:
            d["dh_" + k] = rs.standard_normal((s[0], s[3], H)) * sc
    d.update({"dhdrop": rs.standard_normal((rows, H)) * sc, "dc_in": rs.standard_normal((rows, H)), "c_prev": rs.standard_normal((rows, H)),
              "c_cur": rs.standard_normal((rows, H)),
              "gates": np.concatenate([rs.uniform(0.02, 0.98, (rows, H)), rs.uniform(0.02, 0.98, (rows, H)), rs.uniform(-0.98, 0.98, (rows, H)),
                                       rs.uniform(0.02, 0.98, (rows, H))], axis=1)})
    d = {k: v.astype(np.float32) for k, v in d.items()}
    d["mask"] = rs.choice(MASK_BYTES, size=rows * H).astype(np.uint8)
    return d


def bwd_ref(c, d, mut=None, gates=None, c_cur=None, e_gates=None, e_c=None, keep=None):
    """float64 backward on the fp32 operands -> ((dgates, bound), (dc_prev, bound)); a dead step: zero d gates with bound 0, dc_prev
    None.  gates / c_cur with their bounds e_gates / e_c: the float64 forward cell's, where the kernel reads computed ones (the chained
    case); keep: the forward pass's keep flags in place of the case's own."""
    rows, H = c.rows, c.H
    if c.live == 0:
        return (np.zeros((rows, 4 * H)), np.zeros((rows, 4 * H))), None
    carry = c.carry_live != 0
    sets = bwd_sets(c)
    read = [i for i, s in enumerate(sets) if s is not None and (i or carry)]
    dh, mag, adds = np.zeros((rows, H)), np.zeros((rows, H)), 0
    for i in read:
        x = d["dh_" + "abc"[i]].astype(np.float64)
        if mut == "last_slab" and i == read[-1]:
            x = x[:-1] if x.shape[0] > 1 else x * 0
        n = sets[i][3]
        dh[:n] += x.sum(0)
        mag[:n] += np.abs(x).sum(0)
        adds += sets[i][0] + 1
    if c.dhdrop:
        if keep is None:
            keep = row_keep(c.mode, 0, rows, H, d["mask"], SEED, RNG_OUT, BWD_STEP)
        x = apply_keep(d["dhdrop"].astype(np.float64), keep)
        dh += x
        mag += np.abs(x)
        adds += 1
    e_dh = (adds + 2) * U * mag
    dcin = np.zeros((rows, H))
    if c.dc_in and carry:
        n = rows if mut == "dc_in_beyond" else bwd_dc_rows(c)
        dcin[:n] = d["dc_in"].astype(np.float64)[:n]
    g = d["gates"].astype(np.float64) if gates is None else gates
    eg = np.zeros((rows, 4 * H)) if e_gates is None else e_gates
    gi, gf, gg, go = (g[:, k * H:(k + 1) * H] for k in range(4))
    e_i, e_f, e_g, e_o = (eg[:, k * H:(k + 1) * H] for k in range(4))
    if mut == "swap_fg":
        gf, gg, e_f, e_g = gg, gf, e_g, e_f
    cp = d["c_prev"].astype(np.float64) if c.c_prev else np.zeros((rows, H))
    if mut == "c_prev_next":
        cp = np.roll(cp, -1, axis=1)
    cc = d["c_cur"].astype(np.float64) if c_cur is None else c_cur
    e_cc = np.zeros((rows, H)) if e_c is None else e_c
    tc = np.tanh(cc)
    s = 1.0 - tc * tc
    e_tcin = e_cc * s
    e_tc = e_tcin + TANH_U * U * np.abs(tc)
    e_s = 2 * np.abs(tc) * e_tcin + (2 * TANH_U + 2) * U
    x = dh * go * s
    dcv = dcin + x
    e_dcv = e_dh * np.abs(go) * s + np.abs(dh) * (e_o * s + np.abs(go) * e_s) + 4 * U * (np.abs(dcin) + np.abs(x))
    dg = (1.0 - gg * gg) if mut != "g_deriv" else gg * (1.0 - gg)
    out = [dcv * gg * gi * (1 - gi), dcv * cp * gf * (1 - gf), dcv * gi * dg, dh * tc * go * (1 - go)]
    a = np.abs
    bnd = [e_dcv * a(gg * gi * (1 - gi)) + a(dcv) * (e_g * a(gi * (1 - gi)) + a(gg) * e_i * a(1 - 2 * gi)) + 5 * U * a(out[0]),
           e_dcv * a(cp * gf * (1 - gf)) + a(dcv * cp) * e_f * a(1 - 2 * gf) + 5 * U * a(out[1]),
           e_dcv * a(gi * dg) + a(dcv) * (e_i * a(dg) + a(gi) * 2 * a(gg) * e_g) + a(dcv * gi) * 2 * U + 5 * U * a(out[2]),
           e_dh * a(tc * go * (1 - go)) + a(dh) * (e_tc * a(go * (1 - go)) + a(tc) * e_o * a(1 - 2 * go)) + 5 * U * a(out[3])]
    dcp = dcv * gf
    e_dcp = e_dcv * a(gf) + a(dcv) * e_f + 2 * U * a(dcp)
    return (np.concatenate(out, 1), np.concatenate(bnd, 1) * SECOND), (dcp, e_dcp * SECOND)


# ======================================================================================================================
# the chained case: the forward kernel's stored gates and c' feed the backward kernel
CHAIN_ROW0, CHAIN_ROWS, CHAIN_H = 2, 5, 20        # two evaluation-mode rows in front of five sampled ones
CHAIN_MODES = (1, 2)


def chain_cases(mode):
    """-> (forward case, backward case with a given dh and dc_in, backward case in which nothing but dhdrop carries gradient); both
    sides take the forward's stream and step, the backward over the sampled rows alone"""
    fwd = FwdCase("chain_fwd_mode%d" % mode, CHAIN_ROW0 + CHAIN_ROWS, CHAIN_H, 5, "identity", True, True, mode, CHAIN_ROW0, None, (1, 2),
                  {"loops": NS_LOOPS[5], "wgs": 1, "units": 20, "quads": 5, "route0": 2})
    full = _bwd("chain_bwd_mode%d" % mode, CHAIN_ROWS, CHAIN_H, "a4", True, mode, "all", True, None, None)
    only = _bwd("chain_bwd_only_dhdrop_mode%d" % mode, CHAIN_ROWS, CHAIN_H, "a4", True, mode, None, True, 1, 0)      # the carry is dead: set a is not read
    return fwd, full, only


def chain_ref(mode, fwd_d, bwd_d, bwd_case):
    """the float64 gradient of the float64 cell for the sampled rows: the backward reference on the forward reference's gates and c',
    their bounds carried through, and the forward pass's keep flags (row r of the backward = row r + CHAIN_ROW0 of the forward)"""
    fwd = chain_cases(mode)[0]
    f = fwd_ref(fwd, fwd_d)
    r0 = CHAIN_ROW0
    d = dict(bwd_d)
    d["c_prev"] = fwd_d["c_prev"][r0:]
    return bwd_ref(bwd_case, d, gates=f["gates"][0][r0:], c_cur=f["c"][0][r0:], e_gates=f["gates"][1][r0:], e_c=f["c"][1][r0:], keep=f["keep"][r0:])
