"""CPU-only: the case tables of tests/_token_choice.py are what they say they are (each purpose recomputed as a host predicate, every
deciding comparison exact by construction or at least MARGIN x its counted bound from its neighbours, in the float64 reference alone);
the numpy twin draws the scheduled-sampling streams as csrc/rng.h numbers them; and the icz_test_* entries of the token-choice and
loss kernels refuse what they list before any launch (the pointers handed to them here are not memory)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _philox
import _token_choice as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


# ======================================================================================================================
# the tables
def test_vocabularies_rows_slabs_and_embedding_widths_the_tables_must_hold():
    for cases in (S.GREEDY_CASES, S.SAMPLE_CASES):
        Vs = {c.V for c in cases}
        assert {1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8195} <= Vs and any(10200 <= V <= 10240 for V in Vs)
        assert {1, 2, 4} <= {c.ns for c in cases}
        assert {4, 1024, 4100} <= {c.E for c in cases}
    assert {1, 33, 64} <= {len(c.specs) for c in S.GREEDY_CASES}
    assert {0, 1} <= {c.relu for c in S.GREEDY_CASES}
    assert any(c.ns == 1 and c.bias for c in S.GREEDY_CASES) and any(c.ns > 1 and not c.bias for c in S.GREEDY_CASES)
    assert {1, 32} <= {c.row0 for c in S.SAMPLE_CASES}
    assert {("alive", True), ("sampled_dead", True), ("dead", True), ("dead", False)} <= {(c.gate, c.row0 > 0) for c in S.SAMPLE_CASES}
    assert {0, 1, 2} <= {c.emb_mode for c in S.SAMPLE_CASES} and any(c.philox for c in S.SAMPLE_CASES)
    assert {(5, 4), (33, 3), (2, S.XE_MAX_T)} <= {(c.B, c.T) for c in S.XE_CASES}
    assert {0.0, 0.1, 1.0} <= {c.smoothing for c in S.XE_CASES}
    assert {"absent", "zero", "positive"} <= {"absent" if c.n_dev is None else ("positive" if c.n_dev else "zero") for c in S.XE_CASES}
    assert {"absent", "zero", "positive"} <= {"absent" if c.msum is None else ("positive" if c.msum else "zero") for c in S.RF_CASES}
    assert any(c.B * c.T > 256 for c in S.RF_CASES) and any(c.Bs for c in S.RF_CASES)


@pytest.mark.parametrize("c", S.GREEDY_CASES + S.SAMPLE_CASES, ids=lambda c: type(c).__name__ + "-" + c.name)
def test_layouts_reach_the_load_path_they_are_there_for_and_twins_hold_the_same_values(c):
    lay = S.LAYOUTS[c.layout]
    sample = isinstance(c, S.Sample)
    inp = S.sample_inputs(c) if sample else S.greedy_inputs(c)
    rows = inp["slabs"].shape[1]
    bias = inp["bias"] is not None
    vec = S.takes_vector_loads(lay, c.V, rows, c.ns, bias, store=sample)
    assert vec == (c.layout == "aligned")
    if "scalar" in c.purpose:
        assert c.purpose["scalar"] == (not vec)
        twin = (S.SAMPLE_BY_NAME if sample else S.GREEDY_BY_NAME)[c.purpose["twin"]]
        tin = S.sample_inputs(twin) if sample else S.greedy_inputs(twin)
        assert twin.layout == "aligned" and inp["slabs"].tobytes() == tin["slabs"].tobytes()
        assert (inp["bias"].tobytes() == tin["bias"].tobytes()) if bias else tin["bias"] is None
    ldl, stride = S.geometry(lay, c.V, rows, c.ns)
    assert ldl >= c.V and (c.ns == 1 or stride >= rows * ldl)
    if c.layout == "aligned":
        assert ldl == S.pad_vocab(c.V)
    # NaN wherever the kernel promises not to read: pad columns and the gaps between slabs
    flat = S.place(inp["slabs"], lay, ldl, stride)
    held = np.zeros(flat.size, dtype=bool)
    for z in range(c.ns):
        for r in range(rows):
            held[z * stride + r * ldl:z * stride + r * ldl + c.V] = True
    assert np.isnan(flat[~held]).all() and held.sum() == c.ns * rows * c.V


@pytest.mark.parametrize("c", S.GREEDY_CASES, ids=lambda c: c.name)
def test_greedy_rows_designed_sums_are_exact_and_ties_sit_where_the_rules_are_asked(c):
    inp = S.greedy_inputs(c)
    ref = S.greedy_ref(c, inp)
    x, V = ref["x"], c.V
    with np.errstate(invalid="ignore"):
        exact = inp["slabs"].astype(np.float64).sum(0) + (inp["bias"].astype(np.float64) if c.bias else 0.0)
    kinds = set()
    for r, spec in enumerate(c.specs):
        kinds.add(spec[0])
        if spec[0] == "rand":
            continue
        ok = np.isfinite(x[r])
        assert (x[r][ok].astype(np.float64) == exact[r][ok]).all(), (c.name, r, "a designed row's fp32 sum is not exact")
        if spec[0] == "ties":
            pos = np.asarray([p for p in spec[1] if len(spec) == 2 or p != spec[2]])
            if len(spec) > 2:
                assert ref["ids"][r] == spec[2] and x[r, spec[2]] > x[r, pos].max()
            else:
                assert ref["ids"][r] == pos.min() and len({x[r, p].tobytes() for p in pos}) == 1
                assert int((x[r] == x[r].max()).sum()) == len(pos)
        if spec[0] in ("nan", "ninf"):
            assert ref["ids"][r] == 0
        if spec[0] == "zeros":
            assert ref["ids"][r] == 1 and np.signbit(x[r, spec[2][0]]) and not np.signbit(x[r, spec[1][0]])
    assert {"rand", "onehot", "nan", "ninf", "const"} <= kinds or len(c.specs) == 1
    assert inp["table"][0].any() and (inp["table"] < 0).any()
    ties = [s for s in c.specs if s[0] == "ties" and len(s) == 2]
    for n in (2, 64, 65, 1024, 1025):
        if V >= n and len(c.specs) >= 22:
            assert any(len(s[1]) == n for s in ties), (c.name, n)
    if V >= 4200 and len(c.specs) >= 22:
        big = max(ties, key=lambda s: len(s[1]))[1]
        assert {5, 6, 5 + 1024, 5 + 4096} <= set(big)                   # one group of four; one thread, scalar and vector sweep
        assert len({(p % 1024) // 64 for p in big}) == 16 and len({S.part_of(V, p) for p in big}) == S.PARTS   # every wave, every part
    if V >= 8 and len(c.specs) >= 22:
        Vv = V & ~3
        assert ("ties", [1, V - 1]) in c.specs and ("ties", [0, V - 1]) in c.specs and S.part_of(V, V - 1) != 0
        assert any(s[0] == "ties" and len(s) > 2 and s[2] == V - 1 for s in c.specs) and any(s[0] == "ties" and len(s) > 2 and s[2] == 0 for s in c.specs)
        if Vv < V:
            assert any(s[0] == "ties" and len(s) > 2 and s[2] == Vv for s in c.specs)
    if "empty_parts" in c.purpose:
        per = ((V + S.PARTS - 1) // S.PARTS + 3) & ~3
        assert sum(1 for p in range(S.PARTS) if p * per >= V) == c.purpose["empty_parts"]
    assert set(S.greedy_routes(c)) == ({0, 1, 2} if c.ns == 1 and not c.bias else ({0, 2} if c.ns > 1 else {2}))
    # the <end> bookkeeping has something to count: tokens that are <end> and tokens that are not
    assert len(c.specs) == 1 or V <= S.END or ((ref["ids"] == S.END).any() and (ref["ids"] != S.END).any())


@pytest.mark.parametrize("V", sorted({c.V for c in S.SAMPLE_CASES}))
def test_draw_rows_sit_on_the_edges_and_need_no_excuse(V):
    per, rows = S.per_thread(V), S.draw_rows(V)
    W = 64 * per
    hot = {s[1] for s, _ in rows if s[0] == "onehot"}
    want = {p for p in (0, V - 1, S.END, per - 1, per, W - 1, W) if 0 <= p < V}
    assert want <= hot
    for m in hot:
        assert {float(u) for s, u in rows if s == ("onehot", m)} - {1.0} == {0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24}
    js = set()
    for s, u in rows:
        if s[0] == "const":
            j = int(math.floor(float(u) * V))
            assert abs(float(u) * V - (j + 0.5)) < 0.01 or float(u) == 1.0
            js.add(j)
    assert V < 2 or want <= js
    if V >= 1025:
        lives = [s[1] for s, _ in rows if s[0] == "live"]
        assert any(per - 1 in l and per in l for l in lives) and any(W - 1 in l and W in l for l in lives)
        assert {len(l) for l in lives} >= {2, 4, 8}
    if V < S.SEL_THREADS:
        assert per == 1                                                  # threads V .. 1023 hold empty slices
    # family (d), the scan's one-ulp gap: where exp(-delta) sits on the 2^-52 grid and the ulp margins of u, at per = 1 and per > 1
    gaps = [(s, u) for s, u in S.draw_rows(V, gap=True) if s[0] == "gap"]
    assert len(gaps) == (2 if V >= 1023 else (1 if V >= 5 else 0)) and not any(s[0] == "gap" for s, _ in rows)
    for s, u in gaps:
        g = S.gap_facts(S.designed_row(V, s, S.seeded("gap")), u)
        assert S.gap_holds(g), g
        assert (g["small"], g["big"]) == (s[1], s[2]) and g["big"] != V - 1 and g["lanes"][1] == g["lanes"][0] + 1
        assert 0.70 <= g["cell"] <= 0.80 and g["u_above"] == S.GAP_U_ULPS and g["u_below"] >= 40 and (1 - g["cell"]) * g["grid_ulps"] >= 51
        assert g["u_above"] >= 2 * S.E_EXP and g["u_below"] >= 2 * S.E_EXP
    if V >= 1023:
        assert {g[0][1] % per == per - 1 for g in gaps[:1]} == {True} and gaps[1][0][1] // per // 64 == 1       # a slice edge; the second wave
    assert all(0.0 <= float(u) <= 1.0 for _, u in rows) and sum(float(u) == 1.0 for _, u in rows) == (2 if V >= 2 else 1)
    assert set(s[0] for s, _ in S.draw_rows(V, exact_only=True)) <= {"onehot", "const"}


@pytest.mark.parametrize("c", S.SAMPLE_CASES, ids=lambda c: c.name)
def test_sample_cases_margins_gates_and_reference_invariants(c):
    inp = S.sample_inputs(c)
    log = []
    ref = S.sample_ref(c, inp, log)
    assert all(m >= S.MARGIN for _, m in log), min(log, key=lambda e: e[1])
    B, rows, t = inp["B"], inp["rows"], c.t
    assert rows <= 128 and B >= 4
    want_dead_all = c.gate == "dead"
    assert ref["dead_all"] == want_dead_all and ref["dead_s"] == (c.gate in ("dead", "sampled_dead")) and (c.gate == "alive" or t > 0)
    if c.gate == "sampled_dead":
        assert c.row0 > 0 and inp["nany"][t - 1] > 0 and inp["nunf"][t - 1] == 0
    if ref["dead_s"]:
        assert not ref["seq"].any() and not ref["it_next"][c.row0:].any() and (ref["draw"] == -1).all() and not ref["lse"][0].any()
        assert (ref["unf"] == inp["unf"]).all() and (ref["nunf"] == inp["nunf"]).all() and ref["live_rows"] is None
        return
    assert ref["live_rows"] == (t + 1) * rows
    ended = (ref["draw"][c.row0:] == S.END) | (inp["unf"] == 0)
    assert ended.any() and (~ended).any()
    assert not ref["seq"][ended].any() and not ref["it_next"][c.row0:][ended].any() and not ref["unf"][ended].any()
    assert (ref["seq"][~ended] == ref["draw"][c.row0:][~ended]).all() and ref["nunf"][t] == inp["nunf"][t] + int((~ended).sum())
    if not c.philox:
        x = S.finish(inp["slabs"], inp["bias"])[c.row0:]
        assert any(s[0] == "gap" for s, _ in S.draw_rows(c.V, gap=c.ns == 1)) == (c.ns == 1 and c.V >= 5)
        for b, (spec, u) in enumerate(S.draw_rows(c.V, gap=c.ns == 1)):
            if spec[0] == "onehot":
                assert ref["draw"][c.row0 + b] == (c.V - 1 if float(u) == 1.0 else spec[1]) and S.is_onehot(x[b]) and ref["logp"][1][b] == 0.0
            elif spec[0] == "gap":
                assert ref["draw"][c.row0 + b] == spec[2] != c.V - 1 and x[b, spec[1]] == np.float32(-spec[3]) and x[b, spec[2]] == 0
            elif spec[0] == "const":
                assert ref["draw"][c.row0 + b] == min(int(math.floor(float(u) * c.V)), c.V - 1)
            else:
                assert ref["draw"][c.row0 + b] in spec[1] and ref["logp"][1][b] > 0.0
    else:
        assert (inp["u"] == _philox._uniforms(inp["seed"], S.T_STEPS, B)[t]).all() and len(set(inp["u"].tolist())) > B // 2
    if c.emb_mode and ref["emb"] is not None:
        e = ref["emb"][c.row0:]
        assert (e[inp["mask"] == 0] == 0).all() and 0.3 < inp["mask"].mean() < 0.7


@pytest.mark.parametrize("c", S.SS_CASES, ids=lambda c: c.name)
def test_scheduled_sampling_cases(c):
    inp = S.ss_inputs(c)
    log = []
    tok = S.ss_ref(c, inp, log)
    assert all(m >= S.MARGIN for _, m in log)
    drew = inp["gate"][S.SS_T - 1] < np.float32(c.ss_prob)
    assert (tok[~drew] == inp["tok"][~drew]).all()
    if c.ss_prob == 0.0:
        assert not drew.any()
    elif c.ss_prob == 1.0:
        assert drew.all()
    else:
        assert drew.any() and (~drew).any()
    if not c.philox:
        assert np.isnan(inp["gate"][:S.SS_T - 1]).all() and np.isnan(inp["draw"][:S.SS_T - 1]).all()      # only row t is read


def test_loss_cases_hold_their_edges():
    for c in S.XE_CASES:
        inp = S.xe_inputs(c)
        g, gb, rows, rb, loss, lb, act = S.xe_ref(c, inp)
        assert len(inp["rows_t"]) == c.T and inp["rows_t"][0] == c.B and inp["rows_t"][-1] >= 1
        assert (c.B * c.T <= 10) or (not act.all() and act.any())                       # ragged: inactive rows exist
        assert inp["cap"][0, 1] in (0, c.V - 1) and (c.T == 1 or {int(inp["cap"][0, 1]), int(inp["cap"][0, 2])} == {0, c.V - 1})
        assert S.is_onehot(inp["x"][0]) and np.isfinite(g).all() and (gb[act] > 0).all() and lb > 0
        assert abs(g[act].sum(1)).max() < 1e-7                                          # softmax - true sums to zero (true: fp32 conf + (V - 1) low)
        if c.smoothing == 0.0:
            assert abs(rows[0]) < 1e-12                                                 # saturated on the target: no loss
    assert any(not S.xe_ref(c, S.xe_inputs(c))[6].all() for c in S.XE_CASES)
    for c in S.RF_CASES:
        inp = S.rf_inputs(c)
        ref = S.rf_ref(c, inp)
        assert c.T > 1 and (ref["mask"][:, 0] == 1).all() and ref["mask"][-1, 1:].sum() == 0 and ref["mask"][0].all() and 0 < ref["ms"] < c.B * c.T
        assert (inp["reward"][1 % c.B] == 0).all() and ref["zero_rows"].any() and not ref["zero_rows"].all()
        assert np.isnan(inp["x"][ref["zero_rows"]]).any() and np.isfinite(inp["x"][~ref["zero_rows"]]).all()
        if c.Bs:
            assert c.Bs == c.row0 + c.B and (inp["draw"].reshape(c.T, c.Bs)[:, :c.row0] == -1).all()
        live = inp["draw"][~ref["zero_rows"]]
        assert 0 in live or c.V - 1 in live


def test_philox_twin_numbers_the_streams_as_rng_h_does():
    src = open(os.path.join(ROOT, "simpleimagecaptionzoo_amd", "csrc", "rng.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"(RNG_[A-Z_]+) = (\d+)", src))
    for name in ("RNG_EMB", "RNG_UNIFORM", "RNG_SS_GATE", "RNG_SS_DRAW"):
        assert getattr(_philox, name) == enum[name]
    seed = 0x0123456789ABCDEF
    g, d = _philox._uniforms(seed, 3, 40, _philox.RNG_SS_GATE), _philox._uniforms(seed, 3, 40, _philox.RNG_SS_DRAW)
    assert g.shape == (3, 40) and (g != d).mean() > 0.9 and (g != _philox._uniforms(seed, 3, 40)).mean() > 0.9
    assert ((g >= 0) & (g < 1)).all() and (g * 2 ** 24 == np.floor(g * 2 ** 24)).all()


# ======================================================================================================================
# the entries refuse before they launch
def _refused(status, *words):
    err = _lib().icz_last_error()
    assert status == -1, (status, err)
    for w in words:
        assert w in err, (w, err)


P, ODD = 4096, 4100


def test_the_lds_rule_is_one_number_and_both_select_entries_keep_it():
    from simpleimagecaptionzoo_amd._lib import SampleSelectArgs
    from simpleimagecaptionzoo_amd.token_choice import sample_select_max_vocab
    vmax = sample_select_max_vocab()
    assert vmax == 159 * 1024 // 4 and vmax > 16384
    a = SampleSelectArgs()
    for n, _ in SampleSelectArgs._fields_:
        if getattr(SampleSelectArgs, n).size == 8 and n != "slab_stride":
            setattr(a, n, P)
    a.V, a.ldl, a.ns, a.t, a.T, a.E = vmax + 1, vmax + 64, 1, 0, 4, 4
    _refused(_lib().icz_test_sample_select(ctypes.byref(a), 2, None), b"icz_test_sample_select", b"%d logits does not fit in LDS" % (vmax + 1))
    _refused(_lib().icz_test_ss_select(P, 2, 2, vmax + 1, vmax + 64, 2, 0.5, P, P, P, P, None), b"icz_test_ss_select", b"%d logits" % (vmax + 1))


def test_greedy_select_entry_refusals():
    def call(route=0, logits=P, rows=2, V=300, ldl=320, ns=1, stride=0, bias=None, table=P, E=8, relu=1, t=0, T=4, ids=P, it=P, emb=P, unf=None,
             nunf=None, pv=P, pi=P):
        return _lib().icz_test_greedy_select(route, logits, rows, V, ldl, ns, stride, bias, table, E, relu, t, T, ids, it, emb, unf, nunf, pv, pi, None)
    for kw, word in ((dict(route=3), b"route=3"), (dict(route=-1), b"route=-1"), (dict(V=0), b"V=0"), (dict(ldl=299), b"ldl=299"), (dict(rows=0), b"rows=0"),
                     (dict(ns=0), b"ns=0"), (dict(ns=17, stride=640), b"ns=17"), (dict(ns=2, stride=600, bias=P), b"slab_stride=600"),
                     (dict(E=0), b"E=0"), (dict(E=6), b"E=6"), (dict(table=ODD), b"16-byte"), (dict(emb=ODD), b"16-byte"), (dict(t=4), b"t=4"),
                     (dict(t=-1), b"t=-1"), (dict(T=0), b"T=0"), (dict(logits=None), b"null logits"), (dict(table=None), b"null embedding"),
                     (dict(emb=None), b"null embedding"), (dict(it=None), b"null it_next"), (dict(unf=P), b"go together"),
                     (dict(nunf=P), b"go together"), (dict(route=1, ns=2, stride=640, bias=P), b"two-kernel form"),
                     (dict(route=1, bias=P), b"two-kernel form"), (dict(route=0, unf=P, nunf=P), b"two-kernel form"),
                     (dict(route=1, pv=None), b"part_val"), (dict(pi=None), b"part_val")):
        _refused(call(**kw), b"icz_test_greedy_select", word)


def test_sample_and_ss_select_entry_refusals():
    from simpleimagecaptionzoo_amd._lib import SampleSelectArgs

    def call(rows=2, null_struct=False, **kw):
        a = SampleSelectArgs()
        for n, _ in SampleSelectArgs._fields_:
            if getattr(SampleSelectArgs, n).size == 8 and n != "slab_stride":
                setattr(a, n, P)
        a.V, a.ldl, a.ns, a.t, a.T, a.E, a.emb_mode, a.row0, a.slab_stride = 300, 320, 1, 0, 4, 8, 0, 0, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return _lib().icz_test_sample_select(None if null_struct else ctypes.byref(a), rows, None)
    for kw, word in ((dict(null_struct=True), b"null arguments"), (dict(V=0), b"V=0"), (dict(ldl=299), b"ldl=299"), (dict(rows=0), b"rows=0"),
                     (dict(ns=0), b"ns=0"), (dict(ns=2, slab_stride=100), b"slab_stride=100"), (dict(ns=2, slab_stride=640, bias=None), b"slabs need"),
                     (dict(ns=2, slab_stride=640, logits_store=None), b"slabs need"), (dict(t=4), b"t=4"), (dict(T=0), b"T=0"),
                     (dict(logits=None), b"null logits"), (dict(unfinished=None), b"null argument"), (dict(n_unfinished=None), b"null argument"),
                     (dict(seq_out=None), b"null argument"), (dict(logp_out=None), b"null argument"), (dict(it_next=None), b"null argument"),
                     (dict(draw_out=None), b"null argument"), (dict(lse_out=None), b"null argument"), (dict(uniforms=None, seed=None), b"uniforms or a seed"),
                     (dict(row0=2), b"row0=2"), (dict(row0=-1), b"row0=-1"), (dict(row0=1, ids_out=None), b"merged launch"),
                     (dict(row0=1, g_unfinished=None), b"merged launch"), (dict(row0=1, n_any=None), b"merged launch"), (dict(emb_mode=3), b"emb_mode=3"),
                     (dict(E=6), b"E=6"), (dict(emb_table=None), b"null embedding"), (dict(emb_next=ODD), b"16-byte"), (dict(emb_table=ODD), b"16-byte"),
                     (dict(emb_mode=1, emb_mask=None), b"emb_mask"), (dict(emb_mode=1, emb_mask=P + 2), b"emb_mask"),
                     (dict(emb_mode=2, seed=None), b"need a seed")):
        _refused(call(**kw), b"icz_test_sample_select", word)

    def ss(lp=P, rows=2, B=2, V=300, ldl=320, t=2, p=0.5, gate=P, draw=P, seed=P, tok=P):
        return _lib().icz_test_ss_select(lp, rows, B, V, ldl, t, p, gate, draw, seed, tok, None)
    for kw, word in ((dict(lp=None), b"null logits"), (dict(V=0), b"V=0"), (dict(ldl=299), b"ldl=299"), (dict(rows=0), b"rows=0"), (dict(B=1), b"B=1"),
                     (dict(t=-1), b"t=-1"), (dict(p=1.5), b"ss_prob"), (dict(p=-0.1), b"ss_prob"), (dict(tok=None), b"null argument"),
                     (dict(gate=None, seed=None), b"null argument"), (dict(draw=None, seed=None), b"null argument")):
        _refused(ss(**kw), b"icz_test_ss_select", word)


def test_loss_entry_refusals():
    rt = (ctypes.c_int32 * 4)(5, 4, 2, 1)

    def xe(logits=P, V=300, ldl=320, cap=P, L=6, B=5, T=4, rows_t=rt, s=0.1, n=12.0, n_dev=None, loss_rows=P, loss_out=P):
        return _lib().icz_test_xe_loss(logits, V, ldl, cap, L, B, T, rows_t, s, n, n_dev, loss_rows, loss_out, None)
    big = (ctypes.c_int32 * 129)(*([1] * 129))
    for kw, word in ((dict(V=1, ldl=64), b"V=1"), (dict(ldl=299), b"ldl=299"), (dict(T=0), b"T=0"), (dict(T=129, L=131, rows_t=big), b"T=129"),
                     (dict(L=4), b"L=4"), (dict(B=0), b"B=0"), (dict(rows_t=(ctypes.c_int32 * 4)(5, 6, 2, 1)), b"rows_t[1]=6"),
                     (dict(rows_t=(ctypes.c_int32 * 4)(5, 4, -1, 1)), b"rows_t[2]=-1"), (dict(s=1.5), b"smoothing"), (dict(s=-0.5), b"smoothing"),
                     (dict(n=0.0), b"n_tokens"), (dict(logits=None), b"null argument"), (dict(cap=None), b"null argument"),
                     (dict(rows_t=None), b"null argument"), (dict(loss_rows=None), b"null argument")):
        _refused(xe(**kw), b"icz_test_xe_loss", word)

    def rf(logp=P, seq=P, reward=P, B=5, T=4, msum=None, coef=P, loss=P, ms=P, logits=P, V=300, ldl=320, draw=P, lse=P, Bs=0, row0=0):
        return _lib().icz_test_reinforce(logp, seq, reward, B, T, msum, coef, loss, ms, logits, V, ldl, draw, lse, Bs, row0, None)
    for kw, word in ((dict(V=0), b"V=0"), (dict(ldl=299), b"ldl=299"), (dict(B=0), b"B=0"), (dict(T=0), b"T=0"), (dict(Bs=9, row0=5), b"Bs=9"),
                     (dict(Bs=12, row0=5), b"Bs=12"), (dict(Bs=0, row0=1), b"Bs=0"), (dict(Bs=4, row0=-1), b"Bs=4"),
                     (dict(B=300, T=300), b"exceed the grid"), (dict(logp=None), b"null argument"), (dict(seq=None), b"null argument"),
                     (dict(reward=None), b"null argument"), (dict(coef=None), b"null argument"), (dict(logits=None), b"null argument"),
                     (dict(draw=None), b"null argument"), (dict(lse=None), b"null argument")):
        _refused(rf(**kw), b"icz_test_reinforce", word)


def test_argmax_part_kernel_has_no_parameter_without_a_caller():
    src = open(os.path.join(ROOT, "simpleimagecaptionzoo_amd", "csrc", "token_kernels.h")).read()
    head = src[src.index("void argmax_part_kernel("):]
    head = head[:head.index(")")]
    assert [w.split()[-1].lstrip("*") for w in head.split("(")[1].split(",")] == ["logits", "V", "ldl", "P", "part_val", "part_idx"]
    core = open(os.path.join(ROOT, "simpleimagecaptionzoo_amd", "csrc", "decoder_core.hip")).read()
    call = core[core.index("hipLaunchKernelGGL(argmax_part_kernel"):]
    assert call[:call.index(";")].count(",") == 5 + 6 - 1 + 1             # the launch macro's five leading arguments (one comma in the grid) and the kernel's six
