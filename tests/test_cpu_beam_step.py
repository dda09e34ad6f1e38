"""Host-side checks of tests/_beam_step.py (no GPU): every case serves the purpose its table states -- recomputed here, from
icz_beam_rowtopk_route_for where the threshold is the library's, so a retuned threshold names the case that lost its purpose --; every
comparison that decides a selection is a tie by construction or separated by the margin (64 x the counted score bound); the reference
agrees with torch.log_softmax + topk in float64 on the separated cases and with the two whole-search oracles on the chained ones; and
the icz_test_beam_* entries refuse what they list before any launch (the pointers handed to them here are not memory)."""
import ctypes

import numpy as np
import pytest
import torch

import _beam_opts_oracle as bo
import _beam_step as S
import _diverse_beam_oracle as do


def _route_for(V, ldl, aligned=True):
    from simpleimagecaptionzoo_amd.beam import rowtopk_route_for
    return rowtopk_route_for(V, ldl, aligned)


def _ban_entries(prefix, n):
    """entries of the device's ban list, duplicates counted: start positions whose n - 1 tokens equal the prefix's last n - 1"""
    s = len(prefix) - 1
    if n == 0 or s < n - 1:
        return 0
    return sum(prefix[i:i + n - 1] == prefix[s - n + 2:] for i in range(s - n + 2))


def _margin(log, what):
    assert log, (what, "no selection was decided")
    worst = min(log, key=lambda e: e[1])
    assert worst[1] >= S.MARGIN, (what, worst)


def _empty_middle(c):
    n_act = np.asarray(c.n_act).reshape(c.n_img, c.groups)
    # an empty group with live ones behind it and (where there are more than two groups) in front of it
    return any(n_act[i, g] == 0 and (c.groups == 2 or n_act[i, :g].sum() > 0) and n_act[i, g + 1:].sum() > 0
               for i in range(c.n_img) for g in range(c.groups))


# ---------------------------------------------------------------------------------------------------------------------
# purposes
RT_KEYS = {"route0", "wide_ld", "n_acts", "scored", "ties", "list_cnt", "threads", "path", "rounds", "banned", "ban_entries", "best_banned",
           "slot_classes", "admissible", "no_ban", "empty_middle"}


@pytest.mark.parametrize("c", S.RT_CASES, ids=lambda c: c.name)
def test_row_topk_case_serves_its_purpose(c):
    p = c.purpose
    assert p and not set(p) - RT_KEYS, set(p) - RT_KEYS
    inp = S.case_inputs(c)
    assert c.n_img * c.k <= 24 and c.ldl >= c.V
    aligned = c.off % 4 == 0
    assert _route_for(c.V, c.ldl, aligned) == p["route0"]
    assert 0 in c.routes and p["route0"] in c.routes and 3 in c.routes
    assert set(c.routes) == {0} | {r for r in (1, 2, 3) if S.fits(r, c.V, c.ldl, c.off)}, "every forced route the shape allows"
    if p["route0"] == 3 and c.V <= 10240:
        assert c.ldl % 4 != 0 or not aligned, "a small vocabulary reaches the sweep kernel under route 0 only on an odd stride or base"
    x0 = next(inp["logits"][i] for i in range(inp["logits"].shape[0]) if not np.isnan(inp["logits"][i, 0]))
    na0 = max(S.row_cands_count(inp["n_act"][row // c.k], row % c.k, c.k, c.groups, c.step) for row in range(c.n_img * c.k))
    pre0 = inp["seqs"][0, :c.step].tolist()
    ban0 = S.banned_of(c, inp, 0)
    if "wide_ld" in p:
        assert (c.ldl > S.round4(c.V)) == p["wide_ld"]
    if "n_acts" in p:
        assert sorted(set(np.asarray(c.n_act).tolist())) == p["n_acts"]
    if "scored" in p:
        assert sorted(S.scored_rows(c, inp)) == p["scored"]
    if "ties" in p:
        assert int((x0 == x0.max()).sum()) == p["ties"]
    if "threads" in p:
        owners = {S.owner(int(v))[0] for v in np.flatnonzero(x0 == x0.max())}
        assert len(owners) >= max(p["threads"][1], na0) if p["threads"][0] == "min" else len(owners) <= p["threads"][1]
    if "list_cnt" in p or "path" in p or "rounds" in p:
        cnt, rounds = S.reg_list(x0.astype(np.float64), na0)
        assert cnt == p.get("list_cnt", cnt) and rounds >= p.get("rounds", 1)
        if "path" in p:
            assert (cnt <= S.CAP) == (p["path"] == "list"), cnt
    if "banned" in p:
        assert set(p["banned"]) <= set(ban0)
    if "ban_entries" in p:
        assert c.ngram and _ban_entries(pre0, c.ngram) >= p["ban_entries"]
    if "best_banned" in p:
        assert int(x0.argmax()) in ban0
    if "slot_classes" in p:
        assert len({S.owner(v)[1:] for v in p["banned"]}) == p["slot_classes"] == 4 * (3 if p["route0"] == 1 else 10)
    if "admissible" in p:
        assert c.V - len(ban0) == p["admissible"] < na0, "fewer admissible tokens than candidates: empty slots"
    if "no_ban" in p:
        assert c.ngram and not any(S.banned_of(c, inp, r) for r in range(c.n_img * c.k))
    if "empty_middle" in p:
        assert _empty_middle(c)


def test_row_topk_table_covers_what_it_must():
    """the four sweep instances forced at small V and under route 0; both register kernels on both paths, 128 against 129"""
    def have(pred):
        return [c.name for c in S.RT_CASES if pred(c)]
    ban = lambda c: c.ngram and c.step >= c.ngram
    for grouped in (False, True):
        for banned in (False, True):
            assert have(lambda c: (c.groups > 1) == grouped and bool(ban(c)) == banned and c.V <= 3072 and 3 in c.routes)
            assert have(lambda c: (c.groups > 1) == grouped and bool(ban(c)) == banned and c.V > 10240 and c.purpose["route0"] == 3)
    assert have(lambda c: c.purpose["route0"] == 3 and c.ldl % 2 == 1) and have(lambda c: c.purpose["route0"] == 3 and c.off == 1)
    for route in (1, 2):
        for path, T in (("list", 128), ("overflow", 129)):
            assert have(lambda c: route in c.routes and c.purpose.get("path") == path and c.purpose.get("list_cnt") == T)
    assert {c.k for c in S.RT_CASES} >= {1, 5, 8} and {c.groups and (c.k, c.groups) for c in S.RT_CASES} >= {(4, 2), (6, 3), (8, 4), (8, 8)}
    assert {c.V for c in S.RT_CASES} >= set(S.ROUTE0_AT)


STEP_KEYS = {"end", "ends", "listed_after", "n_act_after", "n_live_after", "vanish", "copy", "cross_tie", "c_of_token", "key_tie", "repeated_token",
             "ban_entries", "empty_middle"}


@pytest.mark.parametrize("c", S.STEP_CASES, ids=lambda c: c.name)
def test_step_case_serves_its_purpose(c):
    p = c.purpose
    assert p and not set(p) - STEP_KEYS, set(p) - STEP_KEYS
    assert set(c.routes) == {0, 1, 2, 3} and c.n_img * c.k <= 24
    inp = S.case_inputs(c)
    before = S.new_state(c, inp)
    log = []
    st = S.step_ref(c, inp, S.new_state(c, inp), log)
    k = c.k
    if "end" in p:
        for img, how in enumerate(p["end"]):
            new = st["hyp"]["score"][img * k]                                   # the <end> pick's score, as listed
            assert st["hyp"]["cnt"][img] == 1 and st["max_bound"] == 0.0
            old = before["best_score"][img]
            assert {"wins": new > old, "loses": new < old, "ties": new == old}[how]
            assert (st["best_len"][img] == c.step + 1) == (how == "wins") and st["best_score"][img] == (new if how == "wins" else old)
    if "n_act_after" in p:
        assert st["n_act"].tolist() == p["n_act_after"]
    if "listed_after" in p:
        assert st["hyp"]["cnt"].tolist() == p["listed_after"]
    if "n_live_after" in p:
        assert st["n_live"] == p["n_live_after"]
    if "ends" in p:
        gone = before["n_act"] - st["n_act"]
        assert (gone - np.asarray([p.get("vanish", 0)] + [0] * (c.n_img - 1))).tolist() == p["ends"]
    if "vanish" in p:
        admissible = sum(c.V - len(S.banned_of(c, inp, r)) for r in range(int(before["n_act"][0])))
        assert before["n_act"][0] - admissible == p["vanish"] > 0
    if "copy" in p:
        assert c.step == p["copy"] and (st["seqs_out"][0, :c.step] != S.CANARY).all()
    if "cross_tie" in p:
        assert st["src_row"][:3].tolist() == [0, 1, 2] and len(set(st["it_next"][:3].tolist())) == 1
    if "repeated_token" in p:
        toks = st["it_next"][:k][st["src_row"][:k] != np.arange(k)].tolist() + st["it_next"][:1].tolist()
        assert len(set(toks)) < len(toks), "no token picked by two groups"
    if "key_tie" in p:
        tok, cnt = p["c_of_token"]
        lam, r0 = np.float32(c.lam), np.float32(c.run[6])
        pen = np.float32(lam * np.float32(cnt))
        assert float(pen) != float(lam) * cnt, "the product is exact: fused and unfused keys agree"
        unfused, fused = np.float32(r0 - pen), np.float32(np.float64(r0) - np.float64(lam) * cnt)
        assert unfused == np.float32(c.run[7]) and fused < unfused, "the unfused key ties the other row's score, the fused one loses to it"
        assert st["it_next"][:8].tolist() == [tok, tok, tok, tok, tok, 0, tok, S.Y_] and st["src_row"][6:8].tolist() == [6, 7]
    if "ban_entries" in p:
        assert _ban_entries(inp["seqs"][0, :c.step].tolist(), c.ngram) >= p["ban_entries"]
    if "empty_middle" in p:
        assert _empty_middle(c)
    _margin(log, c.name)


def test_step_table_covers_what_it_must():
    names = {c.name for c in S.STEP_CASES}
    assert {c.step for c in S.STEP_CASES} >= {1, 64, 65, 130}
    assert {(c.k, c.groups, c.lam) for c in S.STEP_CASES} >= {(k, g, l) for k, g in ((4, 2), (6, 3), (8, 4), (8, 8)) for l in (0.0, 0.5, 0.3)}
    assert any(not c.listed for c in S.STEP_CASES) and any(c.hyp_cnt and c.k - 1 in c.hyp_cnt and c.k in c.hyp_cnt for c in S.STEP_CASES)
    assert any(0 in np.asarray(c.n_act).reshape(c.n_img, -1).sum(1) and c.groups == 1 for c in S.STEP_CASES), names


# ---------------------------------------------------------------------------------------------------------------------
# the margin condition, every case
@pytest.mark.parametrize("c", S.RT_CASES, ids=lambda c: c.name)
def test_row_topk_case_is_decided_by_ties_or_margins(c):
    log = []
    ref = S.rowtopk_ref(c, S.case_inputs(c), log)
    assert ref
    if not ("ties" in c.purpose and c.purpose["ties"] >= c.k) and c.V > 1:
        _margin(log, c.name)
    assert all(r >= S.MARGIN for _, r in log)


@pytest.mark.parametrize("case", S.CHAIN_CASES, ids=lambda a: a[0])
def test_chained_case_is_decided_by_margins(case):
    log = []
    S.chain_ref(*case, log)
    _margin(log, case[0])


@pytest.mark.parametrize("name", list(S.FIN_CASES))
def test_finalize_case_is_decided_by_ties_or_margins(name):
    form, f = S.FIN_CASES[name]
    log = []
    out, lens, scores = S.finalize_ref(form, f, log)
    assert all(r >= S.MARGIN for _, r in log), min(log, key=lambda e: e[1])
    if form:
        _margin(log, name)
        assert (lens == 0).any() and np.isneginf(scores[lens == 0]).all(), "a rank past the image's hypotheses"
        live = [len(S.live_rows(f["n_act"][i], i, f["k"], f["groups"])) for i in range(f["n_img"])]
        assert any(l and h for l, h in zip(live, f["hyp_cnt"])), "finished beside live"
    else:
        assert f["has_complete"].tolist() == [1, 0, 0, 0] and f["n_act"][2] == 0 and f["run"][3] == f["run"][4] > f["run"][5]
        assert lens[:, 0].tolist() == [f["best_len"][0]] + [f["steps_done"] + 1] * 3 and np.isneginf(scores[2, 0])
        n = f["steps_done"] + 1
        assert (out[1, 0, :n] == f["seqs"][3, :n]).all() and (out[3, 0, :n] == f["seqs"][11, :n]).all() and not out[:, 0, n:].any()


def test_score_bound_is_the_counted_one():
    x = np.linspace(-8.0, 8.0, 10300).astype(np.float32)
    sc, bound, exact = S.row_scores(x, -3.0)
    assert not exact and 5e-6 < bound < 16.0 / 10299 / S.MARGIN, bound
    d, ls = 16.0, float(np.log(np.exp(x.astype(np.float64) - 8.0).sum()))
    assert abs(bound - S.U * ((d + d + ls + 3.0 + d + ls) + (41 + 8 + 8 + d) + 8 * ls)) < 1e-12
    sc, bound, exact = S.row_scores(S.make_row(23, ("onehot", 5), S.seeded("x")), -1.25)
    assert exact and bound == 0.0 and sc[5] == -1.25 and sc.max() == sc[5]


# ---------------------------------------------------------------------------------------------------------------------
# the reference against independent statements
@pytest.mark.parametrize("c", [c for c in S.RT_CASES if "ties" not in c.purpose], ids=lambda c: c.name)
def test_reference_equals_float64_log_softmax_and_topk(c):
    inp = S.case_inputs(c)
    ref = S.rowtopk_ref(c, inp, [])
    for row, (idx, val, _) in ref.items():
        x = torch.from_numpy(inp["logits"][row // c.k if c.compact else row].astype(np.float64))
        sc = torch.log_softmax(x, 0) + (0.0 if c.step == 1 else float(inp["run"][row]))
        ban = S.banned_of(c, inp, row)
        if ban:
            sc[ban] = -float("inf")
        n = min(len(idx), int(torch.isfinite(sc).sum()))
        top, ti = sc.topk(n)
        assert ti.tolist() == idx[:n].tolist() and (idx[n:] == S.SENT).all()
        assert np.abs(top.numpy() - val[:n]).max() < 1e-11 and np.isneginf(val[n:]).all()


def _ranked(c, st, img):
    """the image's hypotheses of the reference's final state, ranked as icz_beam_opts says (no penalty)"""
    k, L = c.k, st["seqs_out"].shape[1]
    f = {"n_img": c.n_img, "k": k, "L": L, "steps_done": S.CHAIN_STEPS, "groups": c.groups, "n_best": k, "lp_kind": 0, "lp_alpha": 0.0,
         "n_act": st["n_act"], "run": st["run"].astype(np.float32), "seqs": st["seqs_out"], "hyp_cnt": st["hyp"]["cnt"],
         "hyp_score": st["hyp"]["score"].astype(np.float32), "hyp_len": st["hyp"]["len"], "hyp_seq": st["hyp"]["seq"]}
    out, lens, scores = S.finalize_ref(2 if c.groups > 1 else 1, f, [])
    return [(out[img, m, :lens[img, m]].astype(int).tolist(), float(scores[img, m])) for m in range(k) if lens[img, m]]


@pytest.mark.parametrize("case", S.CHAIN_CASES, ids=lambda a: a[0])
def test_chained_reference_equals_the_whole_search_oracles(case):
    name, k, G, lam, ngram = case
    c, inp, lg, states = S.chain_ref(*case, [])
    kg = k // G
    for img in range(c.n_img):
        calls = [0]

        def step(prev, state):
            s = calls[0]
            calls[0] += 1
            grp = state[0].tolist()
            rows = [img * k if s == 0 else img * k + g * kg + grp[:i].count(g) for i, g in enumerate(grp)]
            return torch.from_numpy(lg[s][rows]), state
        state = (torch.tensor([g for g in range(G) for _ in range(kg)]),)
        if G == 1:
            want = bo.beam_nbest(step, state, k, c.V, S.CHAIN_STEPS, ngram)
        else:
            want = do.diverse_nbest(step, state, k, G, lam, c.V, S.CHAIN_STEPS, ngram)
        got = _ranked(c, states[-1], img)
        assert [w[0] for w in want] == [g[0] for g in got], (name, img)
        assert np.abs(np.asarray([w[1] for w in want]) - np.asarray([g[1] for g in got])).max() < 1e-4
        assert any(w[2] for w in want) and not all(w[2] for w in want), "the case retires some beams and keeps some"
    if ngram:
        plain = S.chain_ref(name, k, G, lam, 0, [])[3][-1]
        assert not np.array_equal(plain["seqs_out"], states[-1]["seqs_out"]), "blocking changed nothing"


# ---------------------------------------------------------------------------------------------------------------------
# refusals, all before any launch
def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _refused(status, *words):
    err = _lib().icz_last_error()
    assert status == -1, (status, err)
    for w in words:
        assert w in err, (w, err)


P, ODD = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
SHAPE_REFUSALS = [(dict(k=0), b"k=0"), (dict(k=9), b"k=9"), (dict(groups=2), b"groups=2"), (dict(groups=0), b"groups=0"),
                  (dict(k=6, groups=4), b"groups=4"), (dict(step=0), b"step=0"), (dict(step=257, L=300), b"step=257"),
                  (dict(step=5, L=5), b"L=5"), (dict(ngram=1), b"ngram=1"), (dict(ngram=5), b"ngram=5"), (dict(ngram=-2), b"ngram=-2"),
                  (dict(compact=1), b"compact=1"), (dict(compact=2, step=1), b"compact=2"), (dict(V=0), b"V=0"), (dict(n_img=0), b"n_img=0"),
                  (dict(route=4), b"route=4"), (dict(route=-1), b"route=-1"), (dict(n_img=1 << 20), b"n_img=1048576"),
                  (dict(V=1 << 30, ldl=1 << 30), b"V=1073741824"), (dict(V=300, ldl=296), b"ldl=296")]


def test_route_entry_and_row_topk_refusals():
    L = _lib()
    for V, ldl, al, want in ((3072, 3072, 1, 1), (3073, 3076, 1, 2), (10240, 10240, 1, 2), (10241, 10244, 1, 3), (300, 301, 1, 3), (300, 300, 0, 3),
                             (300, 302, 1, 3)):
        assert L.icz_beam_rowtopk_route_for(V, ldl, al) == want
    for V, ldl in ((0, 4), (300, 299), (-1, -1)):
        _refused(L.icz_beam_rowtopk_route_for(V, ldl, 1), b"icz_beam_rowtopk_route_for")

    def call(route=0, logits=P, n_img=2, k=5, V=300, ldl=300, step=5, n_act=P, run=P, compact=0, seqs_in=P, L=7, ngram=0, groups=1, cand_val=P,
             cand_idx=P):
        return _lib().icz_test_beam_rowtopk(route, logits, n_img, k, V, ldl, step, n_act, run, compact, seqs_in, L, ngram, groups, cand_val, cand_idx,
                                            None)
    for kw, word in SHAPE_REFUSALS:
        _refused(call(**kw), b"icz_test_beam_rowtopk", word)
    for route, V, ldl, off in S.RT_REFUSED:
        _refused(call(route=route, V=V, ldl=ldl, logits=ODD if off else P), b"icz_test_beam_rowtopk")
        assert route == 0 or ldl < V or not S.fits(route, V, ldl, off)
    _refused(call(route=1, V=3073, ldl=3076), b"route 1 cannot take V=3073")
    _refused(call(route=2, logits=ODD), b"not 16-byte aligned")
    for hole in ("logits", "n_act", "run", "cand_val", "cand_idx"):
        _refused(call(**{hole: None}), b"null argument")
    _refused(call(seqs_in=None, ngram=2), b"null argument")


def test_step_entry_refusals():
    from simpleimagecaptionzoo_amd._lib import BEAM_STEP_FIELDS, BeamStepState

    def call(route=0, state=True, n_img=2, k=5, V=300, ldl=300, step=5, L=7, compact=0, ngram=0, groups=1, lam=0.0, **ptrs):
        vals = {n: 4096 + 64 * i for i, n in enumerate(BEAM_STEP_FIELDS)}
        vals.update(ptrs)
        s = BeamStepState(*[vals[n] for n in BEAM_STEP_FIELDS])
        return _lib().icz_test_beam_step(route, ctypes.byref(s) if state else None, n_img, k, V, ldl, step, L, compact, ngram, groups, lam, None)
    for kw, word in SHAPE_REFUSALS:
        _refused(call(**kw), b"icz_test_beam_step", word)
    for route, V, ldl, off in S.RT_REFUSED:
        _refused(call(route=route, V=V, ldl=ldl, logits=4100 if off else 4096), b"icz_test_beam_step")
    _refused(call(state=False), b"null state")
    for hole in BEAM_STEP_FIELDS:
        if not hole.startswith("hyp_"):
            _refused(call(**{hole: None}), b"null argument")
        else:
            _refused(call(**{hole: None}), b"four pointers or none")
    none = dict(hyp_seq=None, hyp_score=None, hyp_len=None, hyp_cnt=None)
    _refused(call(k=6, groups=3, **none), b"a grouped step needs the n-best list")
    _refused(call(seqs_out=4096 + 64 * BEAM_STEP_FIELDS.index("seqs_in")), b"same buffer")
    for lam, kw in ((-0.5, dict(k=6, groups=3)), (float("nan"), dict(k=6, groups=3)), (float("inf"), dict(k=6, groups=3)), (0.5, {})):
        _refused(call(lam=lam, **kw), b"lambda")
    assert call(step=0, **none) == -1


def test_finalize_entry_refusals():
    names = ("n_act", "run", "seqs", "has_complete", "best_score", "best_len", "best_seq", "hyp_cnt", "hyp_score", "hyp_len", "hyp_seq", "out", "lens",
             "scores")

    def call(form=1, n_img=2, k=4, L=7, steps_done=5, n_best=2, lp_kind=0, lp_alpha=0.0, groups=1, **ptrs):
        vals = dict.fromkeys(names, P)
        vals.update(ptrs)
        return _lib().icz_test_beam_finalize(form, n_img, k, L, steps_done, n_best, lp_kind, lp_alpha, groups, *[vals[n] for n in names], None)
    for kw, word in ((dict(form=3), b"form=3"), (dict(form=-1), b"form=-1"), (dict(k=0), b"k=0"), (dict(k=9), b"k=9"), (dict(groups=2), b"groups=2"),
                     (dict(form=2, groups=3), b"groups=3"), (dict(form=0, groups=2, n_best=1), b"groups=2"), (dict(n_img=0), b"n_img=0"), (dict(n_img=1 << 20), b"n_img=1048576"),
                     (dict(steps_done=0), b"steps_done=0"), (dict(steps_done=257, L=300), b"steps_done=257"), (dict(L=5), b"L=5"),
                     (dict(n_best=0), b"n_best 0"), (dict(n_best=5), b"n_best 5"), (dict(form=0), b"n_best=2"), (dict(lp_kind=3), b"lp_kind 3"),
                     (dict(lp_alpha=-1.0), b"lp_alpha"), (dict(lp_alpha=float("nan")), b"lp_alpha")):
        _refused(call(**kw), b"icz_test_beam_finalize", word)
    for form, holes in ((0, ("n_act", "run", "seqs", "has_complete", "best_score", "best_len", "best_seq", "out", "lens")),
                        (1, ("n_act", "run", "seqs", "hyp_cnt", "hyp_score", "hyp_len", "hyp_seq", "out", "lens", "scores")),
                        (2, ("n_act", "hyp_cnt", "scores"))):
        for hole in holes:
            _refused(call(form=form, n_best=1, **{hole: None}), b"null argument")
