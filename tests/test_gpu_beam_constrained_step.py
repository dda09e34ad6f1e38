"""The kernels of one constrained beam-search step and of its final ranking, each on given logits and a given state through
icz_test_beam_rowtopk_constrained, icz_test_beam_constrained_step and icz_test_beam_finalize_states (include/icz.h): the constrained
instances of both register kernels and of the sweep kernel, beam_merge_states_kernel and beam_finalize_states_kernel, against the
float64 statement of tests/_beam_constrained.py.  The cases and what each is there for: tests/_beam_constrained.py;
tests/test_cpu_beam_constrained.py holds them to it, the margin condition included.

Indices, n_act, cap, src_row, it_next, sequences, lengths, states, n_live and the list counts are compared exactly; cand_val, force_val,
run and hyp_score within the counted score bound of tests/_beam_step.py (0 for an exact row: bits).  All routes must pick the same
indices, route 0 must give the bits of the route icz_beam_rowtopk_route_for names.  Every tensor lies between guards; rows that are not
live and running scores that are not read are NaN; every slot a kernel has no business writing holds a fill that must survive."""
import numpy as np
import pytest
import torch

import _beam_constrained as bc
import _beam_step as S
from test_gpu_beam_step import NAN, Dev, _close, _exact

pytestmark = pytest.mark.gpu


def _logits(d, c, x):
    wide = np.full((x.shape[0], c.ldl), np.nan, dtype=np.float32)
    wide[:, :c.V] = x
    return d.put(wide, NAN)


def _words(d, c, inp):
    return d.put(inp["words"], S.CANARY) if inp["words"].size else None


def _rowtopk(c, inp, route):
    from simpleimagecaptionzoo_amd.constrained import entry_rowtopk
    d = Dev()
    rows = c.n_img * (c.beam << c.C)
    lg = _logits(d, c, inp["logits"])
    n_act, cap, run, seqs = d.put(inp["n_act"], S.CANARY), d.put(inp["cap"], S.CANARY), d.put(inp["run"], NAN), d.put(inp["seqs"], S.CANARY)
    val = d.put(np.full((rows, S.CAND), S.FILL, dtype=np.float32), S.FILL)
    idx = d.put(np.full((rows, S.CAND), S.CANARY, dtype=np.int32), S.CANARY)
    force = d.put(np.full((rows, bc.SLOTS), S.FILL, dtype=np.float32), S.FILL)
    entry_rowtopk(route, lg, c.n_img, c.beam, c.C, c.A, _words(d, c, inp), c.V, c.ldl, c.step, n_act, cap, run, c.compact, seqs, inp["L"], c.ngram,
                  val, idx, force)
    torch.cuda.synchronize()
    d.check()
    return val.cpu().numpy(), idx.cpu().numpy(), force.cpu().numpy()


@pytest.mark.parametrize("c", bc.CONS_CASES, ids=lambda c: c.name)
def test_row_topk_every_route_against_float64(c):
    from simpleimagecaptionzoo_amd.beam import rowtopk_route_for
    inp = bc.cons_inputs(c)
    log = []
    ref = bc.cons_rowtopk_ref(c, inp, log)
    assert all(r >= S.MARGIN for _, r in log), min(log, key=lambda e: e[1])
    got = {}
    for route in c.routes:
        val, idx, force = got[route] = _rowtopk(c, inp, route)
        for row in range(c.n_img * (c.beam << c.C)):
            n = 0
            if row in ref:
                ridx, rval, rforce, bound = ref[row]
                n = len(ridx)
                _exact(idx[row, :n], ridx, (c.name, "route", route, "row", row, "indices"))
                _close(val[row, :n], rval, bound, (c.name, "route", route, "row", row, "scores"))
                _close(force[row], rforce, bound, (c.name, "route", route, "row", row, "forced"))
            else:
                assert (force[row] == S.FILL).all(), (c.name, route, row, "force_val of a row that is not live was written")
            assert (idx[row, n:] == S.CANARY).all() and (val[row, n:] == S.FILL).all(), (c.name, route, row, "a slot that is not the row's was written")
    r0 = rowtopk_route_for(c.V, c.ldl, True)
    assert all(np.array_equal(a, b) for a, b in zip(got[0], got[r0])), (c.name, "route 0 is not route", r0)
    if 1 in got and 2 in got:
        assert np.array_equal(got[1][0], got[2][0]) and np.array_equal(got[1][2], got[2][2]), (c.name, "the two register kernels differ")


def _device_state(d, c, inp, st):
    rows = c.n_img * (c.beam << c.C)
    return {"words": _words(d, c, inp), "n_act": d.put(st["n_act"], S.CANARY), "cap": d.put(st["cap"], S.CANARY),
            "run": d.put(st["run"].astype(np.float32), NAN), "seqs_in": d.put(st["seqs_in"], S.CANARY), "seqs_out": d.put(st["seqs_out"], S.CANARY),
            "src_row": d.put(st["src_row"], S.CANARY), "it_next": d.put(st["it_next"], S.CANARY),
            "n_live": d.put(np.zeros(1, dtype=np.int32), S.CANARY), "hyp_seq": d.put(st["hyp_seq"], S.CANARY),
            "hyp_score": d.put(st["hyp_score"].astype(np.float32), S.FILL), "hyp_len": d.put(st["hyp_len"], S.CANARY),
            "hyp_state": d.put(st["hyp_state"], S.CANARY), "hyp_cnt": d.put(st["hyp_cnt"], S.CANARY),
            "cand_val": d.put(np.full((rows, S.CAND), S.FILL, dtype=np.float32), S.FILL),
            "cand_idx": d.put(np.full((rows, S.CAND), S.CANARY, dtype=np.int32), S.CANARY),
            "force_val": d.put(np.full((rows, bc.SLOTS), S.FILL, dtype=np.float32), S.FILL)}


@pytest.mark.parametrize("c", bc.CONS_CASES, ids=lambda c: c.name)
def test_step_every_route_against_float64(c):
    from simpleimagecaptionzoo_amd.constrained import entry_step
    inp = bc.cons_inputs(c)
    log = []
    ref = bc.cons_step_ref(c, inp, bc.cons_new_state(c, inp), log)
    assert all(r >= S.MARGIN for _, r in log), min(log, key=lambda e: e[1])
    b = ref["max_bound"]
    for route in c.routes:
        d = Dev()
        s = _device_state(d, c, inp, bc.cons_new_state(c, inp))
        s["logits"] = _logits(d, c, inp["logits"])
        entry_step(route, s, c.n_img, c.beam, c.C, c.A, c.V, c.ldl, c.step, inp["L"], c.compact, c.ngram)
        torch.cuda.synchronize()
        d.check()
        what = (c.name, "route", route)
        _exact(s["seqs_in"].cpu().numpy(), inp["seqs"], what + ("seqs_in was written",))
        for key in ("n_act", "cap", "src_row", "it_next", "seqs_out", "hyp_cnt", "hyp_len", "hyp_state", "hyp_seq"):
            _exact(s[key].cpu().numpy(), ref[key], what + (key,))
        assert int(s["n_live"].item()) == int(ref["n_live"]), what + ("n_live",)
        _close(s["run"].cpu().numpy(), ref["run"], b, what + ("run",))
        _close(s["hyp_score"].cpu().numpy(), ref["hyp_score"], b, what + ("hyp_score",))


@pytest.mark.parametrize("name", list(bc.CFIN_CASES))
def test_finalize_states_against_the_rules(name):
    from simpleimagecaptionzoo_amd.constrained import entry_finalize
    f = bc.CFIN_CASES[name]
    out, lens, scores, sat = bc.cons_finalize_ref(f)
    d = Dev()
    t = {key: d.put(f[key], NAN if f[key].dtype == np.float32 else S.CANARY) for key in
         ("n_act", "run", "seqs", "hyp_cnt", "hyp_score", "hyp_len", "hyp_state", "hyp_seq")}
    o = d.put(np.full(out.shape, S.FILL, dtype=np.float32), S.FILL)
    ln = d.put(np.full(lens.shape, S.CANARY, dtype=np.int32), S.CANARY)
    sc = d.put(np.full(scores.shape, S.FILL, dtype=np.float32), S.FILL)
    sa = d.put(np.full(sat.shape, S.CANARY, dtype=np.int32), S.CANARY)
    entry_finalize(f["n_img"], f["beam"], f["C"], f["L"], f["steps_done"], f["n_best"], f["lp_kind"], f["lp_alpha"], t["n_act"], t["run"], t["seqs"],
                   t["hyp_cnt"], t["hyp_score"], t["hyp_len"], t["hyp_state"], t["hyp_seq"], o, ln, sc, sa)
    torch.cuda.synchronize()
    d.check()
    _exact(o.cpu().numpy(), out, (name, "sequences"))
    _exact(ln.cpu().numpy(), lens, (name, "lengths"))
    _exact(sa.cpu().numpy(), sat, (name, "states"))
    assert np.array_equal(sc.cpu().numpy(), scores), (name, "scores")
