"""The kernels of one beam-search step and of the final selection, each on given logits and a given state through icz_test_beam_rowtopk,
icz_test_beam_step and icz_test_beam_finalize (include/icz.h): both register kernels on their list and overflow
paths, the sweep kernel in its four instances (plain / grouped, with and without the ban test; forced at small vocabularies and under
route 0 above 10240 tokens, on an odd row stride and on a base 4 bytes off), the two merges and the three finalize forms -- against the
float64 reference of tests/_beam_step.py.  The cases and what each is there for: tests/_beam_step.py; tests/test_cpu_beam_step.py holds
them to it, the margin condition included.

Indices, n_act, src_row, it_next, sequences, lengths, has_complete, n_live and the list counts are compared exactly; cand_val, run,
best_score and hyp_score within the counted score bound of tests/_beam_step.py (0 for an exact row: bits).  All routes must pick the
same indices, route 0 must give the bits of the route icz_beam_rowtopk_route_for names, and the two register kernels must give the
same bits where both take the shape.  Every tensor lies between guards; padding columns, rows that are not scored and running scores
that are not read are NaN; every slot a kernel has no business writing holds a fill that must survive."""
import numpy as np
import pytest
import torch

import _beam_step as S

pytestmark = pytest.mark.gpu

PAD = 16
NAN = float("nan")
_worst = {}              # what -> largest error / bound seen


class Dev:
    """device copies of numpy arrays, each inside a buffer of `guard` with PAD guard elements on both sides"""

    def __init__(self):
        self.items = []

    def put(self, a, guard, off=0):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a).reshape(-1)
        buf = torch.full((PAD + off + t.numel() + PAD,), guard, dtype=t.dtype, device="cuda")
        buf[PAD + off:PAD + off + t.numel()] = t.cuda()
        self.items.append((buf, PAD + off, t.numel(), guard))
        return buf[PAD + off:PAD + off + t.numel()].view(a.shape)

    def check(self):
        for buf, at, n, guard in self.items:
            g = torch.cat([buf[:at], buf[at + n:]])
            ok = torch.isnan(g).all() if guard != guard else (g == guard).all()
            assert ok.item(), "a write outside a tensor"


def _logits(d, c, x):
    """the case's logits [rows, V] in rows of stride ldl, `off` floats behind a 16-byte boundary, NaN in the padding"""
    wide = np.full((x.shape[0], c.ldl), np.nan, dtype=np.float32)
    wide[:, :c.V] = x
    t = d.put(wide, NAN, off=c.off)
    assert (t.data_ptr() % 16 == 0) == (c.off % 4 == 0)
    return t


def _close(got, ref, bound, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (got == ref) | (np.isnan(got) & np.isnan(ref)) | (np.abs(got - ref) <= bound)
        err = np.where(np.isfinite(got) & np.isfinite(ref), np.abs(got - ref), 0.0)
    if bound > 0 and err.size:
        _worst[what[-1]] = max(_worst.get(what[-1], 0.0), float(err.max()) / bound)
    assert ok.all(), (what, "first at", np.argwhere(~ok)[0].tolist(), got[~ok][:4], ref[~ok][:4], bound)


def _exact(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and (got == ref).all(), (what, "first at", np.argwhere(got != ref)[:1].tolist(), got[got != ref][:6],
                                                          ref[got != ref][:6])


# =====================================================================================================================
# row top-k
def _rowtopk(c, inp, route):
    from simpleimagecaptionzoo_amd.beam import entry_rowtopk
    d = Dev()
    rows = c.n_img * c.k
    lg = _logits(d, c, inp["logits"])
    n_act, run, seqs = d.put(inp["n_act"], S.CANARY), d.put(inp["run"], NAN), d.put(inp["seqs"], S.CANARY)
    val = d.put(np.full((rows, S.CAND), S.FILL, dtype=np.float32), S.FILL)
    idx = d.put(np.full((rows, S.CAND), S.CANARY, dtype=np.int32), S.CANARY)
    entry_rowtopk(route, lg, c.n_img, c.k, c.V, c.ldl, c.step, n_act, run, c.compact, seqs, inp["L"], c.ngram, c.groups, val, idx)
    torch.cuda.synchronize()
    d.check()
    return val.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("c", S.RT_CASES, ids=lambda c: c.name)
def test_row_topk_every_route_against_float64(c):
    from simpleimagecaptionzoo_amd.beam import rowtopk_route_for
    inp = S.case_inputs(c)
    log = []
    ref = S.rowtopk_ref(c, inp, log)
    assert all(r >= S.MARGIN for _, r in log), min(log, key=lambda e: e[1])
    got = {}
    for route in c.routes:
        val, idx = got[route] = _rowtopk(c, inp, route)
        for row in range(c.n_img * c.k):
            n = 0
            if row in ref:
                ridx, rval, bound = ref[row]
                n = len(ridx)
                _exact(idx[row, :n], ridx, (c.name, "route", route, "row", row, "indices"))
                _close(val[row, :n], rval, bound, (c.name, "route", route, "row", row, "scores"))
            assert (idx[row, n:] == S.CANARY).all() and (val[row, n:] == S.FILL).all(), (c.name, route, row, "a slot that is not the row's was written")
    r0 = rowtopk_route_for(c.V, c.ldl, c.off % 4 == 0)
    assert np.array_equal(got[0][0], got[r0][0]) and np.array_equal(got[0][1], got[r0][1]), (c.name, "route 0 is not route", r0)
    if 1 in got and 2 in got:
        assert np.array_equal(got[1][0], got[2][0]), (c.name, "the two register kernels differ in cand_val")


# =====================================================================================================================
# whole steps
def _device_state(d, c, inp, st):
    s = {"n_act": d.put(st["n_act"], S.CANARY), "run": d.put(st["run"].astype(np.float32), NAN),
         "seqs_in": d.put(st["seqs_in"], S.CANARY), "seqs_out": d.put(st["seqs_out"], S.CANARY),
         "src_row": d.put(st["src_row"], S.CANARY), "it_next": d.put(st["it_next"], S.CANARY),
         "best_score": d.put(st["best_score"].astype(np.float32), S.FILL), "best_len": d.put(st["best_len"], S.CANARY),
         "best_seq": d.put(st["best_seq"], S.CANARY), "has_complete": d.put(st["has_complete"], S.CANARY),
         "n_live": d.put(np.zeros(1, dtype=np.int32), S.CANARY),
         "cand_val": d.put(np.full((c.n_img * c.k, S.CAND), S.FILL, dtype=np.float32), S.FILL),
         "cand_idx": d.put(np.full((c.n_img * c.k, S.CAND), S.CANARY, dtype=np.int32), S.CANARY)}
    if st["hyp"] is not None:
        h = st["hyp"]
        s.update(hyp_seq=d.put(h["seq"], S.CANARY), hyp_score=d.put(h["score"].astype(np.float32), S.FILL), hyp_len=d.put(h["len"], S.CANARY),
                 hyp_cnt=d.put(h["cnt"], S.CANARY))
    return s


def _compare_state(s, st, what):
    b = st["max_bound"]
    for key in ("n_act", "src_row", "it_next", "seqs_out", "best_len", "best_seq", "has_complete"):
        _exact(s[key].cpu().numpy(), st[key], what + (key,))
    assert int(s["n_live"].item()) == int(st["n_live"]), what + ("n_live", int(s["n_live"].item()), int(st["n_live"]))
    _close(s["run"].cpu().numpy(), st["run"], b, what + ("run",))
    _close(s["best_score"].cpu().numpy(), st["best_score"], b, what + ("best_score",))
    if st["hyp"] is not None:
        for key in ("cnt", "len", "seq"):
            _exact(s["hyp_" + key].cpu().numpy(), st["hyp"][key], what + ("hyp_" + key,))
        _close(s["hyp_score"].cpu().numpy(), st["hyp"]["score"], b, what + ("hyp_score",))


@pytest.mark.parametrize("c", S.STEP_CASES, ids=lambda c: c.name)
def test_step_every_route_against_float64(c):
    from simpleimagecaptionzoo_amd.beam import entry_step
    inp = S.case_inputs(c)
    log = []
    ref = S.step_ref(c, inp, S.new_state(c, inp), log)
    assert all(r >= S.MARGIN for _, r in log), min(log, key=lambda e: e[1])
    for route in c.routes:
        d = Dev()
        s = _device_state(d, c, inp, S.new_state(c, inp))
        s["logits"] = _logits(d, c, inp["logits"])
        entry_step(route, s, c.n_img, c.k, c.V, c.ldl, c.step, inp["L"], c.compact, c.ngram, c.groups, c.lam)
        torch.cuda.synchronize()
        d.check()
        _exact(s["seqs_in"].cpu().numpy(), inp["seqs"], (c.name, route, "seqs_in was written"))
        _compare_state(s, ref, (c.name, "route", route))


@pytest.mark.parametrize("case", S.CHAIN_CASES, ids=lambda a: a[0])
def test_six_chained_steps_against_the_reference_search(case):
    from simpleimagecaptionzoo_amd.beam import entry_step
    log = []
    c, inp, lg, states = S.chain_ref(*case, log)
    assert all(r >= S.MARGIN for _, r in log), min(log, key=lambda e: e[1])
    for route in c.routes:
        d = Dev()
        s = _device_state(d, c, inp, S.new_state(c, inp))
        lgs = [_logits(d, c, x) for x in lg]
        for step in range(1, S.CHAIN_STEPS + 1):
            s["logits"] = lgs[step - 1]
            entry_step(route, s, c.n_img, c.k, c.V, c.ldl, step, inp["L"], 0, c.ngram, c.groups, c.lam)
            torch.cuda.synchronize()
            _compare_state(s, states[step - 1], (c.name, "route", route, "step", step))
            s["seqs_in"], s["seqs_out"] = s["seqs_out"], s["seqs_in"]
        d.check()


# =====================================================================================================================
# final selection
@pytest.mark.parametrize("name", list(S.FIN_CASES))
def test_finalize_forms_against_the_rules(name):
    from simpleimagecaptionzoo_amd.beam import entry_finalize
    form, f = S.FIN_CASES[name]
    log = []
    out, lens, scores = S.finalize_ref(form, f, log)
    assert all(r >= S.MARGIN for _, r in log), min(log, key=lambda e: e[1])
    d = Dev()
    t = {key: d.put(f[key], NAN if f[key].dtype == np.float32 else S.CANARY) for key in
         ("n_act", "run", "seqs", "has_complete", "best_score", "best_len", "best_seq", "hyp_cnt", "hyp_score", "hyp_len", "hyp_seq")}
    o = d.put(np.full(out.shape, S.FILL, dtype=np.float32), S.FILL)
    ln = d.put(np.full(lens.shape, S.CANARY, dtype=np.int32), S.CANARY)
    sc = d.put(np.full(scores.shape, S.FILL, dtype=np.float32), S.FILL)
    entry_finalize(form, f["n_img"], f["k"], f["L"], f["steps_done"], f["n_best"], f["lp_kind"], f["lp_alpha"], f["groups"], t["n_act"], t["run"],
                   t["seqs"], t["has_complete"], t["best_score"], t["best_len"], t["best_seq"], t["hyp_cnt"], t["hyp_score"], t["hyp_len"],
                   t["hyp_seq"], o, ln, sc)
    torch.cuda.synchronize()
    d.check()
    _exact(o.cpu().numpy(), out, (name, "sequences"))
    _exact(ln.cpu().numpy(), lens, (name, "lengths"))
    _exact(sc.cpu().numpy(), scores, (name, "scores"))


def test_zz_report_worst_error_fractions():
    """Last in the file: the largest error / bound per compared quantity over everything above (DESIGN.md section 3 quotes these)."""
    for k in sorted(_worst):
        print("beam step: %-12s worst error / bound %.3f" % (k, _worst[k]))
    assert _worst and all(f <= 1.0 for f in _worst.values())
