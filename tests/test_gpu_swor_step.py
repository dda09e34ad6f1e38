"""The kernels of SCST on without-replacement samples alone (csrc/swor_objective.hip through icz_test_swor_objective) against the float64
statement of tests/_swor_oracle.py on the same inputs, within its counted bounds: the coefficients and stats, the gradient written
over the logits, the per-(b, t) target log-probs, the loss and its per-image parts.  Inactive rows, rows of coefficient exactly 0 and
the pad columns hold NaN on the way in and must come out as zeros; canaries sit in front of and behind every output; two runs give the
same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import _swor_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY, GUARD = 1234.5, 64          # 64 elements on both sides: the logits stay 16-byte aligned
_WANT = {}


def want_of(c):
    """inputs and the oracle's statement of a case (made once, shared, never changed)"""
    if c.name not in _WANT:
        inp = so.inputs(c)
        _WANT[c.name] = (inp, so.ref(c, inp))
    return _WANT[c.name]


def guarded(shape, dtype, fill=None):
    """a device tensor of `shape` inside a canary-filled allocation -> (the whole allocation, the view)"""
    numel = int(np.prod(shape))
    whole = torch.full((numel + 2 * GUARD,), CANARY, dtype=dtype, device=DEV)
    view = whole[GUARD:GUARD + numel].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return whole, view


def guards_intact(whole):
    return bool((whole[:GUARD] == CANARY).all()) and bool((whole[-GUARD:] == CANARY).all())


def run(c, inp):
    """one call of icz_test_swor_objective on fresh copies of the case's inputs -> the outputs and their allocations"""
    from simpleimagecaptionzoo_amd._lib import SworOpts, check, lib, ptr, stream_ptr
    B, T, n = len(inp["lengths"]), max(inp["lengths"]), c.n
    n_img = B // (n - 1)
    phi, G, scores = (torch.from_numpy(inp[k]).to(DEV) for k in ("phi", "G", "scores"))
    perm = torch.from_numpy(inp["perm"]).to(DEV)
    caps = torch.from_numpy(inp["caps"]).to(DEV)
    bufs = {"x": guarded((T * B, inp["ldl"]), torch.float32, torch.from_numpy(inp["x"])), "coef": guarded((n_img * n,), torch.float32),
            "loss_rows": guarded((T, B), torch.float32), "loss": guarded((1 + n_img,), torch.float32), "stats": guarded((n_img, 3), torch.float64)}
    o = SworOpts(n, so.ESTIMATORS.index(c.estimator), c.n_glob, phi.data_ptr(), G.data_ptr(), scores.data_ptr(), perm.data_ptr(),
                 bufs["stats"][1].data_ptr())
    rows_t = (C.c_int32 * T)(*[sum(1 for x in inp["lengths"] if x > t) for t in range(T)])
    assert bufs["x"][1].data_ptr() % 16 == 0
    check(lib().icz_test_swor_objective(C.byref(o), ptr(bufs["x"][1]), c.V, inp["ldl"], ptr(caps), T + 1, B, T, rows_t, ptr(bufs["coef"][1]),
                                        ptr(bufs["loss_rows"][1]), ptr(bufs["loss"][1]), stream_ptr()))
    torch.cuda.synchronize()
    return bufs


def within(got, want, bound, what):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    if got.size == 0:                  # (no row of the case is read)
        return
    excess = np.abs(got - want) - bound
    ratio = np.abs(got - want) / np.maximum(bound, 1e-300)             # the printed element: the one that uses most of its bound
    i = np.unravel_index(np.argmax(ratio), ratio.shape) if excess.ndim else ()
    print("%-24s max|want| %.3e  worst |err| %.3e against a bound of %.3e" % (what, np.abs(want).max(), np.abs(got - want)[i], np.asarray(bound)[i]))
    assert (excess <= 0).all(), (what, i, got[i], np.asarray(want)[i], np.asarray(bound)[i])


@pytest.mark.parametrize("c", so.CASES, ids=lambda c: c.name)
def test_kernels_alone_against_the_float64_oracle(c):
    inp, want = want_of(c)
    V, B, T, n = c.V, len(inp["lengths"]), max(inp["lengths"]), c.n
    assert T == c.T and (T == 1 or len(set(inp["lengths"])) > 1)
    runs = [run(c, inp), run(c, inp)]
    out = {k: v[1].cpu().numpy() for k, v in runs[0].items()}
    for k, (whole, _) in runs[0].items():
        assert guards_intact(whole), k
        assert torch.equal(whole, runs[1][k][0]), k                        # two runs: the same bits
    # the weights
    within(out["coef"], want["coef"], want["coef_bound"], "coef")
    assert not out["coef"][n - 1::n].any()                                 # the threshold slot
    within(out["stats"], want["stats"], want["stats_bound"], "stats {W, base, ess}")
    # the gradient: read rows within the bound, every other row and every pad column exactly 0 (they held NaN)
    g = out["x"]
    read = want["read"]
    assert read.any() or c.design == "equal"
    within(g[read][:, :V], want["g"][read], want["g_bound"][read], "d loss / d logits")
    assert not g[~read].any() and not g[:, V:].any() and np.isfinite(g).all()
    assert np.isnan(inp["x"][~read]).all() and np.isnan(inp["x"][:, V:]).all()
    # the target log-probs, the loss and its per-image parts
    within(out["loss_rows"], want["lp"], want["lp_bound"], "target log-probs")
    assert not out["loss_rows"].reshape(-1)[~read].any()
    within(out["loss"][1:], want["by_image"], want["by_image_bound"], "sum c logp by image")
    within(out["loss"][0], want["loss"], want["loss_bound"], "loss")
    if c.design == "equal" and c.estimator == "normalised":
        assert not read.any() and not out["loss"].any() and not out["coef"].any()


def test_case_table_covers_what_it_must():
    """the shapes and designs the kernels can go wrong at, counted on the inputs themselves"""
    cs = so.CASES
    assert {c.V for c in cs} >= {53, 1000, 10102} and [so.ldl_of(v) for v in (53, 1000, 10102)] == [64, 1008, 10112]
    assert {c.n for c in cs} >= {3, 5, 8} and {c.n_img for c in cs} >= {1, 3, 7} and {c.T for c in cs} >= {1, 7}
    assert {c.estimator for c in cs} == set(so.ESTIMATORS) and any(c.n_glob for c in cs) and any(not c.n_glob for c in cs)
    assert max(c.n_img * (c.n - 1) * c.T for c in cs) > 256
    d = np.concatenate([(inp["phi"].astype(np.float64).reshape(-1, c.n) - inp["G"].reshape(-1, c.n)[:, -1:])[:, :-1].reshape(-1)
                        for c in cs for inp in [want_of(c)[0]]])
    assert d.min() < -55 and d.max() > 9 and (d < so.D_SWITCH).any() and ((d > so.D_SWITCH) & (d < so.D_SWITCH + 0.01)).any()
    assert any(want_of(c)[0]["phi"].max() < -39 for c in cs)
    tg = np.concatenate([inp["caps"][:, 1].reshape(-1) for c in cs for inp in [want_of(c)[0]]])
    assert (tg == 0).any() and any(int(want_of(c)[0]["caps"][:, 1].max()) == c.V - 1 for c in cs)
    x = want_of(so.CASE_BY_NAME["v1000_n5_3img_t7"])[0]["x"][:, :1000]
    rows = x[~np.isnan(x[:, 0])]
    spread = rows.max(1) - np.median(rows, 1)
    assert (spread > 70).any() and (spread < 0.01).any()                   # a logit 80 above the rest; a near-uniform row


def test_swor_loss_is_the_same_call():
    """simpleimagecaptionzoo_amd.swor.swor_loss on a SworBatch = the entry called by hand, bit for bit"""
    from simpleimagecaptionzoo_amd.swor import SworBatch, swor_loss
    c = so.CASE_BY_NAME["zero_coef_image_n5_3img"]
    inp, _ = want_of(c)
    by_hand = run(c, inp)
    B, n = len(inp["lengths"]), c.n
    rows_of_image = torch.empty(B // (n - 1), n - 1, dtype=torch.int64)
    for b, r in enumerate(inp["perm"].tolist()):
        rows_of_image[r // n, r % n] = b
    batch = SworBatch(torch.from_numpy(inp["caps"]), list(inp["lengths"]), torch.from_numpy(inp["perm"]), rows_of_image)
    x = torch.from_numpy(inp["x"]).to(DEV)
    coef, loss_rows, loss, stats = swor_loss(x, c.V, batch, *(torch.from_numpy(inp[k]) for k in ("phi", "G", "scores")), c.estimator, c.n_glob)
    for got, k in ((x, "x"), (coef, "coef"), (loss_rows, "loss_rows"), (loss, "loss"), (stats, "stats")):
        assert torch.equal(got, by_hand[k][1]), k
