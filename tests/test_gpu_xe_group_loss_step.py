"""xe_group_loss_dlogits_kernel alone (csrc/token_kernels.h through icz_test_xe_group_loss) against the float64 statement of
tests/_xe_grouped_oracle.py on the same inputs, within its counted bounds: the gradient written over the logits, the per-(row, t)
losses and the loss.  Every inactive (row, t) and the pad columns hold NaN on the way in and must come out as zeros; guard words sit
in front of and behind every output; two runs give the same bits; on lengths sorted descending the gradient and the per-row losses
are icz_test_xe_loss's bit for bit."""
import numpy as np
import pytest
import torch

import _xe_grouped_oracle as xo

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY, GUARD = 1234.5, 64          # 64 elements on both sides: the logits stay 16-byte aligned
_WANT = {}


def want_of(c):
    """inputs and the statement of a case (made once, shared, never changed)"""
    if c.name not in _WANT:
        inp = xo.inputs(c)
        _WANT[c.name] = (inp, xo.loss_ref(c, inp))
    return _WANT[c.name]


def guarded(shape, fill=None):
    numel = int(np.prod(shape))
    whole = torch.full((numel + 2 * GUARD,), CANARY, dtype=torch.float32, device=DEV)
    view = whole[GUARD:GUARD + numel].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return whole, view


def guards_intact(whole):
    return bool((whole[:GUARD] == CANARY).all()) and bool((whole[-GUARD:] == CANARY).all())


def run(c, inp, plain=False):
    """one call of icz_test_xe_group_loss (plain: of icz_test_xe_loss, for sorted lengths) on fresh copies of the case's inputs"""
    from simpleimagecaptionzoo_amd.token_choice import entry_xe_group_loss, entry_xe_loss
    rows, T = c.n_img * c.K, c.T
    caps = torch.from_numpy(inp["caps"]).to(DEV)
    lens = torch.tensor(inp["lengths"], dtype=torch.int32, device=DEV)
    n_dev = None if inp["n_dev"] is None else torch.tensor([inp["n_dev"]], dtype=torch.float32, device=DEV)
    bufs = {"x": guarded((T * rows, inp["ldl"]), torch.from_numpy(inp["x"])), "loss_rows": guarded((T * rows,)), "loss": guarded((1,))}
    assert bufs["x"][1].data_ptr() % 16 == 0
    if plain:
        rows_t = [sum(1 for x in inp["lengths"] if x > t) for t in range(T)]
        entry_xe_loss(bufs["x"][1], c.V, inp["ldl"], caps, T + 2, rows, T, rows_t, c.smoothing, xo.n_of(inp) if not inp["n_dev"] else inp["n_tokens"],
                      n_dev, bufs["loss_rows"][1], bufs["loss"][1])
    else:
        entry_xe_group_loss(bufs["x"][1], c.V, inp["ldl"], caps, T + 2, rows, T, lens, c.smoothing, inp["n_tokens"], n_dev, bufs["loss_rows"][1],
                            bufs["loss"][1])
    torch.cuda.synchronize()
    return bufs


def within(got, want, bound, what):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    excess = np.abs(got - want) - bound
    ratio = np.abs(got - want) / np.maximum(bound, 1e-300)             # the printed element: the one that uses most of its bound
    i = np.unravel_index(np.argmax(ratio), ratio.shape) if excess.ndim else ()
    print("%-24s max|want| %.3e  worst |err| %.3e against a bound of %.3e" % (what, np.abs(want).max(), np.abs(got - want)[i], np.asarray(bound)[i]))
    assert (excess <= 0).all(), (what, i, got[i], np.asarray(want)[i], np.asarray(bound)[i])


@pytest.mark.parametrize("c", xo.CASES, ids=lambda c: c.name)
def test_kernel_alone_against_the_float64_statement(c):
    inp, (g, gb, lr, rb, loss, lb, act) = want_of(c)
    V = c.V
    runs = [run(c, inp), run(c, inp)]
    out = {k: v[1].cpu().numpy() for k, v in runs[0].items()}
    for k, (whole, _) in runs[0].items():
        assert guards_intact(whole), k
        assert torch.equal(whole, runs[1][k][0]), k                        # two runs: the same bits
    x = out["x"]
    assert np.isnan(inp["x"][~act]).all() and np.isnan(inp["x"][:, V:]).all()
    within(x[act][:, :V], g[act], gb[act], "d loss / d logits")
    assert not x[~act].any() and not x[:, V:].any() and np.isfinite(x).all()      # they held NaN: exactly 0 now
    within(out["loss_rows"][act], lr[act], rb[act], "loss rows")
    assert not out["loss_rows"][~act].any()
    within(out["loss"][0], loss, lb, "loss")


@pytest.mark.parametrize("c", xo.CASES, ids=lambda c: c.name)
def test_sorted_lengths_give_the_bits_of_the_packed_kernel(c):
    """lengths sorted descending: the active (row, t) are the prefix rows_t[t], and xe_loss_dlogits_kernel takes the same logits"""
    inp = xo.inputs(c, sort=True)
    a, b = run(c, inp), run(c, inp, plain=True)
    assert torch.equal(a["x"][0], b["x"][0]) and torch.equal(a["loss_rows"][0], b["loss_rows"][0])
    assert guards_intact(a["x"][0]) and guards_intact(a["loss_rows"][0]) and guards_intact(a["loss"][0])
    assert abs(a["loss"][1].item() - b["loss"][1].item()) <= 4 * xo.U * abs(b["loss"][1].item())


def test_case_table_covers_what_it_must():
    cs = xo.CASES
    assert {c.V for c in cs} >= {53, 1000, 10102} and [xo.ldl_of(v) for v in (53, 1000, 10102)] == [64, 1008, 10112]
    assert {(c.n_img, c.K) for c in cs} == {(1, 2), (3, 5), (7, 8)} and {c.T for c in cs} == {1, 7}
    assert {c.smoothing for c in cs} == {0.0, 0.1} and {c.n for c in cs} == {"value", "dev", "none"}
    assert max(c.n_img * c.K * c.T for c in cs) > 256
    for c in cs:
        lens = want_of(c)[0]["lengths"]
        assert lens[0] == 1 and lens[1] == c.T and (c.T == 1 or lens != sorted(lens, reverse=True))
