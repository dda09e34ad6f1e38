"""The option "fused_dh1" of the BUTD handle (X2 = d dec . w_dec formed inside the TD-LSTM backward launch of a BPTT step) changes no bit:
SCST rollouts + REINFORCE backward at 3 (a merged chain), 33 and 64 images and a teacher-forced XE forward / backward over ragged
lengths, each with the option on and off and with captured graphs on and off -- the loss and every gradient are the same bits in all
four, and under graphs in the captured call and in its replay.  One sequence flips the option between backward calls of one handle
under graphs: the option is part of the graph key, so a captured backward of one route is never replayed for the other.

H = A = E = D = 64 (widths the fused kernel takes), 5 regions, 37 words, 4 steps."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R, D, H, E, A, V, T = 5, 64, 64, 64, 64, 37, 4
DEV = "cuda"


def _handle(B, fused, graphs, params):
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    h = ButdHandle(R, D, H, E, A, V, B, T)
    h.bind({k: v.clone() for k, v in params.items()})
    h.set_option("fused_dh1", fused)
    h.enable_graphs(graphs)
    return h


def _feats(B, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.relu(torch.randn(B, R, D, generator=g)).to(DEV)


def _backward(h, step, grads=None):
    """one backward call into NaN-filled buffers (the given ones: under graphs the same buffers make the call a replay) -> (loss, {name: gradient})"""
    grads = grads or h.new_grads()
    for v in grads.values():
        v.fill_(float("nan"))
    loss = step(grads)
    torch.cuda.synchronize()
    out = {k: v.clone() for k, v in grads.items()}
    assert all(torch.isfinite(v).all().item() for v in out.values()), "a gradient that is not finite"
    return loss.clone(), out


def _assert_same(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "loss", a[0].item(), b[0].item())
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), (what, k, (a[1][k] - b[1][k]).abs().max().item())


@pytest.fixture(scope="module")
def params():
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    return random_butd_params(R, D, H, E, A, V, DEV, seed=5)


@pytest.mark.parametrize("B", (3, 33, 64))
def test_scst_backward_is_the_same_bits_with_the_option_on_and_off_graphs_on_and_off(B, params):
    from simpleimagecaptionzoo_amd.butd import make_rng
    feats = _feats(B, 11 + B)
    reward = torch.tensor(np.random.RandomState(B).randn(B, 1).astype(np.float32).repeat(T, 1), device=DEV)
    runs = {}
    for fused, graphs in itertools.product((1, 0), (1, 0)):
        h = _handle(B, fused, graphs, params)
        grads, rng = h.new_grads(), make_rng(7)
        runs[(fused, graphs)] = []
        for _ in range(2):                        # (a backward call consumes the stored rollout)
            _, seq, lp = h.rollouts(feats, T, rng)
            runs[(fused, graphs)].append((seq.clone(), lp.clone()))
            runs[(fused, graphs)].append(_backward(h, lambda g: h.sample_backward(reward, g)[0], grads))
        h.close()
    base = runs[(0, 0)]
    for key, r in runs.items():
        for i in (0, 2):
            assert torch.equal(r[i][0], base[0][0]) and torch.equal(r[i][1], base[0][1]), (key, "the rollouts differ")
        _assert_same(r[1], base[1], (B, key, "first backward"))
        _assert_same(r[3], base[1], (B, key, "second backward (graphs: the replay)"))


def test_xe_backward_over_ragged_lengths_is_the_same_bits_with_the_option_on_and_off(params):
    """33 captions of 2 .. 5 tokens: the batch grows from 3 rows at the last step to 33 at the first (rows_a < rows in every step but the last)"""
    from simpleimagecaptionzoo_amd.butd import make_rng
    B, L = 33, T + 1
    rs = np.random.RandomState(3)
    lens = sorted([5] * 3 + [4] * 9 + [3] * 12 + [2] * 9, reverse=True)
    caps = torch.zeros(B, L, dtype=torch.int64)
    for b, n in enumerate(lens):
        caps[b, 0] = 1
        caps[b, 1:n - 1] = torch.from_numpy(rs.randint(4, V, size=n - 2))
        caps[b, n - 1] = 2
    steps = [n - 1 for n in lens]
    feats = _feats(B, 2)
    runs = {}
    for fused, graphs in itertools.product((1, 0), (1, 0)):
        h = _handle(B, fused, graphs, params)
        h.xe_forward(feats, caps.to(DEV), steps, make_rng(9), train=True)
        runs[(fused, graphs)] = _backward(h, lambda g: h.xe_backward(g))
        h.close()
    for key, r in runs.items():
        _assert_same(r, runs[(0, 0)], ("xe", key))


def test_flipping_the_option_between_backward_calls_under_graphs(params):
    """graphs on: capture with the fused step, replay, flip to the two launches (a capture of its own), replay, flip back (the first
    graph again) -- every call gives the bits of an eager handle with the option off"""
    from simpleimagecaptionzoo_amd.butd import make_rng
    B = 33
    feats = _feats(B, 21)
    reward = torch.tensor(np.random.RandomState(1).randn(B, 1).astype(np.float32).repeat(T, 1), device=DEV)
    ref_h = _handle(B, 0, 0, params)
    ref_h.rollouts(feats, T, make_rng(4))
    want = _backward(ref_h, lambda g: ref_h.sample_backward(reward, g)[0])
    ref_h.close()
    h = _handle(B, 1, 1, params)
    grads, rng = h.new_grads(), make_rng(4)       # one set of buffers: the graph key holds their pointers, so the calls below replay

    def again():
        h.rollouts(feats, T, rng)                 # (a backward call consumes the stored rollout)
        for v in grads.values():
            v.fill_(float("nan"))
        loss = h.sample_backward(reward, grads)[0]
        torch.cuda.synchronize()
        return loss.clone(), {k: v.clone() for k, v in grads.items()}

    for i, fused in enumerate((1, 1, 0, 0, 1, 0)):
        h.set_option("fused_dh1", fused)
        _assert_same(again(), want, ("call", i, "fused_dh1", fused))
    h.close()
