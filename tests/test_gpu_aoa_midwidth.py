"""AoA at model widths between the goldens and the benchmark width: tests/_fullwidth.py: AOA_MIDWIDTH lists the widths and what each is
there for (head widths 56 / 64 / 96 / 256 of the refiner's two self-attention kernels, the 48 KB LDS opt-ins, the GEMM routes that only
such a width takes; tests/test_cpu_abi_and_host.py asserts from the host predicates that it takes them).  Per width: an SCST step and an
XE step against the fp32 / float64 CPU oracle under the rules of the full-width tests (at most 2 excused near-tie and 2 CDF-edge rows,
log-probs 1e-4, loss 1e-4, gradients |HIP - f64| <= 2 |torch32 - f64| + 2e-4 max|f64|), the refiner alone, and the same device step
eagerly and under graph replay bit for bit.  With the seeds below the fp32 and the float64 oracle agree on every greedy and sampled row
of every case (counted on the CPU), so an excused row is the device's.
"""
import numpy as np
import pytest
import torch

from _fullwidth import (AOA_MIDWIDTH, AOA_SEEDS, _aoa_device_scst_runs, _aoa_model, _aoa_scst_case, _aoa_xe_case, _oracle_heads,
                        aoa_attention_routes)  # noqa: E402

pytestmark = pytest.mark.gpu

SCST_CASES = [(name, B, T) for name, (_, cases, _) in sorted(AOA_MIDWIDTH.items()) for (B, T, _) in cases]


@pytest.mark.parametrize("name,B,T", SCST_CASES, ids=["%s-%dx%d" % c for c in SCST_CASES])
def test_aoa_midwidth_scst_step_matches_oracle(name, B, T):
    """rollouts (greedy + sampled, explicit uniforms and every dropout mask) + sample_backward on the default options --
    _fullwidth._aoa_scst_case at the width's dims"""
    rep = _aoa_scst_case(AOA_MIDWIDTH[name][0], B, T, seed=AOA_SEEDS[name] + B)
    print(name, B, T, "worst", max(rep.items(), key=lambda kv: kv[1][0]))


XE_CASES = [(name, AOA_MIDWIDTH[name][1][0][0], False) for name in sorted(AOA_MIDWIDTH)] + [("a336", 20, True), ("a512", 64, True)]


@pytest.mark.parametrize("name,B,train_refiner", XE_CASES, ids=["%s-%d-%s" % (n, b, "refiner" if r else "decoder") for n, b, r in XE_CASES])
def test_aoa_midwidth_xe_step_matches_oracle(name, B, train_refiner):
    """xe_forward + xe_backward on ragged caption lengths, label smoothing 0.1 -- _fullwidth._aoa_xe_case; a336 and a512 also with
    train_refiner on: refiner_backward, mha_self_bwd_kernel and the projection gradient at head widths 56 and 64"""
    rep = _aoa_xe_case(AOA_MIDWIDTH[name][0], B, seed=AOA_SEEDS[name] + 50, train_refiner=train_refiner)
    print(name, B, train_refiner, "worst", max(rep.items(), key=lambda kv: kv[1]))


def _refiner_case(name, B=6):
    dims = AOA_MIDWIDTH[name][0]
    cap = _aoa_model(dims, 8, AOA_SEEDS[name] + 70).cuda()
    g = torch.Generator(device="cpu")
    g.manual_seed(AOA_SEEDS[name] + 71)
    feats = torch.relu(torch.randn(B, dims[0], dims[1], generator=g))
    return dims, cap, feats


@pytest.mark.parametrize("name", sorted(AOA_MIDWIDTH))
def test_aoa_midwidth_refiner_matches_oracle(name):
    """h.refine against oracle.aoa.refine (1e-4 / 1e-4, as test_aoa_random_shapes_match_oracle); on the matrix-pipe widths also against
    the blocked kernel (option mha_mfma off) within 2e-5 of max|x|, as
    test_aoa_refiner_self_attention_on_the_matrix_pipe_equals_the_blocked_kernel"""
    dims, cap, feats = _refiner_case(name)
    h = cap._handle()
    p = {k: v.detach().cpu().clone() for k, v in cap.state_dict().items()}
    got = h.refine(feats.cuda()).clone()
    with _oracle_heads(dims[5]) as oa, torch.no_grad():
        want = oa.refine(feats, p)
    print(name, "refine max|err|", float((got.cpu() - want).abs().max()), "max|x|", float(want.abs().max()))
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=1e-4, rtol=1e-4)
    if aoa_attention_routes(dims[0], dims[2], dims[5])[0]:
        h.set_option("mha_mfma", 0)
        blocked = h.refine(feats.cuda()).clone()
        h.set_option("mha_mfma", 1)
        assert (blocked - got).abs().max().item() <= 2e-5 * blocked.abs().max().item()
        np.testing.assert_allclose(blocked.cpu().numpy(), want.numpy(), atol=1e-4, rtol=1e-4)


def test_aoa_midwidth_refiner_with_region_counts_matches_oracle():
    """a512 (head width 64 on the matrix pipe) on a ragged RegionBatch: counts 1, 16, 17 and R among them (one key, a whole 16-row tile,
    one row past it, every region); the valid rows against the oracle's masked refiner and against the blocked kernel"""
    from simpleimagecaptionzoo_amd.aoa import RegionBatch
    dims, cap, feats = _refiner_case("a512")
    R_ = dims[0]
    counts = [R_, 1, 16, 17, 33, R_ - 1]
    valid = torch.arange(R_).unsqueeze(0) < torch.tensor(counts).unsqueeze(1)
    feats = feats * valid.unsqueeze(2)
    h = cap._handle()
    p = {k: v.detach().cpu().clone() for k, v in cap.state_dict().items()}
    got = h.refine(RegionBatch(feats.cuda(), counts)).clone()
    with _oracle_heads(dims[5]) as oa, torch.no_grad():
        want = oa.refine(feats, p, lens=counts)
    np.testing.assert_allclose(got.cpu()[valid].numpy(), want[valid].numpy(), atol=1e-4, rtol=1e-4)
    h.set_option("mha_mfma", 0)
    blocked = h.refine(RegionBatch(feats.cuda(), counts)).clone()
    h.set_option("mha_mfma", 1)
    assert (blocked - got)[valid.cuda()].abs().max().item() <= 2e-5 * blocked[valid.cuda()].abs().max().item()


@pytest.mark.parametrize("name", sorted(AOA_MIDWIDTH))
def test_aoa_midwidth_step_is_the_same_eagerly_and_under_graph_replay(name):
    """One handle, one SCST step (Philox dropout and draws from one seed, fixed reward) three times eagerly, then under captured graphs
    (capture, then replay): ids, log-probs, loss and every gradient tensor are the first run's, bit for bit -- what
    test_aoa_rollouts_and_backward_under_graph_replay_equal_eager_launches asserts at the benchmark width"""
    dims, cases, _ = AOA_MIDWIDTH[name]
    B, T, _ = cases[0]
    runs = _aoa_device_scst_runs(dims, B, T, AOA_SEEDS[name], [{}, {}, {}, {"graphs": 1}, {}])
    labels = ["run 1", "run 2", "run 3", "graphs 1 (capture)", "graphs 1 (replay)"]
    g0, s0, l0, loss0, grads0 = runs[0]
    assert all(torch.isfinite(v).all() for v in grads0.values()) and any(float(v.abs().max()) > 0 for v in grads0.values())
    for label, (g, s, lp, loss, grads) in zip(labels[1:], runs[1:]):
        assert torch.equal(g, g0) and torch.equal(s, s0) and torch.equal(lp, l0) and torch.equal(loss, loss0), (name, label)
        differ = [k for k in grads0 if not torch.equal(grads[k], grads0[k])]
        assert not differ, (name, label, differ, [float((grads[k] - grads0[k]).abs().max()) for k in differ])
