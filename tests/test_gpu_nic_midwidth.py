"""NIC at model widths between the goldens and the benchmark width: tests/_fullwidth.py: NIC_MIDWIDTH lists the widths and what each is
there for (the resident GEMM's four-stage, 512-deep and 128-row forms, gemm_predict over one and two k ranges, widths that are no
multiple of 64; tests/test_cpu_abi_and_host.py asserts from the host predicates that a width takes them).  Per width: an SCST step and an
XE step against the CPU oracle under the rules of test_nic_config1_size_matches_oracle (at most 2 excused near-tie and 2 CDF-edge rows,
log-probs 1e-4, loss 1e-4, gradients 2e-4), and the same device step three times bit for bit.  With the seeds below the fp32 and the
float64 oracle agree on every greedy and sampled row of every case (counted on the CPU).
"""
import pytest
import torch

from _fullwidth import NIC_MIDWIDTH, NIC_SEEDS, NIC_SHARPEN, _nic_scst_case, _nic_xe_case  # noqa: E402

pytestmark = pytest.mark.gpu

SCST_CASES = [(name, B, T) for name, (_, cases, _) in sorted(NIC_MIDWIDTH.items()) for (B, T, _) in cases]


@pytest.mark.parametrize("name,B,T", SCST_CASES, ids=["%s-%dx%d" % c for c in SCST_CASES])
def test_nic_midwidth_scst_step_matches_oracle(name, B, T):
    """greedy, sample (explicit uniforms and output-dropout masks) and sample_backward -- _fullwidth._nic_scst_case at the width's dims"""
    rep = _nic_scst_case(NIC_MIDWIDTH[name][0], B, T, seed=NIC_SEEDS[name] + B, sharpen=NIC_SHARPEN)
    print(name, B, T, "worst", max(rep.items(), key=lambda kv: kv[1]))


@pytest.mark.parametrize("name", sorted(NIC_MIDWIDTH))
def test_nic_midwidth_xe_step_matches_oracle(name):
    """xe_forward + xe_backward on ragged caption lengths (the batch shrinks with t), label smoothing 0.1 -- _fullwidth._nic_xe_case"""
    dims, cases, _ = NIC_MIDWIDTH[name]
    rep = _nic_xe_case(dims, cases[0][0], seed=NIC_SEEDS[name] + 50, sharpen=NIC_SHARPEN)
    print(name, "worst", max(rep.items(), key=lambda kv: kv[1]))


@pytest.mark.parametrize("name", sorted(NIC_MIDWIDTH))
def test_nic_midwidth_step_is_the_same_three_times(name):
    """One handle, one SCST step (Philox dropout and draws from one seed, fixed reward) three times (NIC launches eagerly): ids,
    log-probs, loss and every gradient tensor, the image embedding's too, are the first run's, bit for bit"""
    from simpleimagecaptionzoo_amd.butd import make_rng
    from simpleimagecaptionzoo_amd.nic import NicHandle
    from simpleimagecaptionzoo_amd.synth import random_nic_params
    (E_, H_, V_), cases, _ = NIC_MIDWIDTH[name]
    B, T, _ = cases[0]
    seed = NIC_SEEDS[name]
    params = random_nic_params(E_, H_, V_, "cuda", seed=seed)
    h = NicHandle(E_, H_, V_, B, T)
    h.bind(params)
    g = torch.Generator(device="cpu")
    g.manual_seed(3000 + seed)
    feats = torch.randn(B, E_, generator=g).cuda()
    rw = torch.randn(B, 1, generator=g).repeat(1, T).cuda()
    runs = []
    for _ in range(3):
        greedy, seq, lp = h.rollouts(feats, T, make_rng(seed))
        grads = h.new_grads()
        for v in grads.values():
            v.fill_(float("nan"))                   # every element is written by the backward, none accumulated
        loss, _, dfe = h.sample_backward(rw, grads, want_dfeats=True)
        torch.cuda.synchronize()
        runs.append((greedy.cpu().clone(), seq.cpu().clone(), lp.cpu().clone(), loss.cpu().clone(), dict({k: v.cpu().clone() for k, v in grads.items()}, dfeats=dfe.cpu().clone())))
    h.close()
    g0, s0, l0, loss0, grads0 = runs[0]
    assert all(torch.isfinite(v).all() for v in grads0.values()) and any(float(v.abs().max()) > 0 for v in grads0.values())
    for n, (g_, s, lp, loss, grads) in enumerate(runs[1:], 2):
        assert torch.equal(g_, g0) and torch.equal(s, s0) and torch.equal(lp, l0) and torch.equal(loss, loss0), (name, n)
        differ = [k for k in grads0 if not torch.equal(grads[k], grads0[k])]
        assert not differ, (name, n, differ)
