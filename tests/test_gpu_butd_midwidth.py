"""BUTD at model widths between the goldens (H <= 48) and the benchmark width (H = 1024): tests/_fullwidth.py: MIDWIDTH lists the widths
and what each is there for (the kernel / buffer routes of csrc/ that only such a width takes; tests/test_cpu_abi_and_host.py asserts from
the host predicates that it takes them).  Per width: an SCST step and an XE step against the fp32 / float64 CPU oracle under the rules
of the full-width tests (excused near-tie / CDF-edge rows, log-probs 1e-4, loss 1e-4, gradients |HIP - f64| <= 2 |torch32 - f64| +
2e-4 max|f64|), and the same device step under every schedule (side streams on / off, graphs on / off, three runs) bit for bit.
"""
import pytest
import torch

from _fullwidth import MIDWIDTH, _butd_scst_case, _butd_xe_case, _device_scst_runs  # noqa: E402

pytestmark = pytest.mark.gpu

SCST_CASES = [(name, B, T, kind) for name, (_, cases, _) in sorted(MIDWIDTH.items()) for (B, T, kind) in cases]
SEEDS = {"w256": 301, "w336": 302, "w512": 303, "w640": 304, "w768": 305}


@pytest.mark.parametrize("name,B,T,kind", SCST_CASES, ids=["%s-%dx%d-%s" % c for c in SCST_CASES])
def test_midwidth_scst_step_matches_oracle(name, B, T, kind):
    """rollouts (greedy + sampled, explicit uniforms and dropout masks) + sample_backward on the default options (side streams on, no
    callback) -- _fullwidth._butd_scst_case at the width's dims.  "merged": the merged greedy + sampled chain of a small batch;
    "sample_n4": 4 sampled captions per image (rowgroup_sum_kernel, att_bwd_denc_group_kernel, the per-image rows of tb.dGsum)."""
    dims = MIDWIDTH[name][0]
    options = {"merge_small": 32} if kind == "merged" else None
    rep, kink = _butd_scst_case(B, T, seed=SEEDS[name] + B, options=options, dims=dims, samples_per_image=4 if kind == "sample_n4" else 1)
    print(name, B, T, kind, "kink units", int(kink.sum()), "worst", max(v[0] for v in rep.values()))
    assert max(v[0] for v in rep.values()) < 2e-2, rep


XE_CASES = [("w256", 48, "loss"), ("w336", 20, "loss"), ("w512", 64, "loss"), ("w640", 64, "loss"), ("w768", 64, "loss"),
            ("w512", 64, "dlogits"), ("w640", 64, "callback")]


@pytest.mark.parametrize("name,B,via", XE_CASES, ids=["%s-%d-%s" % c for c in XE_CASES])
def test_midwidth_xe_step_matches_oracle(name, B, via):
    """xe_forward + xe_backward on ragged caption lengths (the batch shrinks with t), label smoothing 0.1 -- _fullwidth._butd_xe_case;
    w512 also through xe_backward_dlogits, w640 also with a gradient callback set (phases as separate calls, the attention tail on the
    caller's stream)."""
    rep, kink = _butd_xe_case(MIDWIDTH[name][0], B, seed=SEEDS[name] + 50, via=via)
    print(name, B, via, "kink units", int(kink.sum()), "worst", max(v[0] for v in rep.values()))
    assert max(v[0] for v in rep.values()) < 2e-2, rep


@pytest.mark.parametrize("name", sorted(MIDWIDTH))
def test_midwidth_backward_is_the_same_however_it_is_scheduled(name):
    """One handle, one SCST step (Philox dropout and draws from one seed, fixed reward) six times: three times in a row on the default
    options, with the side streams off (everything on the caller's stream), back on under captured graphs (capture, then replay).  Ids,
    log-probs and every gradient tensor are the first run's, bit for bit (csrc/gemm_f32.h: fixed splits, slabs summed in slab order, no
    float atomics) -- which two streams writing one slab buffer would break."""
    dims, cases, _ = MIDWIDTH[name]
    B, T, _ = cases[0]
    runs = _device_scst_runs(dims, B, T, SEEDS[name], [{}, {}, {}, {"concurrent": 0}, {"concurrent": 1, "graphs": 1}, {}])
    labels = ["run 1", "run 2", "run 3", "concurrent 0", "graphs 1 (capture)", "graphs 1 (replay)"]
    g0, s0, l0, grads0 = runs[0]
    assert all(torch.isfinite(v).all() for v in grads0.values()) and any(float(v.abs().max()) > 0 for v in grads0.values())
    for label, (g, s, lp, grads) in zip(labels[1:], runs[1:]):
        assert torch.equal(g, g0) and torch.equal(s, s0) and torch.equal(lp, l0), (name, label)
        differ = [k for k in grads0 if not torch.equal(grads[k], grads0[k])]
        assert not differ, (name, label, differ, [float((grads[k] - grads0[k]).abs().max()) for k in differ])
