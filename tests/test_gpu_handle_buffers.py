"""Which outputs of the BUTD, AoA and NIC handles are persistent buffers and which are fresh tensors.  The library's graph cache
keys on output pointers, so this is behaviour: with graphs on BUTD reuses the outputs of greedy / sample / rollouts / sample_backward,
AoA those of rollouts / sample_backward only, NIC none; with graphs off every output is a fresh tensor."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T = 2, 5


def ptrs(*tensors):
    return [t.data_ptr() for t in tensors]


def butd_handle():
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    R, D, H, E, A, V = 36, 128, 64, 64, 64, 203
    h = ButdHandle(R, D, H, E, A, V, 4, 20)
    h.bind(random_butd_params(R, D, H, E, A, V, "cuda:0", seed=3))
    torch.manual_seed(0)
    return h, torch.relu(torch.randn(B, R, D, device="cuda"))


def aoa_handle():
    from simpleimagecaptionzoo_amd.aoa import AoADetection_Captioner
    torch.manual_seed(0)
    cap = AoADetection_Captioner(53, 8, 32, 16, num_regions=36, enc_dim=2048, max_batch=4, max_beam=1).cuda()     # aoa_tiny's widths
    return cap._handle(), torch.relu(torch.randn(B, 36, 2048, device="cuda"))


def nic_handle():
    from simpleimagecaptionzoo_amd.nic import NicHandle
    from simpleimagecaptionzoo_amd.synth import random_nic_params
    E, H, V = 32, 32, 53             # nic_dec_tiny's widths
    h = NicHandle(E, H, V, 4, 20)
    h.bind(random_nic_params(E, H, V, "cuda:0", seed=3))
    torch.manual_seed(0)
    return h, torch.randn(B, E, device="cuda")


def backward_twice(h, feats):
    """(loss, mask sum) of two REINFORCE backward passes, each over a rollout of its own (a backward pass consumes the stored one)"""
    grads, rew, out = h.new_grads(), torch.ones(B, T, device="cuda"), []
    for _ in range(2):
        h.sample(feats, T)
        out.append(h.sample_backward(rew, grads))
    return out


def all_fresh(h, feats):
    """two results of every call held at once share no pointer"""
    a, b = h.greedy(feats, T), h.greedy(feats, T)
    assert a.data_ptr() != b.data_ptr()
    a, b = h.sample(feats, T), h.sample(feats, T)
    assert not set(ptrs(*a)) & set(ptrs(*b))
    a, b = h.rollouts(feats, T), h.rollouts(feats, T)
    assert not set(ptrs(*a)) & set(ptrs(*b))
    a, b = backward_twice(h, feats)
    assert not set(ptrs(*a)) & set(ptrs(*b))


def test_butd_outputs_persist_under_graphs():
    h, feats = butd_handle()
    all_fresh(h, feats)
    assert h._bufs == {}
    h.enable_graphs(True)
    assert h.greedy(feats, T).data_ptr() == h.greedy(feats, T).data_ptr()
    ids, alphas = h.greedy(feats, T, want_alphas=True)
    assert ptrs(ids, alphas) == ptrs(*h.greedy(feats, T, want_alphas=True))
    assert ptrs(*h.sample(feats, T)) == ptrs(*h.sample(feats, T))
    first = h.rollouts(feats, T)
    assert ptrs(*first) == ptrs(*h.rollouts(feats, T))
    assert first[0].data_ptr() == ids.data_ptr() and ptrs(*first[1:]) == ptrs(*h.sample(feats, T))
    a, b = backward_twice(h, feats)
    assert ptrs(*a) == ptrs(*b)
    losses = []
    for _ in range(2):
        h.xe_forward(feats, torch.ones(B, T, dtype=torch.int64), [T - 1, T - 2])
        losses.append(h.xe_backward(h.new_grads()))
    assert losses[0].data_ptr() != losses[1].data_ptr()       # the XE loss is fresh
    assert sorted(h._bufs) == [("greedy_alphas", B, T, 36), ("greedy_ids", B, T), ("rl_loss", 1), ("rl_msum", 1), ("sample_lp", B, T),
                               ("sample_seq", B, T)]
    torch.cuda.synchronize()


def test_aoa_only_rollouts_and_backward_persist_under_graphs():
    h, feats = aoa_handle()
    all_fresh(h, feats)
    assert h._bufs == {}
    h.enable_graphs(True)
    assert ptrs(*h.rollouts(feats, T)) == ptrs(*h.rollouts(feats, T))
    a, b = backward_twice(h, feats)
    assert ptrs(*a) == ptrs(*b)
    a, b = h.greedy(feats, T), h.greedy(feats, T)
    assert a.data_ptr() != b.data_ptr()
    a, b = h.sample(feats, T), h.sample(feats, T)
    assert not set(ptrs(*a)) & set(ptrs(*b))
    assert sorted(h._bufs) == [("greedy_ids", B, T), ("rl_loss", 1), ("rl_msum", 1), ("sample_lp", B, T), ("sample_seq", B, T)]
    torch.cuda.synchronize()


def test_nic_outputs_are_always_fresh():
    h, feats = nic_handle()
    all_fresh(h, feats)
    h.enable_graphs(True)
    assert h._persistent
    all_fresh(h, feats)
    assert h._bufs == {}
    torch.cuda.synchronize()
