"""The public surface of the three decoder handles and the three captioners, and what the handles share.

SURFACE is the output of surface() at the commit before the handles got their common base (simpleimagecaptionzoo_amd/handle.py):
the base must not add, drop or re-sign a public method of any of the six classes."""
import inspect

import pytest
import torch.nn as nn

from simpleimagecaptionzoo_amd import _lib
from simpleimagecaptionzoo_amd.aoa import AoADetection_Captioner, AoaHandle
from simpleimagecaptionzoo_amd.butd import ButdHandle
from simpleimagecaptionzoo_amd.captioner import BUTDDetection_Captioner
from simpleimagecaptionzoo_amd.handle import CaptionerBase, DecoderHandle
from simpleimagecaptionzoo_amd.nic import NICDecoder_Captioner, NicHandle

HANDLES = (ButdHandle, AoaHandle, NicHandle)
CAPTIONERS = (BUTDDetection_Captioner, AoADetection_Captioner, NICDecoder_Captioner)

SURFACE = {'AoADetection_Captioner': {'__init__': '(self, vocab_size, num_heads=8, hidden_dim=1024, embed_dim=1024, dropout_aoa=0.3, dropout_prob=0.5, '
                                        "device='cuda:0', num_regions=36, enc_dim=2048, max_batch=128, max_beam=5, max_len=20)",
                            'beam_search_nbest': '(self, visual_inputs, beam_size=5, n_best=None, length_penalty=None, block_ngram=0, groups=1, '
                                                 'diversity=0.0)',
                            'beam_search_sampler': '(self, visual_inputs, beam_size=5)',
                            'eval_test_image': '(self, visual_inputs, caption_vocab, max_len=20, eval_beam_size=-1)',
                            'forward': '(self, visual_inputs, captions, lengths, rng=None)',
                            'get_param_groups': '(self, lr_dict)',
                            'sample_decode': '(self, visual_inputs, n=1, max_len=20, temperature=1.0, top_k=0, top_p=1.0, rng=None)',
                            'sampler': '(self, visual_inputs, max_len=20)',
                            'sampler_rl': '(self, visual_inputs, max_len=20, rng=None)',
                            'set_scheduled_sampling_draws': '(self, gate=None, draw=None)'},
 'AoaHandle': {'__init__': "(self, R, D, Hd, E, V, NH, max_rows, max_len=20, device='cuda:0')",
               'beam_search': '(self, feats, beam_size=5, max_steps=50)',
               'beam_search_opts': '(self, feats, beam_size=5, max_steps=50, n_best=1, length_penalty=None, block_ngram=0, groups=1, diversity=0.0)',
               'bind': '(self, tensors)',
               'close': '(self)',
               'enable_graphs': '(self, on)',
               'greedy': '(self, feats, max_len=20)',
               'new_grads': '(self)',
               'refine': '(self, feats)',
               'refresh': '(self)',
               'rollouts': '(self, feats, max_len=20, rng=None)',
               'sample': '(self, feats, max_len=20, rng=None)',
               'sample_backward': '(self, reward, grads, mask_sum_global=0.0)',
               'sample_decode': '(self, feats, n=1, max_len=20, temperature=1.0, top_k=0, top_p=1.0, rng=None)',
               'sample_mask_sum': '(self)',
               'saved_alphas': '(self, B, T, regions)',
               'set_grad_callback': '(self, fn)',
               'set_mask_sum_global': '(self, t)',
               'set_option': '(self, name, value)',
               'set_regions': '(self, regions, counts=None)',
               'set_scheduled_sampling': '(self, ss_prob, gate=None, draw=None)',
               'xe_backward': '(self, grads, smoothing=0.1, n_tokens_global=0.0)',
               'xe_forward': '(self, feats, captions, lengths, rng=None, train=True, want_logits=False)'},
 'BUTDDetection_Captioner': {'__init__': "(self, atten_dim, embed_dim, hidden_dim, vocab_size, dropout=0.5, device='cuda:0', enc_dim=2048, "
                                         'num_regions=36, max_batch=128, max_beam=5, max_len=20)',
                             'beam_search_nbest': '(self, visual_inputs, beam_size=5, n_best=None, length_penalty=None, block_ngram=0, groups=1, '
                                                  'diversity=0.0)',
                             'beam_search_sampler': '(self, visual_inputs, beam_size=5)',
                             'eval_test_image': '(self, visual_inputs, caption_vocab, max_len=20, eval_beam_size=-1)',
                             'forward': '(self, visual_inputs, captions, lengths, rng=None)',
                             'get_param_groups': '(self, lr_dict)',
                             'sample_decode': '(self, visual_inputs, n=1, max_len=20, temperature=1.0, top_k=0, top_p=1.0, rng=None)',
                             'sampler': '(self, visual_inputs, max_len=20)',
                             'sampler_rl': '(self, visual_inputs, max_len=20, rng=None)',
                             'set_scheduled_sampling_draws': '(self, gate=None, draw=None)',
                             'set_seed': '(self, seed)'},
 'ButdHandle': {'__init__': "(self, R, D, H, E, A, V, max_rows, max_len=20, device='cuda:0')",
                'beam_search': '(self, feats, beam_size=5, max_steps=50)',
                'beam_search_opts': '(self, feats, beam_size=5, max_steps=50, n_best=1, length_penalty=None, block_ngram=0, groups=1, diversity=0.0)',
                'bind': '(self, tensors)',
                'close': '(self)',
                'enable_graphs': '(self, on=True)',
                'greedy': '(self, feats, max_len=20, want_alphas=False)',
                'new_grads': '(self)',
                'refresh': '(self)',
                'rollouts': '(self, feats, max_len=20, rng=None)',
                'sample': '(self, feats, max_len=20, rng=None)',
                'sample_backward': '(self, reward, grads, mask_sum_global=0.0)',
                'sample_backward_dlogp': '(self, dlogp, grads)',
                'sample_decode': '(self, feats, n=1, max_len=20, temperature=1.0, top_k=0, top_p=1.0, rng=None)',
                'sample_mask_sum': '(self)',
                'sample_n': '(self, feats, n, max_len=20, rng=None)',
                'saved_alphas': '(self, B, T)',
                'set_concurrent': '(self, on=True)',
                'set_grad_callback': '(self, fn)',
                'set_mask_sum_global': '(self, t)',
                'set_option': '(self, name, value)',
                'set_scheduled_sampling': '(self, ss_prob, gate=None, draw=None)',
                'step': '(self, feats, it, h1, c1, h2, c2)',
                'xe_backward': '(self, grads, smoothing=0.1, n_tokens_global=0.0)',
                'xe_backward_dlogits': '(self, dpacked, grads)',
                'xe_forward': '(self, feats, captions, lengths, rng=None, train=True, want_logits=False)'},
 'NICDecoder_Captioner': {'__init__': "(self, embed_dim, hidden_dim, vocab_size, dropout=0.5, device='cuda:0', encoder=None, max_batch=128, "
                                      'max_beam=5, max_len=20)',
                          'beam_search_nbest': '(self, visual_inputs, beam_size=5, n_best=None, length_penalty=None, block_ngram=0, groups=1, '
                                               'diversity=0.0)',
                          'beam_search_sampler': '(self, visual_inputs, beam_size=5)',
                          'eval_test_image': '(self, visual_inputs, caption_vocab, max_len=20, eval_beam_size=-1)',
                          'forward': '(self, visual_inputs, captions, lengths, rng=None)',
                          'get_param_groups': '(self, lr_dict)',
                          'sample_decode': '(self, visual_inputs, n=1, max_len=20, temperature=1.0, top_k=0, top_p=1.0, rng=None)',
                          'sampler': '(self, visual_inputs, max_len=20)',
                          'sampler_rl': '(self, visual_inputs, max_len=20, rng=None)',
                          'set_scheduled_sampling_draws': '(self, gate=None, draw=None)'},
 'NicHandle': {'__init__': "(self, E, H, V, max_rows, max_len=20, device='cuda:0')",
               'beam_search': '(self, feats, beam_size=5, max_steps=50)',
               'beam_search_opts': '(self, feats, beam_size=5, max_steps=50, n_best=1, length_penalty=None, block_ngram=0, groups=1, diversity=0.0)',
               'bind': '(self, tensors)',
               'close': '(self)',
               'enable_graphs': '(self, on)',
               'greedy': '(self, feats, max_len=20)',
               'new_grads': '(self)',
               'refresh': '(self)',
               'rollouts': '(self, feats, max_len=20, rng=None)',
               'sample': '(self, feats, max_len=20, rng=None)',
               'sample_backward': '(self, reward, grads, mask_sum_global=0.0, want_dfeats=False)',
               'sample_decode': '(self, feats, n=1, max_len=20, temperature=1.0, top_k=0, top_p=1.0, rng=None)',
               'sample_mask_sum': '(self)',
               'set_mask_sum_global': '(self, t)',
               'set_scheduled_sampling': '(self, ss_prob, gate=None, draw=None)',
               'xe_backward': '(self, grads, smoothing=0.1, n_tokens_global=0.0, want_dfeats=False)',
               'xe_forward': '(self, feats, captions, lengths, rng=None, train=True, want_logits=False)'}}


def surface(cls):
    """name -> signature of __init__ and of every public callable that the class or a base of its own (not nn.Module / object) defines"""
    own = {n for k in cls.__mro__ if k not in nn.Module.__mro__ for n in vars(k)}
    names = sorted(n for n in own if n == "__init__" or not n.startswith("_"))
    return {n: str(inspect.signature(getattr(cls, n))) for n in names if callable(getattr(cls, n, None))}


@pytest.mark.parametrize("cls", HANDLES + CAPTIONERS, ids=lambda c: c.__name__)
def test_public_surface_is_unchanged(cls):
    got, want = surface(cls), SURFACE[cls.__name__]
    assert sorted(got) == sorted(want)
    assert got == want


def test_entry_tables_name_declared_symbols_only():
    lib = _lib.lib()
    for cls in HANDLES:
        table = vars(cls._entries())
        assert {"create", "destroy", "bind_params", "refresh_weights", "greedy", "sample", "sample_backward", "xe_forward", "xe_backward",
                "set_scheduled_sampling", "set_norm_global", "beam_search", "beam_search_opts", "beam_search_diverse",
                "sample_decode"} <= set(table)
        for name, fn in table.items():
            assert fn.__name__.startswith("icz_%s_" % cls.family), (cls, name, fn.__name__)
            assert fn is getattr(lib, fn.__name__) and fn.argtypes is not None, (cls, name)      # declared in _lib.lib()
        assert cls._entries() is cls._entries()                    # resolved once
    assert ButdHandle._entries().set_norm_global.__name__ == "icz_butd_set_mask_sum_global"
    assert "scst_rollouts" in vars(ButdHandle._entries()) and "scst_rollouts" in vars(AoaHandle._entries())
    # NIC has neither entry: its rollouts is greedy then sample in Python, and callers ask hasattr(h, "set_grad_callback")
    assert not {"scst_rollouts", "set_grad_callback"} & set(vars(NicHandle._entries()))
    assert not hasattr(NicHandle, "set_grad_callback") and not hasattr(NicHandle, "set_option")


def test_kinds_and_shared_methods():
    assert [(c.family, c.kind) for c in HANDLES] == [("butd", 0), ("aoa", 1), ("nic", 2)]
    assert all(issubclass(c, DecoderHandle) for c in HANDLES) and all(issubclass(c, CaptionerBase) for c in CAPTIONERS)
    for name in ("close", "bind", "refresh", "new_grads", "_buf", "_grad_struct", "sample", "xe_forward", "set_scheduled_sampling",
                 "set_mask_sum_global", "beam_search", "beam_search_opts", "sample_decode"):
        assert getattr(ButdHandle, name) is getattr(AoaHandle, name) is getattr(NicHandle, name) is getattr(DecoderHandle, name), name
    for name in ("rollouts", "sample_backward", "xe_backward", "set_option", "set_grad_callback"):
        assert getattr(ButdHandle, name) is getattr(AoaHandle, name), name
    for name in ("_handle", "_replay_handle", "_next_rng", "beam_search_sampler", "beam_search_nbest", "sample_decode", "sampler", "_words"):
        assert all(getattr(c, name) is getattr(CaptionerBase, name) for c in CAPTIONERS), name
    for c in CAPTIONERS:                                            # each captioner has its own feature hook
        assert "_features" in vars(c)


def test_no_method_is_defined_twice_in_the_subclasses():
    """no two of the family classes define a method with the same code"""
    for group in (HANDLES, CAPTIONERS):
        seen = {}
        for cls in group:
            for name, fn in vars(cls).items():
                if inspect.isfunction(fn):                          # `_make_rng = staticmethod(make_rng)` declares, it defines nothing
                    code = fn.__code__
                    key = (name, code.co_code, code.co_consts, code.co_names)
                    assert key not in seen, (name, cls.__name__, seen[key])
                    seen[key] = cls.__name__
