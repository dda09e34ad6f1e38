"""Host-side owner of one libicz NIC decoder handle (Models/NIC_Model.py:39-212) and the Captioner on top of it."""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from ._lib import NIC_PARAM_KEYS, NicDims, NicParams, check, ptr, stream_ptr
from .butd import make_rng
from .handle import CaptionerBase, DecoderHandle


class NicHandle(DecoderHandle):
    family, kind = "nic", 2
    _Params, _param_keys = NicParams, NIC_PARAM_KEYS
    _make_rng = staticmethod(make_rng)
    _own_entries = ("sample_n", "xe_backward_dlogits")

    def __init__(self, E, H, V, max_rows, max_len=20, device="cuda:0"):
        self._create(NicDims(E, H, V, max_rows, max_len), device)

    def enable_graphs(self, on):      # the NIC paths are launched eagerly
        self._persistent = bool(on)

    def _feats(self, f):
        if f.dtype != torch.float32 or not f.is_cuda or f.dim() != 2 or f.shape[1] != self.E:
            raise _lib.IczError("features must be an fp32 CUDA tensor (B,%d)" % self.E)
        return f.contiguous()

    def rollouts(self, feats, max_len=20, rng=None):
        """Greedy baseline (eval mode) then the sampled rollout (train mode): Engine.py:256-261."""
        greedy = self.greedy(feats, max_len)
        seq, lp = self.sample(feats, max_len, rng)
        return greedy, seq, lp

    def sample_backward(self, reward, grads, mask_sum_global=0.0, want_dfeats=False):
        feats = self._live[0]
        reward = reward.to(device=self.device, dtype=torch.float32).contiguous()
        loss = torch.zeros(1, device=self.device)
        msum = torch.zeros(1, device=self.device)
        dfe = torch.zeros_like(feats) if want_dfeats else None
        gs = self._grad_struct(grads)
        check(self._e.sample_backward(self._h, ptr(reward), C.byref(gs), ptr(dfe), ptr(loss), ptr(msum), float(mask_sum_global),
                                      stream_ptr()))
        return (loss, msum, dfe) if want_dfeats else (loss, msum)

    def xe_backward(self, grads, smoothing=0.1, n_tokens_global=0.0, want_dfeats=False):
        feats = self._live[0]
        loss = torch.zeros(1, device=self.device)
        dfe = torch.zeros_like(feats) if want_dfeats else None
        gs = self._grad_struct(grads)
        check(self._e.xe_backward(self._h, float(smoothing), C.byref(gs), ptr(dfe), ptr(loss), float(n_tokens_global), stream_ptr()))
        return (loss, dfe) if want_dfeats else loss


class NICDecoder_Captioner(CaptionerBase, nn.Module):
    """The decoder half of NIC_Captioner (Models/NIC_Model.py:214-332) on libicz (forward :246-260, sampler :262-273, sampler_rl
    :275-287, beam_search_sampler :289-301).  The CNN encoder + img_embedding (NIC_Model.py:8-37) is outside the hot path: pass
    its output as visual_inputs['img_feats'] (B, embed_dim), or supply `encoder` (any nn.Module mapping
    visual_inputs['img_tensors'] to that embedding)."""

    _Handle = NicHandle

    def __init__(self, embed_dim, hidden_dim, vocab_size, dropout=0.5, device="cuda:0", encoder=None, max_batch=128,
                 max_beam=5, max_len=20):
        super().__init__()
        if dropout != 0.5:
            raise ValueError("the HIP path implements the reference's fixed nn.Dropout(p=0.5) (NIC_Model.py:50)")
        import math
        E, H, V = embed_dim, hidden_dim, vocab_size
        k = 1.0 / math.sqrt(H)
        U = lambda shape, b: (torch.rand(shape) * 2 - 1) * b
        self.decoder = nn.Module()
        self.decoder.embed = nn.Module()
        self.decoder.embed.register_parameter("weight", nn.Parameter(torch.randn(V, E)))       # nn.Embedding default N(0,1)
        self.decoder.lstm = nn.Module()
        for name, shape in (("weight_ih", (4 * H, E)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,))):
            self.decoder.lstm.register_parameter(name, nn.Parameter(U(shape, k)))
        v = U((V, H), k)
        self.decoder.predict = nn.Module()
        self.decoder.predict.register_parameter("bias", nn.Parameter(U((V,), k)))
        self.decoder.predict.register_parameter("weight_g", nn.Parameter(v.norm(dim=1, keepdim=True)))
        self.decoder.predict.register_parameter("weight_v", nn.Parameter(v))
        self.encoder = encoder
        self.dims = (E, H, V)
        self._decode_init(max_batch, max_beam, max_len)

    def _features(self, visual_inputs):
        if "img_feats" in visual_inputs:
            return visual_inputs["img_feats"].detach()
        if self.encoder is None:
            raise RuntimeError("no 'img_feats' in visual_inputs and no encoder module was supplied")
        return self.encoder(visual_inputs["img_tensors"]).detach()

    def eval_test_image(self, visual_inputs, caption_vocab, max_len=20, eval_beam_size=-1):
        """NIC_Model.py:306-331 -> (caption words, []): NIC has no attention maps."""
        assert self._features(visual_inputs).size(0) == 1
        if eval_beam_size != -1:
            ids = self.beam_search_sampler(visual_inputs, eval_beam_size)
        else:
            ids = self.sampler(visual_inputs, max_len)
        return self._words(ids[0], caption_vocab), []
