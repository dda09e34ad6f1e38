"""Drop-in Captioner for the reference's Engine: same constructor arguments, same state_dict keys, same five
methods that Engine calls (reference class Models/BUTD_Model.py:443-544), all compute in libicz.

Two ways to train with it:
  * the reference's *unmodified* Engine.training_epoch / SCST_training_epoch work: forward() and sampler_rl()
    return tensors wired into autograd through _XEFunction / _SampleFunction, whose backward runs the HIP BPTT;
  * the Engine subclasses in engine.py call the fused entry points (loss + gradient + clamp + Adam on the device,
    no autograd graph) -- the fast path that bench.py measures.
"""
import math

import torch
import torch.nn as nn

from ._lib import BUTD_PARAM_KEYS
from .butd import ButdHandle
from .handle import CaptionerBase
from .regions import RegionBatch, region_features


class _Holder(nn.Module):
    """A module that only owns parameters (gives them the reference's dotted names)."""

    def __init__(self, **tensors):
        super().__init__()
        for k, v in tensors.items():
            self.register_parameter(k, nn.Parameter(v))


def _uniform(shape, bound):
    return (torch.rand(shape) * 2 - 1) * bound


class _DecoderParams(nn.Module):
    """Parameter tree of DecoderRNN (BUTD_Model.py:64-90) with the reference's initialisation."""

    def __init__(self, atten_dim, embed_dim, hidden_dim, vocab_size, enc_dim):
        super().__init__()
        A, E, H, V, D = atten_dim, embed_dim, hidden_dim, vocab_size, enc_dim

        def wn_linear(o, i, wbound=None, zero_bias=False):
            b = 1.0 / math.sqrt(i)
            v = _uniform((o, i), wbound if wbound is not None else b)
            bias = torch.zeros(o) if zero_bias else _uniform((o,), b)
            return _Holder(bias=bias, weight_g=v.norm(dim=1, keepdim=True), weight_v=v)

        self.atten = nn.Module()
        self.atten.enc_att = wn_linear(A, D)
        self.atten.dec_att = wn_linear(A, H)
        self.atten.affine = wn_linear(1, A)
        self.embed = nn.ModuleList([_Holder(weight=_uniform((V, E), 0.1))])      # key "embed.0.weight"
        k = 1.0 / math.sqrt(H)
        self.TD_atten = _Holder(weight_ih=_uniform((4 * H, H + D + E), k), weight_hh=_uniform((4 * H, H), k),
                                bias_ih=_uniform((4 * H,), k), bias_hh=_uniform((4 * H,), k))
        self.language_model = _Holder(weight_ih=_uniform((4 * H, D + H), k), weight_hh=_uniform((4 * H, H), k),
                                      bias_ih=_uniform((4 * H,), k), bias_hh=_uniform((4 * H,), k))
        self.predict = wn_linear(V, H, wbound=0.1, zero_bias=True)


class PackedLogits(tuple):
    """Stands in for the PackedSequence the reference returns: Engine only reads element [0] (Engine.py:182)."""
    @property
    def data(self):
        return self[0]


class _SampleFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cap, feats, max_len, rng, *params):
        seq, lp = cap._handle().sample(feats, max_len, rng)
        ctx.cap = cap
        ctx.mark_non_differentiable(seq)
        return seq, lp

    @staticmethod
    def backward(ctx, _gseq, glp):
        cap = ctx.cap
        grads = cap._grad_buffers()
        cap._handle().sample_backward_dlogp(glp, grads)
        return (None, None, None, None) + tuple(grads[k] for k in BUTD_PARAM_KEYS)


class _XEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cap, feats, captions, lengths, rng, train, *params):
        logits = cap._handle().xe_forward(feats, captions, lengths, rng, train=train, want_logits=True)
        ctx.cap = cap
        return logits

    @staticmethod
    def backward(ctx, glogits):
        cap = ctx.cap
        grads = cap._grad_buffers()
        cap._handle().xe_backward_dlogits(glogits, grads)
        return (None, None, None, None, None, None) + tuple(grads[k] for k in BUTD_PARAM_KEYS)


class BUTDDetection_Captioner(CaptionerBase, nn.Module):
    """Models/BUTD_Model.py:443-544 on libicz (sampler :478-489, beam_search_sampler :505-517).  enc_dim / num_regions default to
    the bottom-up 36 x 2048 layout (49 regions = BUTDSpatial's 7x7 grid features, the same decoder, BUTD_Model.py:321-440).
    num_regions is the handle's capacity (up to 128); a batch may be narrower.

    region_masks (beyond the reference; a plain attribute, like ss_prob, set after construction): False, the default, keeps the reference's behaviour -- its model drops `bu_masks` (:458-517), so a padded
    'adaptive' batch attends over the zero padding and divides the region mean by the padded length.  True hands the handle the
    region count of each image (`bu_counts`, or read back from the prefix `bu_masks`; a non-prefix mask raises ValueError): an
    image then decodes and trains exactly as it would alone with its own boxes."""

    _Handle = ButdHandle
    region_masks = False

    def __init__(self, atten_dim, embed_dim, hidden_dim, vocab_size, dropout=0.5, device="cuda:0", enc_dim=2048,
                 num_regions=36, max_batch=128, max_beam=5, max_len=20):
        super().__init__()
        if dropout != 0.5:
            raise ValueError("the HIP path implements the reference's fixed nn.Dropout(p=0.5) (BUTD_Model.py:66)")
        self.decoder = _DecoderParams(atten_dim, embed_dim, hidden_dim, vocab_size, enc_dim)
        self.dims = dict(R=num_regions, D=enc_dim, H=hidden_dim, E=embed_dim, A=atten_dim, V=vocab_size)
        self._decode_init(max_batch, max_beam, max_len)
        self._grads = None
        self._device = torch.device(device)

    # ---- plumbing --------------------------------------------------------------------------------
    def _new_handle(self, max_rows, max_len, device):
        d = self.dims
        return ButdHandle(d["R"], d["D"], d["H"], d["E"], d["A"], d["V"], max_rows, max_len, device)

    def _features(self, visual_inputs):
        return region_features(visual_inputs) if self.region_masks else visual_inputs["bu_feats"]

    def _grad_buffers(self):
        if self._grads is None or next(iter(self._grads.values())).device != next(self.parameters()).device:
            self._grads = {k: torch.zeros_like(p.data) for k, p in self._named().items()}
        return self._grads

    def set_seed(self, seed):
        self._seed = int(seed)

    # ---- the two methods Engine calls that are wired into autograd -------------------------------
    def forward(self, visual_inputs, captions, lengths, rng=None):
        """XE forward (BUTD_Model.py:458-476): returns an object whose [0] is the packed logits (sum(lengths), V)."""
        feats = self._features(visual_inputs)
        train = self.training
        if train and rng is None:
            rng = self._next_rng()
        params = list(self._named().values())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            logits = _XEFunction.apply(self, feats, captions, list(lengths), rng, train, *params)
        else:
            logits = self._handle().xe_forward(feats, captions, list(lengths), rng, train=train, want_logits=True)
        return PackedLogits((logits, None))

    def sampler_rl(self, visual_inputs, max_len=20, rng=None):
        """Multinomial rollout (BUTD_Model.py:491-503) -> (seq LongTensor (B,T), seqLogprobs (B,T) with grad)."""
        feats = self._features(visual_inputs)
        rng = rng or self._next_rng()
        params = list(self._named().values())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _SampleFunction.apply(self, feats, max_len, rng, *params)
        return self._handle().sample(feats, max_len, rng)

    def eval_test_image(self, visual_inputs, caption_vocab, max_len=20, eval_beam_size=-1):
        """BUTD_Model.py:519-544 -> (caption words, [alphas (1, steps, regions of the batch)]).  Greedy: the attention maps come out of the decode
        itself.  Beam search: the decoder state of a beam is a function of its token prefix, so the maps of the returned
        sentence are those of an evaluation-mode teacher-forced pass over it.  (The reference means to carry them along beam
        by beam, :282,:309-317, but appends every step's maps without the beam permutation -- `alpha.unsqueeze(1)` is not
        indexed by prev_word_inds and the history is never compacted with incomplete_inds -- so for beam > 1 its result mixes
        the maps of different beams; for beam 1 both agree, tests/test_gpu_round2.py.)"""
        feats = self._features(visual_inputs)
        raw = feats.feats if isinstance(feats, RegionBatch) else feats
        assert raw.size(0) == 1
        h = self._handle()
        if eval_beam_size != -1:
            seqs, lens = h.beam_search(feats, eval_beam_size, 50)
            n = int(lens[0])
            ids = seqs[:, :n]
            steps = n - 1                                   # one map per generated token (the leading <sta> has none, :316)
            if steps > 0:
                rh = self._replay_handle()
                rh.xe_forward(feats, ids.long(), [steps], None, train=False)
                alphas = rh.saved_alphas(1, steps)
            else:
                alphas = torch.zeros(1, 0, raw.shape[1], device=raw.device)
        else:
            ids, alphas = h.greedy(feats, max_len, want_alphas=True)
            ids, alphas = ids.clone(), alphas.clone()
        return self._words(ids[0], caption_vocab), [alphas]
