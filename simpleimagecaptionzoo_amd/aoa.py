"""Host-side owner of one libicz AoA handle (Models/AoA_Model.py) and the AoADetection Captioner on top of it.

Region sets: `'fixed'` (36 boxes, `bu_masks` None), the 7x7 grid (49) and `'adaptive'` (10..100 boxes per image, padded to
the batch's largest count with prefix `bu_masks`, AoA_Engine.py:33-46) -- the handle is created for the largest region
count it will see (`num_regions`) and every batch may be narrower."""
import copy

import torch
import torch.nn as nn

from . import _lib
from ._lib import AOA_DECODER_KEYS, AOA_PARAM_KEYS, AoaDims, AoaParams, AoaRng, check, ptr, stream_ptr
from .handle import CaptionerBase, GraphDecoderHandle
from .regions import RegionBatch, RegionSets, counts_from_masks, region_features  # noqa: F401  (RegionBatch / counts_from_masks: this module's names)

_MASKS = ("proj", "ref_att", "ref_aoa", "ref_sc", "emb", "ctx", "att", "out")


def make_aoa_rng(seed=0, uniforms=None, masks=None):
    """icz_aoa_rng: Philox streams from `seed` for everything that is not given explicitly.  `masks`: dict with any of
    proj / ref_att / ref_aoa / ref_sc / emb / ctx / att / out -> uint8 keep-mask CUDA tensors (parity tests)."""
    r = AoaRng()
    r.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    keep = []
    if uniforms is not None:
        if uniforms.dtype != torch.float32 or not uniforms.is_cuda:
            raise _lib.IczError("uniforms must be an fp32 CUDA tensor")
        uniforms = uniforms.contiguous()
        r.uniforms = uniforms.data_ptr()
        keep.append(uniforms)
    for name in _MASKS:
        m = (masks or {}).get(name)
        if m is None:
            continue
        if m.dtype != torch.uint8 or not m.is_cuda:
            raise _lib.IczError("mask %s must be a uint8 CUDA tensor" % name)
        m = m.contiguous()
        setattr(r, name + "_mask", m.data_ptr())
        keep.append(m)
    r._keep = keep
    return r


class AoaHandle(RegionSets, GraphDecoderHandle):
    family, kind = "aoa", 1
    _Params, _param_keys = AoaParams, AOA_PARAM_KEYS            # icz_aoa_params as the flat table p0..p81
    _frozen_keys = frozenset(AOA_PARAM_KEYS) - frozenset(AOA_DECODER_KEYS)
    _make_rng = staticmethod(make_aoa_rng)
    _own_entries = ("set_regions", "refine", "saved_alphas", "sample_n", "xe_backward_dlogits")

    def __init__(self, R, D, Hd, E, V, NH, max_rows, max_len=20, device="cuda:0"):
        self._create(AoaDims(R, D, Hd, E, V, NH, max_rows, max_len), device)
        self._regions_init()

    def _option_set(self, name, value):
        if name == "train_refiner":       # on: new_grads / _grad_struct cover every key, the refiner's buffers are required
            self._frozen_keys = frozenset() if value else type(self)._frozen_keys

    def set_regions(self, regions, counts=None):
        """icz_aoa_set_regions: the batches that follow are [B, regions, D]; counts = valid regions per image or None."""
        self._set_regions(regions, counts)

    def refine(self, feats):
        feats = self._feats(feats)
        out = torch.empty(feats.shape[0], feats.shape[1], self.Hd, device=feats.device)
        check(self._e.refine(self._h, ptr(feats), feats.shape[0], ptr(out), stream_ptr()))
        return out

    def saved_alphas(self, B, T, regions):
        """Head-averaged decoder attention [B, T, regions] of the forward pass the handle holds (last xe_forward / sample)."""
        out = torch.empty(B, T, regions, device=self.device)
        check(self._e.saved_alphas(self._h, ptr(out), stream_ptr()))
        return out


# ---- parameter containers with the reference's module tree (state_dict keys and shapes equal the reference's) ----------
class _Norm(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.gain = nn.Parameter(torch.ones(n))
        self.bias = nn.Parameter(torch.zeros(n))


class _Block(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.linear_Q, self.linear_K, self.linear_V = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)
        self.aoa_module = nn.Sequential(nn.Linear(2 * d, 2 * d), nn.GLU())


class _RefineLayer(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.aoa_block = _Block(d)
        self.sublayer = nn.Module()
        self.sublayer.norm = _Norm(d)


class AoADetection_Captioner(CaptionerBase, nn.Module):
    """AoADetection_Captioner (Models/AoA_Model.py:657-753) on libicz: same constructor arguments, state_dict and methods
    (forward :676-696, sampler :698-714, sampler_rl :716-734, beam_search_sampler :736-753)."""

    _Handle = AoaHandle
    # Beyond the reference (which optimises the decoder only, AoA_Model.py:669-674): True also trains aoa_refine.* and
    # img_feats_porjection.* -- get_param_groups / _trainable return every parameter and the handle's backward passes fill the
    # refiner's gradient buffers (icz_aoa_set_option "train_refiner").  A plain attribute, like ss_prob.
    train_refiner = False

    def __init__(self, vocab_size, num_heads=8, hidden_dim=1024, embed_dim=1024, dropout_aoa=0.3, dropout_prob=0.5, device="cuda:0",
                 num_regions=36, enc_dim=2048, max_batch=128, max_beam=5, max_len=20):
        super().__init__()
        if dropout_aoa != 0.3 or dropout_prob != 0.5:
            raise ValueError("the HIP path implements the reference's default drop probabilities (0.3 / 0.5 / 0.1)")
        Hd, E, V = hidden_dim, embed_dim, vocab_size
        self.img_feats_porjection = nn.Sequential(nn.Linear(enc_dim, Hd), nn.ReLU(), nn.Dropout(p=dropout_prob))
        self.aoa_refine = nn.Module()
        layer = _RefineLayer(Hd)
        self.aoa_refine.aoa_layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(6)])     # clones(): identical initial weights
        self.aoa_refine.norm = _Norm(Hd)
        dec = nn.Module()
        dec.lstm = nn.LSTMCell(E + Hd, Hd)
        dec.aoa_block = _Block(Hd)
        dec.embed = nn.Sequential(nn.Embedding(V, E), nn.ReLU(), nn.Dropout(p=dropout_prob))
        dec.h_norm = _Norm(Hd)
        dec.embed[0].weight.data.uniform_(-0.1, 0.1)
        v = torch.empty(V, Hd).uniform_(-0.1, 0.1)
        dec.predict = nn.Module()
        dec.predict.register_parameter("bias", nn.Parameter(torch.zeros(V)))
        dec.predict.register_parameter("weight_g", nn.Parameter(v.norm(dim=1, keepdim=True)))
        dec.predict.register_parameter("weight_v", nn.Parameter(v))
        self.decoder = dec
        self.dims = (num_regions, enc_dim, Hd, E, V, num_heads)
        self._decode_init(max_batch, max_beam, max_len)

    def _named(self):
        sd = dict(self.named_parameters())
        return {k: sd[k] for k in AOA_PARAM_KEYS}

    def _trainable(self):
        """The decoder's parameters; with train_refiner the projection's and the refiner's behind them (the order of the flat
        gradient buffer: the decoder's layout does not move)."""
        sd = dict(self.named_parameters())
        keys = AOA_DECODER_KEYS + (tuple(k for k in AOA_PARAM_KEYS if k not in AOA_DECODER_KEYS) if self.train_refiner else ())
        return {k: sd[k] for k in keys}

    def get_param_groups(self, lr_dict):
        """The decoder only (AoA_Model.py:669-674); with train_refiner every parameter, the decoder's first."""
        if not self.train_refiner:
            return super().get_param_groups(lr_dict)
        return [{"params": list(self._trainable().values()), "lr": lr_dict["lr"]}]

    def _push_options(self, h):
        want = bool(self.train_refiner)
        if getattr(h, "_train_refiner", False) != want:
            h.set_option("train_refiner", 1 if want else 0)
            h._train_refiner = want

    def _features(self, visual_inputs):
        """bu_feats (+ the region counts behind bu_masks: `bu_counts` when the Engine supplies them, else read back from the
        mask)."""
        return region_features(visual_inputs)

    def eval_test_image(self, visual_inputs, caption_vocab, max_len=20, eval_beam_size=-1):
        """AoA_Model.py:755-786 -> (caption words, [alphas (1, steps, regions)]): the decoder block's attention weights
        averaged over the heads (:118), taken from an evaluation-mode teacher-forced pass over the decoded sentence (the
        decoder state is a function of the token prefix, so these are the maps the reference records while decoding)."""
        feats = self._features(visual_inputs)
        raw = feats[0] if isinstance(feats, RegionBatch) else feats
        assert raw.size(0) == 1
        h = self._handle()
        if eval_beam_size != -1:
            seqs, lens = h.beam_search(feats, eval_beam_size, 50)
            ids = seqs[:, :int(lens[0])].long()
            replay = ids                                     # <sta> w1 .. wn [<end>]
        else:
            ids = h.greedy(feats, max_len)
            replay = torch.cat([torch.ones(1, 1, dtype=torch.int64, device=ids.device), ids], 1)
        steps = replay.shape[1] - 1
        if steps > 0:
            rh = self._replay_handle()
            rh.xe_forward(feats, replay, [steps], None, train=False)
            alphas = rh.saved_alphas(1, steps, raw.shape[1])
        else:
            alphas = torch.zeros(1, 0, raw.shape[1], device=raw.device)
        return self._words(ids[0], caption_vocab), [alphas]
