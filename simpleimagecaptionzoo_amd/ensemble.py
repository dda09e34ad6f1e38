"""Model ensembles (beyond the reference; self-critical.pytorch's AttEnsemble): several BUTD / AoA / NIC checkpoints of one
vocabulary decode together, greedy, with every beam-search option or by sampling (temperature, top-k, nucleus), averaging the
members' word probabilities each step (include/icz.h: icz_ensemble_*).  The members' steps and the combine kernel run on the device (csrc/ensemble.hip)."""
import ctypes as C
import math
import numbers

import torch

from . import beam as _beam
from . import sampling as _sampling
from ._lib import check, lib, ptr, stream_ptr
from .beam import nbest_lists
from .handle import CaptionerBase, DecoderHandle

MAX_MEMBERS = 4


def check_weights(weights, m):
    """None (uniform) or m finite reals >= 0 with a positive sum -> list of floats (normalised on the device); ValueError otherwise."""
    if weights is None:
        return None
    weights = list(weights)
    if len(weights) != m:
        raise ValueError("%d weights for %d members" % (len(weights), m))
    for w in weights:
        if isinstance(w, bool) or not isinstance(w, numbers.Real) or not math.isfinite(float(w)) or float(w) < 0:
            raise ValueError("weight %r: expected a finite real >= 0" % (w,))
    if sum(float(w) for w in weights) <= 0:
        raise ValueError("the weights sum to 0")
    return [float(w) for w in weights]


def check_members(n):
    if not 1 <= n <= MAX_MEMBERS:
        raise ValueError("an ensemble has 1..%d members, got %d" % (MAX_MEMBERS, n))


class EnsembleHandle:
    """Wraps icz_ensemble_* over decoder handles (ButdHandle / AoaHandle / NicHandle) of one vocabulary.  The handles stay the
    caller's (this object keeps them referenced): bound and refreshed, they decode image b of each member's features as image b."""

    def __init__(self, handles, weights=None):
        handles = list(handles)
        check_members(len(handles))
        for h in handles:
            if not isinstance(h, DecoderHandle):
                raise ValueError("ensemble member %r: expected a ButdHandle, AoaHandle or NicHandle" % (h,))
        if len({id(h) for h in handles}) != len(handles):
            raise ValueError("an ensemble member appears twice: each member needs a handle of its own")
        if len({h.V for h in handles}) != 1:
            raise ValueError("ensemble members have different vocabulary sizes %s" % [h.V for h in handles])
        w = check_weights(weights, len(handles))
        self.handles, self.V, self.device = handles, handles[0].V, handles[0].device
        self._h = C.c_void_p()
        arr_k = (C.c_int32 * len(handles))(*[h.kind for h in handles])       # icz_ensemble_create's member kinds
        arr_m = (C.c_void_p * len(handles))(*[h._h.value for h in handles])
        arr_w = (C.c_float * len(handles))(*w) if w is not None else None
        with torch.cuda.device(self.device):
            check(lib().icz_ensemble_create(arr_k, arr_m, arr_w, len(handles), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().icz_ensemble_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _feats(self, feats_list):
        """each member's features through its handle's own checks (a BUTD or AoA member's RegionBatch sets its region counts) ->
        (the host pointer array, the batch size)"""
        feats_list = list(feats_list)
        if len(feats_list) != len(self.handles):
            raise ValueError("%d feature tensors for %d members" % (len(feats_list), len(self.handles)))
        out = [h._feats(f) for h, f in zip(self.handles, feats_list)]
        sizes = {int(f.shape[0]) for f in out}
        if len(sizes) != 1:
            raise ValueError("the members' features hold different image counts %s" % sorted(sizes))
        self._keep = out           # the kernels of this call read them
        return (C.c_void_p * len(out))(*[f.data_ptr() for f in out]), sizes.pop()

    def greedy(self, feats_list, max_len=20):
        """argmax of the combined log-probabilities for max_len steps -> ids (B, max_len) int64, as the members' greedy."""
        arr, B = self._feats(feats_list)
        ids = torch.empty(B, max_len, dtype=torch.int64, device=self.device)
        check(lib().icz_ensemble_greedy(self._h, arr, B, max_len, ptr(ids), stream_ptr()))
        return ids

    def beam_search_opts(self, feats_list, beam_size=5, max_steps=50, n_best=1, length_penalty=None, block_ngram=0, groups=1, diversity=0.0):
        """The members' beam_search_opts on the combined log-probabilities: (seqs float32 (n_img, n_best, max_steps+1), lens int32
        (n_img, n_best), raw scores (n_img, n_best)); the options as ButdHandle.beam_search_opts."""
        opts = _beam.make_opts(n_best, length_penalty, block_ngram)        # ValueError before the features are looked at
        div = _beam.make_diversity(groups, diversity, beam_size)
        arr, n = self._feats(feats_list)
        m, dev = int(opts.n_best), self.device
        seqs = torch.zeros(n, m, max_steps + 1, dtype=torch.float32, device=dev)
        lens = torch.zeros(n, m, dtype=torch.int32, device=dev)
        scores = torch.zeros(n, m, dtype=torch.float32, device=dev)
        check(lib().icz_ensemble_beam_search_diverse(self._h, arr, n, beam_size, max_steps, C.byref(opts), C.byref(div), ptr(seqs), ptr(lens),
                                                      ptr(scores), stream_ptr()))
        return seqs, lens, scores

    @property
    def max_rows(self):
        """decoder rows one call may hold: the smallest member capacity"""
        return min(h.max_rows for h in self.handles)

    def sample_decode(self, feats_list, n=1, max_len=20, temperature=1.0, top_k=0, top_p=1.0, rng=None):
        """The members' sample_decode on the combined log-probabilities (include/icz.h: icz_ensemble_sample_decode): n = 1..8
        captions per image drawn from softmax(lp / temperature) restricted to the top_k largest tokens (0 = off) and then to the
        nucleus of mass top_p (1 = off).  rng: None / an integer Philox seed, or explicit uniforms (max_len, B n) fp32 on the
        device.  Returns (ids int64 (B n, max_len) with the drawn <end> and 0 behind it, the ensemble's own log-prob of every token
        (B n, max_len), their sum (B n,)), row img * n + j.  Bad options raise ValueError before the features are looked at."""
        opts = _sampling.make_sample_opts(temperature, top_k, top_p, n)
        if top_k > self.V:
            raise ValueError("top_k %d above the vocabulary size %d" % (top_k, self.V))
        seed, uniforms = _sampling.rng_args(rng)
        arr, n_img = self._feats(feats_list)
        n, max_len = int(n), int(max_len)
        rows = n_img * n
        if rows > self.max_rows:
            raise ValueError("%d images x %d samples exceed the ensemble's row capacity %d" % (n_img, n, self.max_rows))
        if uniforms is not None and tuple(uniforms.shape) != (max_len, rows):
            raise ValueError("uniforms must be (%d, %d), got %s" % (max_len, rows, tuple(uniforms.shape)))
        ids = torch.zeros(rows, max_len, dtype=torch.int64, device=self.device)
        logp = torch.zeros(rows, max_len, dtype=torch.float32, device=self.device)
        score = torch.zeros(rows, dtype=torch.float32, device=self.device)
        check(lib().icz_ensemble_sample_decode(self._h, arr, n_img, n, max_len, C.byref(opts), seed, ptr(uniforms), ptr(ids), ptr(logp),
                                                ptr(score), stream_ptr()))
        return ids, logp, score


def sample_filter_draw(members, weights, rows, V, uniforms, temperature=1.0, top_k=0, top_p=1.0):
    """icz_ensemble_sample_filter_draw (the kernel alone, tests): members = [(logits tensor, bias or None, nsplit, ld)], weights =
    None or one per member -> (tokens (rows,), logp (rows,), keep (rows, V) uint8)"""
    opts = _sampling.make_sample_opts(temperature, top_k, top_p, 1, V)
    members = list(members)
    check_members(len(members))
    w = check_weights(weights, len(members))
    M, dev = len(members), members[0][0].device
    lg = (C.c_void_p * M)(*[t.data_ptr() for t, _, _, _ in members])
    bs = (C.c_void_p * M)(*[b.data_ptr() if b is not None else None for _, b, _, _ in members])
    ns = (C.c_int32 * M)(*[int(k) for _, _, k, _ in members])
    ld = (C.c_int32 * M)(*[int(l) for _, _, _, l in members])
    arr_w = (C.c_float * M)(*w) if w is not None else None
    tok = torch.zeros(rows, dtype=torch.int64, device=dev)
    logp = torch.zeros(rows, dtype=torch.float32, device=dev)
    keep = torch.zeros(rows, V, dtype=torch.uint8, device=dev)
    check(lib().icz_ensemble_sample_filter_draw(M, lg, bs, ns, ld, arr_w, rows, V, C.byref(opts), ptr(uniforms), ptr(tok), ptr(logp), ptr(keep),
                                                 stream_ptr()))
    return tok, logp, keep


def member_features(captioner, visual_inputs):
    """The features `captioner`'s own sampler hands its handle."""
    if not isinstance(captioner, CaptionerBase):
        raise ValueError("ensemble member %r: expected a BUTD, AoA or NIC captioner" % (captioner,))
    return captioner._features(visual_inputs)


class CaptionEnsemble:
    """The Captioner decode methods over several captioners (BUTDDetection / AoADetection / NICDecoder) of one vocabulary.  Each
    method takes one `visual_inputs` per member, in member order."""

    def __init__(self, captioners, weights=None):
        self.captioners = list(captioners)
        check_members(len(self.captioners))
        for c in self.captioners:
            if not isinstance(c, CaptionerBase):
                raise ValueError("ensemble member %r: expected a BUTD, AoA or NIC captioner" % (c,))
        self.weights = check_weights(weights, len(self.captioners))
        self._ens = None

    def _handle(self):
        """the members' handles, (re)bound and refreshed as their own samplers do, under one ensemble handle"""
        handles = [c._handle() for c in self.captioners]
        if self._ens is None or any(a is not b for a, b in zip(self._ens.handles, handles)):
            self._ens = EnsembleHandle(handles, self.weights)
        return self._ens

    def _feats(self, visual_inputs_list):
        visual_inputs_list = list(visual_inputs_list)
        if len(visual_inputs_list) != len(self.captioners):
            raise ValueError("%d visual_inputs for %d members" % (len(visual_inputs_list), len(self.captioners)))
        return [member_features(c, vi) for c, vi in zip(self.captioners, visual_inputs_list)]

    def sampler(self, visual_inputs_list, max_len=20):
        """Greedy decode -> LongTensor (B, max_len)."""
        feats = self._feats(visual_inputs_list)
        return self._handle().greedy(feats, max_len)

    def beam_search_sampler(self, visual_inputs_list, beam_size=5):
        """Beam search: a batch of one image returns a (1, L) float tensor, larger batches a list of (1, L_i) tensors."""
        feats = self._feats(visual_inputs_list)
        seqs, lens, _ = self._handle().beam_search_opts(feats, beam_size, 50)
        lens = lens[:, 0].tolist()
        out = [seqs[i:i + 1, 0, :lens[i]] for i in range(len(lens))]
        return out[0] if len(out) == 1 else out

    def beam_search_nbest(self, visual_inputs_list, beam_size=5, n_best=None, length_penalty=None, block_ngram=0, groups=1, diversity=0.0):
        """Each image's n-best list as the captioners' beam_search_nbest: [(ids float32 (1, L_i), raw score)], best first."""
        opts = (beam_size if n_best is None else n_best, length_penalty, block_ngram, groups, diversity)
        _beam.make_opts(*opts[:3])
        _beam.make_diversity(groups, diversity, beam_size)
        feats = self._feats(visual_inputs_list)
        return nbest_lists(*self._handle().beam_search_opts(feats, beam_size, 50, *opts))

    def sample_decode(self, visual_inputs_list, n=1, max_len=20, temperature=1.0, top_k=0, top_p=1.0, rng=None):
        """n sampled captions per image with temperature / top-k / nucleus filtering (EnsembleHandle.sample_decode) -> (ids (B n,
        max_len), log-probs (B n, max_len), scores (B n,)), row img * n + j.  Bad options raise ValueError before any device work."""
        _sampling.make_sample_opts(temperature, top_k, top_p, n)
        _sampling.rng_args(rng)
        feats = self._feats(visual_inputs_list)
        return self._handle().sample_decode(feats, n, max_len, temperature, top_k, top_p, rng)


__all__ = ["EnsembleHandle", "CaptionEnsemble", "check_weights", "member_features", "sample_filter_draw"]
