"""Sampling without replacement: stochastic beam search (include/icz.h: icz_*_sample_distinct; Kool, van Hoof and Welling,
"Stochastic Beams and Where to Find Them", ICML 2019).  n distinct captions per image that are exactly a sample without replacement
from the model's (tempered) sequence distribution, for one beam search of width n, with the perturbed values G the unbiased
without-replacement estimators need.  The search runs on the device (csrc/stochastic_beam.hip, csrc/sbs_kernels.h); this module
checks the arguments and shapes the results.  The entry points are functions: the handles and captioners keep their public surface."""
import ctypes as C
import math
import numbers

import torch

from ._lib import SBS_STEP_FIELDS, SampleDistinctOut, SbsStepState, check, lib, ptr, stream_ptr

MAX_N = 8


def check_args(n=5, max_len=20, temperature=1.0, vocab_size=None):
    """ValueError (before any device work) for n outside 1..8 or above the vocabulary, a temperature that is not finite or not
    positive, max_len outside 1..256 -> (n, max_len, temperature)"""
    if not isinstance(n, numbers.Integral) or isinstance(n, bool) or not 1 <= n <= MAX_N:
        raise ValueError("hypotheses per image %r outside 1..%d" % (n, MAX_N))
    if vocab_size is not None and n > vocab_size:
        raise ValueError("hypotheses per image %d above the vocabulary size %d" % (n, vocab_size))
    if not isinstance(temperature, numbers.Real) or isinstance(temperature, bool) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError("temperature %r not positive or not finite" % (temperature,))
    if not isinstance(max_len, numbers.Integral) or isinstance(max_len, bool) or not 1 <= max_len <= 256:
        raise ValueError("max_len %r outside 1..256" % (max_len,))
    return int(n), int(max_len), float(temperature)


MAX_IMAGES = 1 << 28      # first_image + n_img: the image index shares a 32-bit word of the Philox counter with the slot


def _is_int(x):
    return isinstance(x, numbers.Integral) and not isinstance(x, bool)


def rng_args(rng, max_len, n_img, n, V):
    """rng: None (seed 0), an int seed (Philox), a pair of ints (seed, first_image) -- the call holds images first_image .. of a
    batch decoded in chunks and draws that batch's noise -- or a pair (uniforms [max_len, n_img, n, V], root_uniforms [n_img]) of
    fp32 CUDA tensors with every value strictly inside (0, 1) -> (seed, first_image, uniforms, root_uniforms)"""
    if rng is None:
        return 0, 0, None, None
    if _is_int(rng):
        return int(rng) & 0xFFFFFFFFFFFFFFFF, 0, None, None
    if isinstance(rng, (tuple, list)) and len(rng) == 2 and all(_is_int(x) for x in rng):
        if not 0 <= rng[1] <= MAX_IMAGES - n_img:
            raise ValueError("first_image %d negative or first_image + %d images above %d" % (rng[1], n_img, MAX_IMAGES))
        return int(rng[0]) & 0xFFFFFFFFFFFFFFFF, int(rng[1]), None, None
    if isinstance(rng, (tuple, list)) and len(rng) == 2 and all(torch.is_tensor(t) for t in rng):
        u, root = rng
        if u.dtype != torch.float32 or root.dtype != torch.float32 or not u.is_cuda or not root.is_cuda:
            raise ValueError("explicit uniforms must be fp32 CUDA tensors")
        if tuple(u.shape) != (max_len, n_img, n, V) or tuple(root.shape) != (n_img,):
            raise ValueError("uniforms must be (%d, %d, %d, %d) and root uniforms (%d,), got %s and %s"
                             % (max_len, n_img, n, V, n_img, tuple(u.shape), tuple(root.shape)))
        return 0, 0, u.contiguous(), root.contiguous()
    raise ValueError("rng must be None, an integer seed, a pair (seed, first_image) of integers or a pair (uniforms, root_uniforms) of tensors")


def _outputs(rows, max_len, dev):
    ids = torch.zeros(rows, max_len, dtype=torch.int64, device=dev)
    lens = torch.zeros(rows, dtype=torch.int32, device=dev)
    fin = torch.zeros(rows, dtype=torch.int32, device=dev)
    phi = torch.zeros(rows, dtype=torch.float32, device=dev)
    G = torch.zeros(rows, dtype=torch.float64, device=dev)
    return (ids, lens, fin, phi, G), SampleDistinctOut(ids.data_ptr(), lens.data_ptr(), fin.data_ptr(), phi.data_ptr(), G.data_ptr())


def sample_distinct(handle, feats, n=5, max_len=20, temperature=1.0, rng=None):
    """n distinct captions per image under `handle` -- a ButdHandle / AoaHandle / NicHandle with its features, or an EnsembleHandle
    with `feats` a list of one per member (the members' averaged distribution).  rng: None / an integer Philox seed, (seed, first_image)
    for a chunk of a larger batch, or the pair of explicit uniform tensors (tests): rng_args.  Returns (ids int64 (B n, max_len) in sample_decode's format: no <sta>, <end>
    included, 0 behind it; lens int32 (B n,); finished int32 (B n,), 0 for a caption cut at max_len; phi fp32 (B n,), the caption's
    log-probability under the tempered distribution; G float64 (B n,), its perturbed value), row img * n + slot, the slots of an
    image sorted by G descending.  An image with fewer than n sequences in all (toy vocabularies only) leaves its last slots at
    length 0 with phi = G = -inf.  <pad> (0) is a token like any other: a caption that sampled it holds a 0 inside its length (only
    lens tells it from the padding), and score_captions, which ends a caption at its first 0, scores it up to there only.  ValueError, before the library is called, for bad arguments or more rows than the capacity."""
    from .ensemble import EnsembleHandle
    n, max_len, temperature = check_args(n, max_len, temperature, handle.V)
    if isinstance(handle, EnsembleHandle):
        f, n_img = handle._feats(feats)
        entry, dev = lib().icz_ensemble_sample_distinct, handle.device
    else:
        feats = handle._feats(feats)
        f, n_img, dev = ptr(feats), int(feats.shape[0]), feats.device
        entry = handle._e.sample_distinct
    if n_img * n > handle.max_rows:
        raise ValueError("%d images x %d hypotheses exceed the handle's row capacity %d" % (n_img, n, handle.max_rows))
    seed, first, uniforms, root = rng_args(rng, max_len, n_img, n, handle.V)
    outs, st = _outputs(n_img * n, max_len, dev)
    check(entry(handle._h, f, n_img, n, max_len, temperature, seed, first, ptr(uniforms), ptr(root), C.byref(st), stream_ptr()))
    return outs


def captioner_sample_distinct(captioner, visual_inputs, n=5, max_len=20, temperature=1.0, rng=None):
    """sample_distinct for a captioner (BUTDDetection / AoADetection / NICDecoder) on its `visual_inputs`, or a CaptionEnsemble on
    one `visual_inputs` per member -> (ids, lens, finished, phi, G) as sample_distinct returns them."""
    from .ensemble import CaptionEnsemble
    check_args(n, max_len, temperature)                    # ValueError before the features are looked at
    feats = captioner._feats(visual_inputs) if isinstance(captioner, CaptionEnsemble) else captioner._features(visual_inputs)
    return sample_distinct(captioner._handle(), feats, n, max_len, temperature, rng)


# ---- test entries (include/icz.h): the kernels on device tensors -------------------------------------------------------------------
def entry_rowtopk(logits, bias, nsplit, ld, n_img, n, V, step, compact, temperature, occ, frozen, phi, uniforms, seed, cand_g, cand_phi,
                  cand_idx, first_image=0):
    check(lib().icz_test_sbs_rowtopk(ptr(logits), ptr(bias), int(nsplit), int(ld), int(n_img), int(n), int(V), int(step), int(compact),
                                     float(temperature), ptr(occ), ptr(frozen), ptr(phi), ptr(uniforms), int(seed), int(first_image), ptr(cand_g),
                                     ptr(cand_phi), ptr(cand_idx), stream_ptr()))


def entry_step(state, nsplit, ld, n_img, n, V, step, L, compact=0, temperature=1.0, seed=0, first_image=0):
    """icz_test_sbs_step on `state`, a dict of device tensors keyed as icz_sbs_step_state (missing / None: null)"""
    s = SbsStepState(*[None if state.get(k) is None else state[k].data_ptr() for k in SBS_STEP_FIELDS])
    check(lib().icz_test_sbs_step(C.byref(s), int(nsplit), int(ld), int(n_img), int(n), int(V), int(step), int(L), int(compact), float(temperature),
                                  int(seed), int(first_image), stream_ptr()))


def entry_init(n_img, n, root_uniforms, seed, occ, frozen, phi, G, length, it, img_of_row, src_row, first_image=0):
    check(lib().icz_test_sbs_init(int(n_img), int(n), ptr(root_uniforms), int(seed), int(first_image), ptr(occ), ptr(frozen), ptr(phi), ptr(G), ptr(length), ptr(it),
                                  ptr(img_of_row), ptr(src_row), stream_ptr()))


def entry_finalize(n_img, n, L, occ, frozen, phi, G, length, seqs):
    outs, st = _outputs(n_img * n, L, seqs.device)
    check(lib().icz_test_sbs_finalize(int(n_img), int(n), int(L), ptr(occ), ptr(frozen), ptr(phi), ptr(G), ptr(length), ptr(seqs), C.byref(st),
                                      stream_ptr()))
    return outs


__all__ = ["sample_distinct", "captioner_sample_distinct", "check_args", "rng_args", "MAX_N"]
