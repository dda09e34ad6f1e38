"""XE training on K captions per image (include/icz.h: icz_butd_xe_forward_n; Engine.training_epoch_grouped), host side: the batch of an
SCST-style loader -- image ids and every image's reference strings -- becomes the image-major caption rows the grouped forward takes.
Beyond the reference, whose XE loader hands every annotation over as a batch row of its own (Datasets.py:47-51)."""
import ctypes as C

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

K_MIN, K_MAX = 2, 8          # ATT_CTX_MAX_G: the rows of an image that share one workgroup of the grouped attention kernels


def check_captions_per_image(k):
    """captions_per_image as an int in 2..8; ValueError for anything else (a bool and a float included)"""
    if isinstance(k, bool) or not isinstance(k, int) or not K_MIN <= k <= K_MAX:
        raise ValueError("captions per image must be an integer in %d..%d, got %r" % (K_MIN, K_MAX, k))
    return k


def encode(vocab, sentence, max_len=None):
    """One reference string as CaptionTrainDataset encodes an annotation's tokens (Datasets.py:47-51): <sta>, the words through the
    vocabulary's <unk> fallback, <end>.  max_len: at most that many words are kept (None: all, as the reference)."""
    words = sentence.split() if isinstance(sentence, str) else list(sentence)
    if max_len is not None:
        words = words[:max_len]
    return [vocab("<sta>")] + [vocab(w) for w in words] + [vocab("<end>")]


def make_batch(vocab, img_ids, img_gts, captions_per_image, max_len=None):
    """The first K = captions_per_image reference strings of every image of `img_ids` (img_gts: image id -> list of strings), encoded
    by encode() -> (captions int64 [B K, L] zero padded, row = image * K + k in the order of img_ids; lengths: the B K token counts
    with <sta> and <end>, as the XE loader's).  L is the longest row.  Nothing is sorted.  ValueError for a bad K, a bad max_len, no
    image, or an image with fewer than K references."""
    k = check_captions_per_image(captions_per_image)
    if max_len is not None and (isinstance(max_len, bool) or not isinstance(max_len, int) or max_len < 1):
        raise ValueError("max_len must be None or a positive integer, got %r" % (max_len,))
    if len(img_ids) == 0:
        raise ValueError("a batch without images")
    rows = []
    for img_id in img_ids:
        refs = img_gts[img_id]
        if len(refs) < k:
            raise ValueError("image %r has %d references, fewer than the %d captions per image" % (img_id, len(refs), k))
        rows += [encode(vocab, s, max_len) for s in refs[:k]]
    lengths = [len(r) for r in rows]
    captions = torch.zeros(len(rows), max(lengths), dtype=torch.int64)
    for i, r in enumerate(rows):
        captions[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return captions, lengths


def xe_forward_n(h, feats, captions, lengths, K, rng=None, train=True, want_logits=False):
    """Teacher-forced XE on K = 2..8 captions per image on a ButdHandle `h` (include/icz.h: icz_butd_xe_forward_n; a function of this
    module, as multisample.sample_n and swor.swor_forward are: the handle keeps its public surface).  feats: the B images' features (or
    a RegionBatch); captions (B K, L) int64, row img * K + k with its <sta> in front, zero padded, in any length order; lengths = the
    B K caption lengths minus one.  The per-image work runs once per image; explicit rng arrays are laid out for B K rows.
    h.xe_backward then works as behind h.xe_forward.  Returns the logits (B K, T, V), zero behind a row's end, if want_logits.
    IczError, before anything is queued, for a K outside 2..8, captions / lengths that are not B K rows, B K above the handle's row
    capacity, and whatever the library refuses."""
    K = int(K)
    if not K_MIN <= K <= K_MAX:          # checked before the features are looked at
        raise _lib.IczError("xe_forward_n: K=%d captions per image outside %d..%d" % (K, K_MIN, K_MAX))
    entry = getattr(h._e, "xe_forward_n", None)
    if entry is None:
        raise _lib.IczError("xe_forward_n: the %s family has no grouped XE forward" % h.family)
    feats = h._feats(feats)
    B = feats.shape[0]
    lengths = [int(x) for x in lengths]
    if captions.dim() != 2 or captions.shape[0] != B * K or len(lengths) != B * K:
        raise _lib.IczError("xe_forward_n: captions %s and %d lengths are not %d images x %d rows" % (tuple(captions.shape), len(lengths), B, K))
    if B * K > h.max_rows:
        raise _lib.IczError("xe_forward_n: %d images x %d captions exceed the handle's row capacity %d" % (B, K, h.max_rows))
    L = captions.shape[1]
    captions = captions.to(device=feats.device, dtype=torch.int64).contiguous()
    lens = (C.c_int32 * (B * K))(*lengths)
    if train and rng is None:
        rng = h._make_rng(0)
    T = max(lengths)
    out = torch.empty(B * K, T, h.V, device=feats.device) if want_logits and 1 <= T < L else None
    check(entry(h._h, ptr(feats), ptr(captions), B, K, L, lens, C.byref(rng) if rng is not None else None, 1 if train else 0, ptr(out), stream_ptr()))
    h._live = (feats, rng, captions)
    h._xe_tokens = sum(lengths)
    return out
