"""Caption sets (beyond the reference): K candidate captions per image -- n-best lists, diverse beams, ensembles, sampled captions
-- packed for the device, reranked by consensus and measured for diversity.

The device side is in csrc/ciderd.hip (include/icz.h "Caption sets"): candidates are cooked on the device (icz_ciderd_cook_device),
matched against their siblings (icz_ciderd_pairwise) or against the reference store (icz_ciderd_scores_csr), and their distinct
n-grams counted (icz_ngram_diversity).  `CiderDReward.pairwise` / `.scores_csr` (ciderd.py) call the scorer entries; this module holds
the packing, the metrics that are computed on the host from the device statistics, and `consensus_host`, the plain float64
restatement of the consensus arithmetic that the tests compare the kernels with (as `loo_baseline_reward` is for the reward).

  consensus      CIDEr-D of a candidate with the other K - 1 candidates of its image as its reference set (minimum-Bayes-risk
                 reranking keeps the candidate with the largest one);
  Div-n          distinct n-grams / total words of the set (Aneja et al., self-critical.pytorch eval_multi);
  mBLEU          corpus BLEU of every candidate against its K - 1 siblings (lower = more diverse);
  pairwise       mean off-diagonal CIDEr-D between the candidates of an image (lower = more diverse).
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_ptr

MAX_TOKENS = 60          # csrc/ciderd.hip CD_MAXT
MAX_K = 8

CandidateSet = namedtuple("CandidateSet", "tok ptr n_img K tok_host ptr_host")
CandidateSet.__doc__ = """K candidates per image in CSR form: candidate c = img * K + k is tok[ptr[c] .. ptr[c + 1]).  tok / ptr: int32 device
tensors (tok carries one spare element, so it is never an empty buffer); tok_host / ptr_host: the same as numpy arrays."""


def check_k(K, lo=1, what="samples_per_image"):
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < lo or K > MAX_K:
        raise ValueError("%s %r outside %d..%d" % (what, K, lo, MAX_K))
    return int(K)


def pack_candidates(captions_per_image, word2ix, device):
    """[[K caption strings of image 0], ...] -> CandidateSet on `device`.  Captions are split on blanks (str.split); a word outside
    `word2ix`, a caption with more than 60 words, an image with another number of captions than the first one or with none raise
    ValueError.  Empty captions are legal."""
    captions_per_image = [list(c) for c in captions_per_image]
    if not captions_per_image:
        raise ValueError("pack_candidates: no images")
    K = len(captions_per_image[0])
    if K < 1 or K > MAX_K:
        raise ValueError("pack_candidates: %d captions per image outside 1..%d" % (K, MAX_K))
    tok, off = [], [0]
    for i, caps in enumerate(captions_per_image):
        if len(caps) != K:
            raise ValueError("pack_candidates: image %d has %d captions, image 0 has %d" % (i, len(caps), K))
        for cap in caps:
            words = cap.split()
            if len(words) > MAX_TOKENS:
                raise ValueError("pack_candidates: caption with %d words: the device scorer handles at most %d" % (len(words), MAX_TOKENS))
            try:
                tok += [word2ix[w] for w in words]
            except KeyError as e:
                raise ValueError("pack_candidates: word %s is not in the vocabulary" % (e,)) from None
            off.append(len(tok))
    tok_host = np.asarray(tok + [0], dtype=np.int32)
    ptr_host = np.asarray(off, dtype=np.int32)
    dev = torch.device(device)
    return CandidateSet(torch.from_numpy(tok_host).to(dev), torch.from_numpy(ptr_host).to(dev), len(captions_per_image), K, tok_host, ptr_host)


def ngram_counts(cands):
    """int32 [n_img, 4, 2] from icz_ngram_diversity: for n = 1..4 (distinct n-grams over the image's K candidates, n-gram positions
    over them)."""
    out = torch.empty((cands.n_img, 4, 2), dtype=torch.int32, device=cands.tok.device)
    with torch.cuda.device(cands.tok.device):
        check(lib().icz_ngram_diversity(ptr(cands.tok), ptr(cands.ptr), cands.n_img, cands.K, ptr(out), stream_ptr()))
        return out.cpu().numpy()


def div_n(counts, n):
    """Div-n of Aneja et al. ("Sequential latent spaces for modeling the intention during diverse image captioning") as
    self-critical.pytorch's eval_multi computes it: the number of distinct n-grams of an image's candidate set divided by the set's
    total number of WORDS (its 1-gram count, not its n-gram count), averaged over the images.  counts: the [n_img, 4, 2] statistics
    of `ngram_counts`.  An image whose candidates are all empty contributes 0."""
    counts = np.asarray(counts)
    if n < 1 or n > 4:
        raise ValueError("div_n: n=%r outside 1..4" % (n,))
    vals = []
    for img in range(counts.shape[0]):
        words = int(counts[img, 0, 1])
        vals.append(float(int(counts[img, n - 1, 0])) / float(words) if words else 0.0)
    return float(np.mean(vals))


def mean_pairwise(pair):
    """Mean pairwise CIDEr-D of a set report: the mean of the off-diagonal entries of pair [n_img, K, K] (`CiderDReward.pairwise`),
    per image over its K (K - 1) ordered pairs, then over the images.  This is NOT the Self-CIDEr of Wang & Chan, which is built on
    the eigenvalues of the pairwise kernel matrix."""
    pair = np.asarray(pair, dtype=np.float64)
    K = pair.shape[1]
    if pair.ndim != 3 or pair.shape[2] != K or K < 2:
        raise ValueError("mean_pairwise: pair of shape %r is not [n_img, K, K] with K >= 2" % (pair.shape,))
    off = ~np.eye(K, dtype=bool)
    return float(np.mean([np.mean(pair[i][off]) for i in range(pair.shape[0])]))


def mbleu_stats(cands):
    """icz_bleu_stats of every candidate against its K - 1 siblings: int32 [n_img K, 6] (testlen, closest sibling length, clipped
    matches 1..4)."""
    n_img, K = cands.n_img, cands.K
    if K < 2:
        raise ValueError("mBLEU needs at least 2 candidates per image")
    tok, off = cands.tok_host, cands.ptr_host.astype(np.int64)
    n = n_img * K
    # reference list of candidate c = its siblings in ascending order; the tokens are copied per use (CSR rows are contiguous)
    sib = np.asarray([[b for b in range(K) if b != a] for a in range(K)], dtype=np.int64)                # [K, K - 1]
    ref_of = (np.arange(n_img, dtype=np.int64)[:, None, None] * K + sib[None]).reshape(-1)              # [n (K - 1)] candidate index
    lens = off[ref_of + 1] - off[ref_of]
    ref_ptr = np.zeros(len(ref_of) + 1, np.int64)
    ref_ptr[1:] = np.cumsum(lens)
    idx = np.repeat(off[ref_of] - ref_ptr[:-1], lens) + np.arange(int(ref_ptr[-1]), dtype=np.int64)
    ref_tok = np.concatenate([tok[idx], np.zeros(1, np.int32)]).astype(np.int32)
    img_ref_ptr = (np.arange(n + 1, dtype=np.int64) * (K - 1)).astype(np.int32)
    dev = cands.tok.device
    with torch.cuda.device(dev):
        d_tok, d_ptr, d_irp = (torch.from_numpy(a).to(dev) for a in (ref_tok, ref_ptr.astype(np.int32), img_ref_ptr))
        stats = torch.empty((n, 6), dtype=torch.int32, device=dev)
        check(lib().icz_bleu_stats(ptr(cands.tok), ptr(cands.ptr), ptr(d_tok), ptr(d_ptr), ptr(d_irp), n, ptr(stats), stream_ptr()))
        return stats.cpu().numpy()


def mbleu(cands):
    """mBLEU-1..4: the corpus BLEU of coco_eval.Bleu (option "closest") over all n_img K candidates, each scored against its K - 1
    siblings as references -> [mBleu_1, .., mBleu_4].  The integer statistics come from the device (icz_bleu_stats), the scores from
    `coco_eval.bleu_from_stats`."""
    from .coco_eval import bleu_from_stats
    return bleu_from_stats(mbleu_stats(cands))[0]


def consensus_host(cooker, captions_per_image, sigma=6.0):
    """Host restatement (tests) of icz_ciderd_pairwise in plain float64: captions_per_image = [[K caption strings], ...], cooker = a
    `ciderd.ReferenceCooker` (its df table; the candidates are cooked by its host cooker) -> (pair [n_img, K, K], consensus
    [n_img, K], best [n_img] int32).  pair[i][a][b]: sim() of ciderD_scorer.py:155-183 of a against b alone, mean over n, * 10;
    consensus[i][a]: the per-order sums of sim() over b ascending, b != a, then mean over n, / (K - 1), * 10 (compute_cider,
    :185-206, with the siblings as the reference set); best: the first largest consensus."""
    n_img = len(captions_per_image)
    K = len(captions_per_image[0])
    pen = [np.e ** (-(float(d) ** 2) / (2 * sigma ** 2)) for d in range(64)]
    pair = np.zeros((n_img, K, K), np.float64)
    cons = np.zeros((n_img, K), np.float64)
    best = np.zeros(n_img, np.int32)
    for i, (ep, keys, order, w, norm, length) in enumerate(cooker.cook_images([list(c) for c in captions_per_image])):
        vec = []
        for c in range(K):
            vec.append({(int(order[e]),) + tuple(int(x) for x in keys[e]): float(w[e]) for e in range(int(ep[c]), int(ep[c + 1]))})
        for a in range(K):
            score = [0.0] * 4
            for b in range(K):
                val = [0.0] * 4
                for g, wh in vec[a].items():                      # dict-insertion order = entry order
                    wr = vec[b].get(g, 0.0)
                    val[g[0] - 1] += min(wh, wr) * wr
                d = abs(int(length[a]) - int(length[b]))
                for n in range(4):
                    nh, nr = float(norm[a][n]), float(norm[b][n])
                    if nh != 0 and nr != 0:
                        val[n] /= (nh * nr)
                    val[n] *= pen[min(d, 63)]
                s = val[0]
                s += val[1]
                s += val[2]
                s += val[3]
                pair[i, a, b] = s / 4.0 * 10.0
                if b != a:
                    for n in range(4):
                        score[n] += val[n]
            s = score[0]
            s += score[1]
            s += score[2]
            s += score[3]
            s = s / 4.0
            if K > 1:
                s /= float(K - 1)
            cons[i, a] = s * 10.0
        best[i] = int(np.argmax(cons[i]))
    return pair, cons, best


def group_entries(entries, samples_per_image, lo=2):
    """The common argument check of the Engine's set methods: entries = [{"image_id", "caption", ...}] with samples_per_image
    consecutive entries per image -> (image ids [n_img], captions [n_img][K]).  ValueError on anything else."""
    K = check_k(samples_per_image, lo)
    entries = list(entries)
    if not entries or len(entries) % K:
        raise ValueError("%d entries are not a positive multiple of samples_per_image = %d" % (len(entries), K))
    ids, caps = [], []
    for g in range(0, len(entries), K):
        grp = entries[g:g + K]
        for e in grp:
            if not isinstance(e, dict) or "image_id" not in e or not isinstance(e.get("caption"), str):
                raise ValueError("entry %r is not a dict with 'image_id' and a 'caption' string" % (e,))
        if any(e["image_id"] != grp[0]["image_id"] for e in grp):
            raise ValueError("entries %d..%d do not belong to one image: %d consecutive entries per image are expected" % (g, g + K - 1, K))
        ids.append(grp[0]["image_id"])
        caps.append([e["caption"] for e in grp])
    return ids, caps
