"""Evaluation metrics of the step that follows `Engine.eval_captions_json_generation`: corpus CIDEr
(`coco_eval`, what Engine.training keeps) and the evaluation report's Bleu_1..4, ROUGE_L and CIDEr (`evaluate_captions`).

The reference scores the generated captions with `coco_eval` (COCO_Eval_Utils.py:15-35): pycocotools loads the annotation
file, a Java PTB tokeniser splits references and candidates, and `Cider().compute_score` (coco_caption/pycocoevalcap/cider/
cider.py:34-56 -> cider_scorer.py:96-195) returns the corpus CIDEr.  Neither pycocotools nor the Stanford jar is needed here:

  * `load_annotations` reads the COCO caption json directly ({image_id: [caption, ...]}, what COCO.imgToAnns holds);
  * `ptb_lite_tokenize` is a rule-based stand-in for `PTBTokenizer -preserveLines -lowerCase` followed by the reference's
    punctuation filter (ptbtokenizer.py:24-25,66-68).  PARITY UNPINNED: the jar cannot run in this image, so there are
    no golden vectors for the tokeniser itself (it agrees with PTB on plain captions; rare symbols may differ).  The rules that are
    implemented are the documented Penn-Treebank conventions (contractions n't / 's / 're / 've / 'll / 'd / 'm split off,
    cannot -> can not, gonna -> gon na, brackets to -lrb- / -rrb-, $ % & # as tokens, digit groups like 1,000 and 3:30
    kept whole, sentence-final periods split, abbreviations kept), each with an explicit expectation in
    tests/test_cpu_abi_and_host.py;
  * `Cider.compute_score` scores on the device with the CIDEr-D kernel of the SCST reward (csrc/ciderd.hip): the
    per-image formula is the same (clipped tf-idf cosine x Gaussian length penalty), only the document frequencies differ
    -- here they are counted over the evaluated references themselves (cider_scorer.py:96-107,164).  Scores are bit-exact
    against the reference scorer (tests/golden/corpus_cider_cases.json).
  * `Bleu.compute_score` / `Rouge.compute_score` restate bleu.py:24-47 -> bleu_scorer.py (option "closest") and rouge.py:38-104.
    The device counts integers only (csrc/coco_metrics.hip: testlen, closest reference length and clipped n-gram matches per
    image; LCS length per reference, bit-parallel); the scores are computed from them on the host with the reference's float
    arithmetic in its order, so they are bit-exact (tests/golden/coco_metric_cases.json).  `evaluate_captions` runs Bleu, Rouge
    and Cider in the order of eval.py:24-69.  METEOR and SPICE are not computed: both are Java programs (meteor-1.5.jar,
    spice-1.0.jar) that this project does not run.
"""
import json
import math
import re
from itertools import chain

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_ptr
from .ciderd import CiderDReward
from .synth import document_frequency

# ptbtokenizer.py:24-25 -- compared AFTER lower-casing, so the bracket names of the list can never match (kept as is)
PUNCTUATIONS = ["''", "'", "``", "`", "-LRB-", "-RRB-", "-LCB-", "-RCB-", ".", "?", "!", ",", ":", "-", "--", "...", ";"]

_BRACKETS = {"(": "-lrb-", ")": "-rrb-", "[": "-lsb-", "]": "-rsb-", "{": "-lcb-", "}": "-rcb-"}
_ABBREV = {"mr.", "mrs.", "ms.", "dr.", "st.", "jr.", "sr.", "vs.", "etc.", "no.", "inc.", "co.", "ave.", "mt."}      # kept with their period
_CONTRACTION = re.compile(r"(?i)\b(can)(not)\b")
_SUFFIX = re.compile(r"(?i)([a-z0-9])('ll|'re|'ve|n't|'s|'m|'d)\b")
_SPLIT = re.compile(r"(\.\.\.|--|[\"(){}\[\]?!;$%&#]|(?<!\d)[,:]|[,:](?!\d)|``|'')")      # "1,000" and "3:30" stay whole


def ptb_lite_tokenize(sentence):
    """One caption -> lower-cased, space-joined PTB-style tokens without punctuation tokens."""
    s = sentence.replace("\n", " ").lower()
    s = _CONTRACTION.sub(r"\1 \2", s)
    s = re.sub(r"\b(gon|wan)(na)\b|\b(got)(ta)\b|\b(lem|gim)(me)\b", lambda m: " ".join(g for g in m.groups() if g), s)   # PTB: gon na, got ta, lem me
    s = _SUFFIX.sub(r"\1 \2", s)
    s = _SPLIT.sub(r" \1 ", s)
    out = []
    for tok in s.split():
        if tok == '"':
            tok = "''"
        tok = _BRACKETS.get(tok, tok)
        # a sentence-final period is its own token; periods inside abbreviations / numbers stay attached
        while len(tok) > 1 and tok.endswith(".") and tok not in _ABBREV and not re.fullmatch(r"\.+|([a-z]\.)+|\d+(\.\d+)+\.?", tok):
            tok = tok[:-1]
            out.append(tok)
            tok = "."
        # leading / trailing apostrophes are quote tokens; word-internal ones ("o'clock") stay
        while len(tok) > 1 and tok.startswith("'") and tok not in ("'ll", "'re", "'ve", "'s", "'m", "'d"):
            out.append("'")
            tok = tok[1:]
        if len(tok) > 1 and tok.endswith("'") and tok != "''":
            out.append(tok[:-1])
            tok = "'"
        out.append(tok)
    return " ".join(w for w in out if w not in PUNCTUATIONS)


def tokenize(captions_for_image):
    """PTBTokenizer.tokenize (ptbtokenizer.py:30-70): {id: [{'caption': str}, ...]} -> {id: [tokenised str, ...]}."""
    return {k: [ptb_lite_tokenize(c["caption"]) for c in v] for k, v in captions_for_image.items()}


def load_annotations(path):
    """{image_id: [{'caption': ...}, ...]} from a COCO caption annotation file (COCO.imgToAnns of pycocotools)."""
    data = json.load(open(path, "r", encoding="utf-8"))
    out = {}
    for ann in data["annotations"]:
        out.setdefault(ann["image_id"], []).append({"caption": ann["caption"]})
    return out


def _check_pairs(gts, res):
    """The scorers' common contract (bleu.py:26-37, rouge.py:83-96, cider.py:34-49): the same keys in the same order, one
    candidate and at least one reference per image -> the image ids."""
    ids = list(gts.keys())
    assert list(res.keys()) == ids
    for i in ids:
        assert type(res[i]) is list and len(res[i]) == 1
        assert type(gts[i]) is list and len(gts[i]) > 0
    return ids


def _check_length(T, max_tokens):
    if T > max_tokens:
        raise ValueError("candidate caption with %d tokens: the device scorer handles at most %d" % (T, max_tokens))


def encode_corpus(ids, gts, res, split=str.split):
    """Corpus-local word ids of the device scorers: ids 0..3 stay reserved (0 terminates a hypothesis row of the CIDEr kernel),
    every other word is numbered in order of first appearance over gts[i] + res[i], image by image.  `split` is the scorer's
    own tokenisation (str.split for BLEU and CIDEr, split(" ") for ROUGE-L, where "" is a word).
    -> (word2ix, hyps [image][token id], refs [image][reference][token id])."""
    word2ix = {"<pad>": 0, "<sta>": 1, "<end>": 2, "<unk>": 3}
    get = word2ix.setdefault
    hyps, refs = [], []
    for i in ids:
        refs.append([[get(w, len(word2ix)) for w in split(s)] for s in gts[i]])
        hyps.append([get(w, len(word2ix)) for w in split(res[i][0])])
    return word2ix, hyps, refs


def _split_space(s):
    return s.split(" ")


def _upload_csr(hyps, refs, device):
    """Token lists -> int32 device tensors (hyp_tok, hyp_ptr, ref_tok, ref_ptr, img_ref_ptr) on the current stream, plus the
    host arrays of hypothesis lengths, reference lengths and reference pointers."""
    flat_refs = list(chain.from_iterable(refs))
    hyp_len = np.fromiter(map(len, hyps), np.int64, count=len(hyps))
    ref_len = np.fromiter(map(len, flat_refs), np.int64, count=len(flat_refs))
    img_ref_ptr = np.zeros(len(refs) + 1, np.int64)
    img_ref_ptr[1:] = np.cumsum(np.fromiter(map(len, refs), np.int64, count=len(refs)))
    arrays = []
    for lists, lens in ((hyps, hyp_len), (flat_refs, ref_len)):
        off = np.zeros(len(lens) + 1, np.int64)
        off[1:] = np.cumsum(lens)
        tok = np.fromiter(chain.from_iterable(lists), np.int32, count=int(off[-1]))
        arrays += [np.concatenate([tok, np.zeros(1, np.int32)]), off.astype(np.int32)]     # + 1: never an empty (NULL) buffer
    arrays.append(img_ref_ptr.astype(np.int32))
    dev = [torch.from_numpy(a).to(device, non_blocking=False) for a in arrays]
    return dev, hyp_len, ref_len, img_ref_ptr


def bleu_from_stats(stats, n=4):
    """BleuScorer.compute_score(option='closest') (bleu_scorer.py:201-266) from the integer statistics of icz_bleu_stats:
    stats = rows of (testlen, closest reflen, correct_1..correct_n), one per image.  Plain Python floats in the reference's order.
    -> (corpus scores [n], per-image scores [n][n_img])."""
    small = 1e-9
    tiny = 1e-15
    bleu_list = [[] for _ in range(n)]
    testlen_total, reflen_total = 0, 0
    guess_total, correct_total = [0] * n, [0] * n
    for row in stats:
        testlen, reflen, correct = int(row[0]), int(row[1]), [int(c) for c in row[2:2 + n]]
        guess = [max(0, testlen - k + 1) for k in range(1, n + 1)]
        testlen_total += testlen
        reflen_total += reflen
        for k in range(n):
            guess_total[k] += guess[k]
            correct_total[k] += correct[k]
        bleu = 1.
        for k in range(n):
            bleu *= (float(correct[k]) + tiny) / (float(guess[k]) + small)
            bleu_list[k].append(bleu ** (1. / (k + 1)))
        ratio = (testlen + tiny) / (reflen + small)
        if ratio < 1:
            for k in range(n):
                bleu_list[k][-1] *= math.exp(1 - 1 / ratio)
    bleus = []
    bleu = 1.
    for k in range(n):
        bleu *= float(correct_total[k] + tiny) / (guess_total[k] + small)
        bleus.append(bleu ** (1. / (k + 1)))
    ratio = (testlen_total + tiny) / (reflen_total + small)
    if ratio < 1:
        for k in range(n):
            bleus[k] *= math.exp(1 - 1 / ratio)
    return bleus, bleu_list


def rouge_from_lcs(lcs, hyp_len, ref_len, img_ref_ptr, beta=1.2):
    """Rouge.calc_score / compute_score (rouge.py:38-104) from the LCS lengths of icz_rouge_lcs: lcs [n_ref] and ref_len [n_ref]
    per reference, hyp_len [n_img] per image, img_ref_ptr [n_img + 1] (every image has a reference).  float64 elementwise in the
    reference's order.  -> (np.float64 mean, per-image float64 scores)."""
    lcs = np.asarray(lcs, dtype=np.float64)
    img_ref_ptr = np.asarray(img_ref_ptr, dtype=np.int64)
    hyp_of_ref = np.repeat(np.asarray(hyp_len, dtype=np.float64), np.diff(img_ref_ptr))
    prec = lcs / hyp_of_ref                                            # lcs / float(len(token_c))
    rec = lcs / np.asarray(ref_len, dtype=np.float64)                  # lcs / float(len(token_r))
    prec_max = np.maximum.reduceat(prec, img_ref_ptr[:-1])
    rec_max = np.maximum.reduceat(rec, img_ref_ptr[:-1])
    b2 = beta ** 2
    score = np.zeros(len(prec_max), dtype=np.float64)
    ok = (prec_max != 0) & (rec_max != 0)
    score[ok] = ((1 + b2) * prec_max[ok] * rec_max[ok]) / (rec_max[ok] + b2 * prec_max[ok])
    return np.mean(score), score


class Cider:
    """Cider (cider.py:17-56) on the device.  compute_score(gts, res): both {image id: [tokenised sentence, ...]} with one
    candidate per image and the same key order -> (corpus CIDEr, per-image float64 scores)."""

    MAX_TOKENS = 60          # csrc/ciderd.hip: one wave per hypothesis, at most 60 tokens
    BATCH = 1024

    def __init__(self, n=4, sigma=6.0, device="cuda:0"):
        if n != 4:
            raise ValueError("the device scorer implements the reference default n = 4")
        self._sigma = sigma
        self.device = torch.device(device)

    def method(self):
        return "CIDEr"

    def compute_score(self, gts, res):
        ids = _check_pairs(gts, res)
        word2ix, hyps, _ = encode_corpus(ids, gts, res)
        df = document_frequency({i: gts[i] for i in ids})
        scorer = CiderDReward(df["document_frequency"], df["ref_len"], word2ix, self.device, sigma=self._sigma)
        T = max(1, max(len(h) for h in hyps))
        _check_length(T, self.MAX_TOKENS)
        scores = np.zeros(len(ids), dtype=np.float64)
        for b0 in range(0, len(ids), self.BATCH):
            chunk = ids[b0:b0 + self.BATCH]
            gen = np.zeros((len(chunk), T), dtype=np.int64)
            for j, h in enumerate(hyps[b0:b0 + self.BATCH]):
                gen[j, :len(h)] = h
            gen_t = torch.from_numpy(gen).to(self.device)
            _, sc = scorer.reward(gen_t, torch.zeros_like(gen_t), gts, chunk, return_scores=True)
            scores[b0:b0 + len(chunk)] = sc[:len(chunk)].cpu().numpy()
        scorer.close()
        return float(np.mean(scores)), scores


class Bleu:
    """Bleu (bleu.py:17-47, option 'closest') with the n-gram statistics on the device (csrc/coco_metrics.hip) and the scores on
    the host.  compute_score(gts, res): both {image id: [tokenised sentence, ...]} with one candidate per image and the same key
    order -> (corpus Bleu_1..4, per-image scores [4][n_img]); bit-exact against the reference (tests/golden/coco_metric_cases.json)."""

    MAX_TOKENS = Cider.MAX_TOKENS

    def __init__(self, n=4, device="cuda:0"):
        if n != 4:
            raise ValueError("the device scorer implements the reference default n = 4")
        self._n = n
        self.device = torch.device(device)

    def method(self):
        return "Bleu"

    def statistics(self, gts, res):
        """int32 [n_img, 6] = testlen, closest reflen, correct_1..4 of every image (what cook_test keeps, bleu_scorer.py:63-86)."""
        ids = _check_pairs(gts, res)
        _, hyps, refs = encode_corpus(ids, gts, res)
        _check_length(max((len(h) for h in hyps), default=0), self.MAX_TOKENS)
        if not ids:
            return np.zeros((0, 6), dtype=np.int32)
        with torch.cuda.device(self.device):
            (hyp_tok, hyp_ptr, ref_tok, ref_ptr, img_ref_ptr), _, _, _ = _upload_csr(hyps, refs, self.device)
            stats = torch.empty((len(ids), 6), dtype=torch.int32, device=self.device)
            check(lib().icz_bleu_stats(ptr(hyp_tok), ptr(hyp_ptr), ptr(ref_tok), ptr(ref_ptr), ptr(img_ref_ptr), len(ids), ptr(stats),
                                       stream_ptr()))
            return stats.cpu().numpy()

    def compute_score(self, gts, res):
        return bleu_from_stats(self.statistics(gts, res), self._n)


class Rouge:
    """Rouge (rouge.py:38-104) with the LCS lengths on the device (csrc/coco_metrics.hip) and the F-measure on the host.
    compute_score(gts, res) -> (np.float64 mean ROUGE-L, per-image float64 scores); bit-exact against the reference."""

    MAX_TOKENS = Cider.MAX_TOKENS

    def __init__(self, device="cuda:0"):
        self.beta = 1.2
        self.device = torch.device(device)

    def method(self):
        return "Rouge"

    def lcs(self, gts, res):
        """-> (lcs [n_ref], hypothesis lengths [n_img], reference lengths [n_ref], img_ref_ptr [n_img + 1]), split(" ") tokens."""
        ids = _check_pairs(gts, res)
        _, hyps, refs = encode_corpus(ids, gts, res, _split_space)
        _check_length(max((len(h) for h in hyps), default=0), self.MAX_TOKENS)
        with torch.cuda.device(self.device):
            (hyp_tok, hyp_ptr, ref_tok, ref_ptr, img_ref_ptr), hyp_len, ref_len, img_ref_ptr_host = _upload_csr(hyps, refs, self.device)
            out = torch.empty(max(len(ref_len), 1), dtype=torch.int32, device=self.device)
            check(lib().icz_rouge_lcs(ptr(hyp_tok), ptr(hyp_ptr), ptr(ref_tok), ptr(ref_ptr), ptr(img_ref_ptr), len(ids), ptr(out),
                                      stream_ptr()))
            return out.cpu().numpy()[:len(ref_len)], hyp_len, ref_len, img_ref_ptr_host

    def compute_score(self, gts, res):
        return rouge_from_lcs(*self.lcs(gts, res), beta=self.beta)


def coco_eval(results, eval_caption_path, device="cuda:0"):
    """coco_eval (COCO_Eval_Utils.py:15-35) restricted to the metric Engine.training keeps (CIDEr, Engine.py:117-131):
    results = [{'image_id', 'caption'}, ...] as produced by eval_captions_json_generation."""
    anns = load_annotations(eval_caption_path)
    res = {}
    for r in results:
        res.setdefault(r["image_id"], []).append({"caption": r["caption"]})
    img_ids = list(res.keys())
    gts = tokenize({i: anns[i] for i in img_ids})
    res = tokenize({i: res[i][:1] for i in img_ids})
    score, _ = Cider(device=device).compute_score(gts, res)
    print("---------------Evaluation performance-----------------")
    print("%s: %.3f" % ("CIDEr", score))
    return score


def evaluate_captions(results, eval_caption_path, device="cuda:0"):
    """COCOEvalCap.evaluate (eval.py:24-69) without the Java scorers: Bleu_1..4, ROUGE_L and CIDEr of results = [{'image_id',
    'caption'}, ...] against the annotation file, in the reference's order and with its "%s: %0.3f" lines.
    -> (eval {metric: corpus score}, img_to_eval {image id: {"image_id", metric: score}}), the shapes of COCOEvalCap.eval and
    COCOEvalCap.imgToEval.  METEOR and SPICE are not computed (they need Java)."""
    anns = load_annotations(eval_caption_path)
    res = {}
    for r in results:
        res.setdefault(r["image_id"], []).append({"caption": r["caption"]})
    img_ids = list(res.keys())
    gts = tokenize({i: anns[i] for i in img_ids})
    res = tokenize({i: res[i][:1] for i in img_ids})
    ev, img_to_eval = {}, {i: {"image_id": i} for i in img_ids}
    scorers = [(Bleu(4, device=device), ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4"]), (Rouge(device=device), "ROUGE_L"),
               (Cider(device=device), "CIDEr")]
    for scorer, method in scorers:
        print("computing %s score..." % scorer.method())
        score, scores = scorer.compute_score(gts, res)
        pairs = zip(score, scores, method) if type(method) == list else [(score, scores, method)]
        for sc, scs, m in pairs:
            ev[m] = sc
            for i, v in zip(img_ids, scs):
                img_to_eval[i][m] = v
            print("%s: %0.3f" % (m, sc))
    return ev, img_to_eval
