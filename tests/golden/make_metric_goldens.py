#!/usr/bin/env python3
"""Golden vectors of the evaluation report's BLEU and ROUGE-L (runs ONLY in the build container, CPU).

Imports the reference's pure-Python scorers from /root/reference *unmodified* -- Bleu / BleuScorer
(coco_caption/pycocoevalcap/bleu/bleu.py, bleu_scorer.py) and Rouge / my_lcs (rouge/rouge.py) -- drives them on seeded
synthetic corpora, hand-made edge cases and the abstract48S sentences, and writes coco_metric_cases.json next to this script.
Per case: the inputs (ids, gts, res), the reference's corpus and per-image Bleu_1..4 and ROUGE-L as float.hex strings, the
integer statistics the device computes (testlen, closest reflen, guess, correct per image) and my_lcs of every
(image, reference) pair.  Data only; no reference source travels with the fixture.

Usage:  python tests/golden/make_metric_goldens.py
"""
import contextlib
import io
import json
import os
import sys
from collections import defaultdict

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
TAG = "coco_metric_cases"


def zipf_sentence(rng, words, L):
    z = np.minimum(rng.zipf(1.3, size=L), len(words)) - 1
    return " ".join(words[j] for j in z)


def synthetic_case(seed=11, n_img=200):
    """Zipf corpus: 1-7 references of 8-12 tokens (one of 80), hypotheses of every length 0..60, repeated n-grams (clipping),
    a hypothesis longer than all its references (no brevity factor) and one that copies a reference."""
    rng = np.random.RandomState(seed)
    words = ["w%d" % i for i in range(60)]
    gts, res = {}, {}
    for i in range(n_img):
        gts[str(i)] = [zipf_sentence(rng, words, rng.randint(8, 13)) for _ in range(rng.randint(1, 8))]
        res[str(i)] = [zipf_sentence(rng, words, i % 61)]
    gts["7"].append(zipf_sentence(rng, words, 80))                       # a reference longer than any hypothesis
    res["8"] = ["w1 w2 w1 w2 w1 w2 w1 w2 w0 w0 w0"]                       # repeated n-grams: counts clipped by the references
    gts["8"] = ["w1 w2 w0 w3 w1 w2", "w0 w0 w1 w5"]
    res["9"] = [" ".join(["w0 w1 w2 w3"] * 6)]                            # 24 tokens against references of at most 12
    res["10"] = [gts["10"][0]]                                            # exact copy of a reference
    res["11"] = [zipf_sentence(rng, words, 60)]
    return gts, res


def edge_case():
    """Tokenisation edges (split() vs split(" ")), empty strings, and the closest-length tie rule."""
    gts = {
        "e0": ["a man rides a horse", "a person on a horse"],
        "e1": ["", "two dogs"],                                           # empty reference
        "e2": ["a  b c", " a b", "a b "],                                 # double / leading / trailing spaces
        "e3": ["x y z w v u", "x y"],                                     # testlen 4: refs of 2 and 6 tie -> 2
        "e4": [""],
        "e5": ["the cat sat on the mat", "a cat on a mat"],
        "e6": ["p q r s t", "p q r s t u v w"],
    }
    res = {
        "e0": [""],                                                       # empty hypothesis
        "e1": ["two dogs"],
        "e2": ["a  b"],
        "e3": ["x y z w"],
        "e4": [""],                                                       # ROUGE-L 1.0: [""] against [""]
        "e5": [" the cat the cat"],                                       # leading space
        "e6": ["p q r s t u"],                                            # testlen 6: refs of 5 and 8 -> 5
    }
    return gts, res


def single_case():
    return {"s0": ["w1 w2 w3 w4", "w2 w3 w4 w5 w6"]}, {"s0": ["w1 w2 w3 w4 w5"]}


def abstract_case(n=80):
    """The first 80 abstract48S images with a candidate (abstract_candsB), lower-cased -- as the corpus-CIDEr golden."""
    refs = json.load(open(os.path.join(REF, "cider/data/abstract48S.json")))
    cands = json.load(open(os.path.join(REF, "cider/data/abstract_candsB.json")))
    g = defaultdict(list)
    for r in refs:
        g[r["image_id"]].append(r["caption"].lower())
    res = {}
    for c in cands:
        if c["image_id"] in g and c["image_id"] not in res and len(res) < n:
            res[c["image_id"]] = [c["caption"].lower()]
    return {k: g[k][:5] for k in res}, res


def main():
    sys.path.insert(0, REF)
    from coco_caption.pycocoevalcap.bleu.bleu import Bleu
    from coco_caption.pycocoevalcap.bleu.bleu_scorer import BleuScorer
    from coco_caption.pycocoevalcap.rouge.rouge import Rouge, my_lcs
    cases = {"synthetic": synthetic_case(), "edge": edge_case(), "single": single_case(), "abstract80": abstract_case()}
    fx = {}
    for name, (gts, res) in cases.items():
        ids = list(gts.keys())
        res = {k: res[k] for k in ids}
        with contextlib.redirect_stdout(io.StringIO()):                  # compute_score(verbose=1) prints its totals
            bleu, bleus = Bleu(4).compute_score(gts, res)
        rouge, rouges = Rouge().compute_score(gts, res)
        # the integer statistics of the same cooking (bleu.py:33-42 -> cook_refs / cook_test)
        bs = BleuScorer(n=4)
        for k in ids:
            bs += (res[k][0], gts[k])
        stats = []
        for comps in bs.ctest:
            t = comps["testlen"]
            stats.append({"testlen": t, "reflen": bs._single_reflen(comps["reflen"], "closest", t), "guess": comps["guess"],
                          "correct": comps["correct"]})
        lcs = [[my_lcs(r.split(" "), res[k][0].split(" ")) for r in gts[k]] for k in ids]
        fx[name] = {"ids": ids, "gts": gts, "res": res,
                    "bleu": [float(x).hex() for x in bleu], "bleu_scores": [[float(x).hex() for x in b] for b in bleus],
                    "rouge": float(rouge).hex(), "rouge_scores": [float(x).hex() for x in rouges],
                    "bleu_stats": stats, "lcs": lcs}
        print(name, "%d images: Bleu_4 %.4f ROUGE_L %.4f" % (len(ids), bleu[3], rouge))
    path = os.path.join(OUT, TAG + ".json")
    with open(path, "w") as f:
        json.dump(fx, f)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
