"""BLEU / ROUGE-L of the evaluation report without a device: the host halves of coco_eval.Bleu / coco_eval.Rouge against the
reference scorers' own values (tests/golden/coco_metric_cases.json, tests/golden/make_metric_goldens.py), the corpus-local
token encoding, and the argument checks of icz_bleu_stats / icz_rouge_lcs."""
import ctypes
import json
import os

import numpy as np
import pytest

from simpleimagecaptionzoo_amd.coco_eval import (Bleu, Rouge, bleu_from_stats, encode_corpus, rouge_from_lcs)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_metric_cases.json")


def cases():
    return json.load(open(GOLDEN))


def hexes(xs):
    return [float(x).hex() for x in xs]


@pytest.mark.parametrize("name", ["synthetic", "edge", "single", "abstract80"])
def test_bleu_host_formula_bit_exact_from_golden_statistics(name):
    c = cases()[name]
    stats = [[s["testlen"], s["reflen"]] + s["correct"] for s in c["bleu_stats"]]
    for s in c["bleu_stats"]:      # guess is derived on the host from testlen (cook_test, bleu_scorer.py:78)
        assert s["guess"] == [max(0, s["testlen"] - k + 1) for k in range(1, 5)]
    score, scores = bleu_from_stats(np.asarray(stats, dtype=np.int32))
    assert len(score) == 4 and len(scores) == 4 and all(len(x) == len(c["ids"]) for x in scores)
    assert hexes(score) == c["bleu"], name
    assert [hexes(x) for x in scores] == c["bleu_scores"], name


@pytest.mark.parametrize("name", ["synthetic", "edge", "single", "abstract80"])
def test_rouge_host_formula_bit_exact_from_golden_lcs(name):
    c = cases()[name]
    ids = c["ids"]
    hyp_len = [len(c["res"][k][0].split(" ")) for k in ids]
    ref_len = [len(r.split(" ")) for k in ids for r in c["gts"][k]]
    img_ref_ptr = np.cumsum([0] + [len(c["gts"][k]) for k in ids])
    lcs = [x for row in c["lcs"] for x in row]
    mean, scores = rouge_from_lcs(lcs, hyp_len, ref_len, img_ref_ptr)
    assert isinstance(mean, np.float64) and scores.dtype == np.float64
    assert float(mean).hex() == c["rouge"], name
    assert hexes(scores) == c["rouge_scores"], name


def test_token_encoding_split_versus_split_space():
    """BLEU / CIDEr split with str.split(), ROUGE-L with split(" "): "" is a one-word sentence and double spaces make empty
    words there.  Ids 0..3 stay reserved; words are numbered in order of first appearance, references before the hypothesis."""
    gts = {"a": [" a  b", ""], "b": ["c a"]}
    res = {"a": ["b  c "], "b": [""]}
    w2i, hyps, refs = encode_corpus(["a", "b"], gts, res)
    assert w2i == {"<pad>": 0, "<sta>": 1, "<end>": 2, "<unk>": 3, "a": 4, "b": 5, "c": 6}
    assert refs == [[[4, 5], []], [[6, 4]]] and hyps == [[5, 6], []]
    w2i, hyps, refs = encode_corpus(["a", "b"], gts, res, lambda s: s.split(" "))
    assert w2i == {"<pad>": 0, "<sta>": 1, "<end>": 2, "<unk>": 3, "": 4, "a": 5, "b": 6, "c": 7}
    assert refs == [[[4, 5, 4, 6], [4]], [[7, 5]]] and hyps == [[6, 4, 7, 4], [4]]


def test_golden_edge_strings_and_closest_tie():
    """The edge case's statistics pin the two tokenisations and the "closest" tie rule (bleu_scorer.py:73-74: min over
    (|l - testlen|, l), so refs of testlen - 2 and testlen + 2 give the shorter); the other choice gives another Bleu."""
    c = cases()["edge"]
    st = dict(zip(c["ids"], c["bleu_stats"]))
    lcs = dict(zip(c["ids"], c["lcs"]))
    assert st["e0"]["testlen"] == 0 and st["e2"]["testlen"] == 2                 # "" and "a  b" under split()
    assert [len(r.split(" ")) for r in c["gts"]["e2"]] == [4, 3, 3]              # ... and under split(" ")
    assert lcs["e4"] == [1] and lcs["e2"] == [3, 2, 2]                          # [""] vs [""]; the empty word of "a  b" counts
    assert st["e3"]["testlen"] == 4 and st["e3"]["reflen"] == 2                 # refs of 6 and 2 tokens: the tie goes to 2
    rows = [[s["testlen"], s["reflen"]] + s["correct"] for s in c["bleu_stats"]]
    assert hexes(bleu_from_stats(rows)[0]) == c["bleu"]
    rows[c["ids"].index("e3")][1] = 6
    assert hexes(bleu_from_stats(rows)[0]) != c["bleu"]


def test_argument_checks_before_the_device():
    """icz_bleu_stats / icz_rouge_lcs reject null pointers and n_img < 0 with status -1 and a message, without a GPU; the
    Python scorers reject an over-long candidate and mismatched keys before any upload."""
    from simpleimagecaptionzoo_amd._lib import lib
    L = lib()
    buf = (ctypes.c_int32 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn, name in ((L.icz_bleu_stats, b"icz_bleu_stats"), (L.icz_rouge_lcs, b"icz_rouge_lcs")):
        assert fn(None, p, p, p, p, 1, p, None) == -1
        assert name in L.icz_last_error() and b"null" in L.icz_last_error()
        assert fn(p, p, p, p, p, 1, None, None) == -1
        assert fn(p, p, p, p, p, -1, p, None) == -1
        assert b"n_img=-1" in L.icz_last_error()
    long_hyp = {"x": [" ".join(["w"] * 61)]}
    for scorer in (Bleu(), Rouge()):
        with pytest.raises(ValueError, match="61 tokens"):
            scorer.compute_score({"x": ["w"]}, long_hyp)
        with pytest.raises(AssertionError):
            scorer.compute_score({"x": ["a"], "y": ["b"]}, {"y": ["b"], "x": ["a"]})
    with pytest.raises(ValueError):
        Bleu(n=3)
    assert Bleu().method() == "Bleu" and Rouge().method() == "Rouge"
