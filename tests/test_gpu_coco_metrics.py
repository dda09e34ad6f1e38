"""BLEU / ROUGE-L of the evaluation report on the device (csrc/coco_metrics.hip): integer statistics and LCS lengths against the
reference's own (tests/golden/coco_metric_cases.json), scores bit-exact, evaluate_captions end to end, and a 5 000-image corpus
against an independent pure-Python count."""
import json
import os
import random
import time
from collections import Counter

import numpy as np
import pytest
import torch

from simpleimagecaptionzoo_amd.coco_eval import Bleu, Rouge

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_metric_cases.json")


def hexes(xs):
    return [float(x).hex() for x in xs]


def load(c):
    return {k: c["gts"][k] for k in c["ids"]}, {k: c["res"][k] for k in c["ids"]}


@pytest.mark.parametrize("name", ["synthetic", "edge", "single", "abstract80"])
def test_device_statistics_and_scores_match_reference(name):
    c = json.load(open(GOLDEN))[name]
    gts, res = load(c)
    stats = Bleu().statistics(gts, res)
    want = [[s["testlen"], s["reflen"]] + s["correct"] for s in c["bleu_stats"]]
    assert stats.tolist() == want, name
    lcs, _, _, ptr = Rouge().lcs(gts, res)
    assert [lcs[ptr[i]:ptr[i + 1]].tolist() for i in range(len(c["ids"]))] == c["lcs"], name
    score, scores = Bleu().compute_score(gts, res)
    assert hexes(score) == c["bleu"] and [hexes(s) for s in scores] == c["bleu_scores"], name
    mean, per = Rouge().compute_score(gts, res)
    assert isinstance(mean, np.float64) and float(mean).hex() == c["rouge"] and hexes(per) == c["rouge_scores"], name


def test_evaluate_captions_end_to_end(tmp_path, capsys):
    from simpleimagecaptionzoo_amd.coco_eval import coco_eval, evaluate_captions, load_annotations, tokenize
    caps = {11: ["A man rides a horse.", "A person on a horse, outside.", "Man riding a brown horse"],
            12: ["Two dogs play in the snow!", "Dogs playing; it's snowing.", "a couple of dogs in snow"],
            13: ["A plate of food.", "Food on a white plate", "some food"]}
    anns = {"annotations": [{"image_id": i, "caption": c} for i, cs in caps.items() for c in cs]}
    p = tmp_path / "captions_val.json"
    p.write_text(json.dumps(anns))
    results = [{"image_id": 12, "caption": "two dogs in the snow"}, {"image_id": 11, "caption": "a man riding a horse"},
               {"image_id": 13, "caption": "a plate"}]
    ev, img_to_eval = evaluate_captions(results, str(p))
    out = capsys.readouterr().out
    gts = tokenize(load_annotations(str(p)))
    ids = [12, 11, 13]
    g = {i: gts[i] for i in ids}
    r = {i: [x["caption"] for x in results if x["image_id"] == i] for i in ids}
    bleu, bleus = Bleu().compute_score(g, r)
    rouge, rouges = Rouge().compute_score(g, r)
    assert [ev["Bleu_%d" % (k + 1)] for k in range(4)] == bleu and ev["ROUGE_L"] == rouge
    assert ev["CIDEr"] == coco_eval(results, str(p))
    assert sorted(ev) == sorted(["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"])
    assert list(img_to_eval) == ids
    for j, i in enumerate(ids):
        assert img_to_eval[i]["image_id"] == i
        assert [img_to_eval[i]["Bleu_%d" % (k + 1)] for k in range(4)] == [bleus[k][j] for k in range(4)]
        assert img_to_eval[i]["ROUGE_L"] == rouges[j] and "CIDEr" in img_to_eval[i]
    for m in ("Bleu_1", "Bleu_4", "ROUGE_L", "CIDEr"):
        assert "%s: %0.3f" % (m, ev[m]) in out


def _corpus(n_img, n_ref, seed):
    rng = random.Random(seed)
    words = ["w%d" % i for i in range(300)]
    weights = [1.0 / (i + 1) for i in range(300)]

    def sent(L):
        return " ".join(rng.choices(words, weights, k=L))
    gts = {i: [sent(rng.randint(8, 12)) for _ in range(n_ref)] for i in range(n_img)}
    res = {i: [sent(rng.randint(0, 60))] for i in range(n_img)}
    return gts, res


def _clipped_counts(hyp, refs):
    """Independent count: per order k, sum over distinct hypothesis n-grams of min(count, max count in one reference)."""
    out = []
    for k in range(1, 5):
        h = Counter(tuple(hyp[i:i + k]) for i in range(len(hyp) - k + 1))
        rc = [Counter(tuple(r[i:i + k]) for i in range(len(r) - k + 1)) for r in refs]
        out.append(sum(min(c, max(x[g] for x in rc)) for g, c in h.items()))
    return out


def _lcs_dp(a, b):
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[-1]


def test_scale_5000_images_against_python_count():
    gts, res = _corpus(5000, 5, seed=3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = Bleu().statistics(gts, res)
    lcs, _, _, ptr = Rouge().lcs(gts, res)
    print("device statistics of 5000 images x 5 refs: %.1f ms" % (1e3 * (time.perf_counter() - t0)))
    for i in range(5000):
        hyp, refs = res[i][0].split(), [r.split() for r in gts[i]]
        closest = min((abs(len(r) - len(hyp)), len(r)) for r in refs)[1]
        assert stats[i].tolist() == [len(hyp), closest] + _clipped_counts(hyp, refs), i
        h = res[i][0].split(" ")
        assert lcs[ptr[i]:ptr[i + 1]].tolist() == [_lcs_dp(r.split(" "), h) for r in gts[i]], i


def test_side_stream_gives_the_same_scores():
    c = json.load(open(GOLDEN))["synthetic"]
    gts, res = load(c)
    base = (Bleu().compute_score(gts, res), Rouge().compute_score(gts, res))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        side = (Bleu().compute_score(gts, res), Rouge().compute_score(gts, res))
    assert base[0] == side[0]
    assert base[1][0] == side[1][0] and np.array_equal(base[1][1], side[1][1])


def test_long_candidate_and_key_order_rejected():
    with pytest.raises(ValueError, match="61 tokens"):
        Bleu().compute_score({1: ["a b"]}, {1: [" ".join(["a"] * 61)]})
    with pytest.raises(ValueError, match="61 tokens"):
        Rouge().compute_score({1: ["a b"]}, {1: [" ".join(["a"] * 61)]})
    Bleu().compute_score({1: ["a b"]}, {1: [" ".join(["a"] * 60)]})          # 60 is the bound itself
    for scorer in (Bleu(), Rouge()):
        with pytest.raises(AssertionError):
            scorer.compute_score({1: ["a"], 2: ["b"]}, {2: ["b"], 1: ["a"]})
