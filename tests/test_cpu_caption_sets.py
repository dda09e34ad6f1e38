"""CPU-only checks of the caption-set feature (no GPU): the argument errors of the four C entries, reported before any device work,
the packing errors, the host-side metrics on hand-computed cases, and the ValueErrors of the Engine methods."""
import ctypes

import numpy as np
import pytest


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _handle(L):
    """a live scorer handle (host-side construction only: it keeps the table pointers, touches no device memory)"""
    keep = ((ctypes.c_int32 * 8)(*([-1] * 8)), (ctypes.c_double * 2)(), (ctypes.c_double * 64)())
    h = ctypes.c_void_p()
    assert L.icz_ciderd_create(keep[0], keep[1], 2, 0.0, keep[2], ctypes.byref(h)) == 0
    return h, keep


def test_pairwise_argument_errors():
    L = _lib()
    h, keep = _handle(L)
    buf = (ctypes.c_int32 * 16)()
    try:
        for K in (1, 9):
            assert L.icz_ciderd_pairwise(None, None, None, 4, K, None, None, None, None, 0, None) == -1
            assert b"K=%d" % K in L.icz_last_error()
        for n in (0, -3):
            assert L.icz_ciderd_pairwise(None, None, None, n, 5, None, None, None, None, 0, None) == -1
            assert b"n_img=%d" % n in L.icz_last_error()
        assert L.icz_ciderd_pairwise(None, None, None, 4, 5, None, None, None, None, 0, None) == -1
        assert b"null argument" in L.icz_last_error()
        assert L.icz_ciderd_pairwise(None, buf, buf, 4, 5, buf, None, None, buf, 0, None) == -1
        assert b"null handle" in L.icz_last_error()
        assert L.icz_ciderd_pairwise(h, buf, buf, 4, 5, buf, None, None, buf, 64, None) == -1        # a workspace that is too small
        assert b"workspace" in L.icz_last_error()
        assert L.icz_ciderd_pairwise_workspace_bytes(4, 5) >= 20 * 240 * 28
        assert L.icz_ciderd_pairwise_workspace_bytes(4, 1) == 0 and L.icz_ciderd_pairwise_workspace_bytes(0, 5) == 0
    finally:
        L.icz_ciderd_destroy(h)


def test_scores_csr_argument_errors():
    L = _lib()
    buf = (ctypes.c_int32 * 16)()
    store = [None] * 8
    for K in (0, 9):
        assert L.icz_ciderd_scores_csr(None, None, None, 4, K, *store, None, None) == -1
        assert b"K=%d" % K in L.icz_last_error()
    assert L.icz_ciderd_scores_csr(None, None, None, 0, 1, *store, None, None) == -1
    assert b"n_img=0" in L.icz_last_error()
    assert L.icz_ciderd_scores_csr(None, buf, buf, 4, 1, *store, buf, None) == -1
    assert b"null argument" in L.icz_last_error()
    assert L.icz_ciderd_scores_csr(None, buf, buf, 4, 1, *([buf] * 8), buf, None) == -1
    assert b"null handle" in L.icz_last_error()


def test_cook_device_and_diversity_argument_errors():
    L = _lib()
    buf = (ctypes.c_int32 * 16)()
    out = [None] * 6
    assert L.icz_ciderd_cook_device(None, None, None, 0, *out, None) == -1
    assert b"n_cand=0" in L.icz_last_error()
    assert L.icz_ciderd_cook_device(None, buf, buf, 3, *out, None) == -1
    assert b"null argument" in L.icz_last_error()
    assert L.icz_ciderd_cook_device(None, buf, buf, 3, *([buf] * 6), None) == -1
    assert b"null handle" in L.icz_last_error()
    for K in (0, 9):
        assert L.icz_ngram_diversity(None, None, 4, K, None, None) == -1
        assert b"K=%d" % K in L.icz_last_error()
    assert L.icz_ngram_diversity(None, None, 0, 3, None, None) == -1
    assert b"n_img=0" in L.icz_last_error()
    assert L.icz_ngram_diversity(buf, buf, 4, 3, None, None) == -1
    assert b"null argument" in L.icz_last_error()


def test_pack_candidates_errors():
    from simpleimagecaptionzoo_amd.caption_sets import pack_candidates
    w2i = {"a": 4, "b": 5}
    with pytest.raises(ValueError, match="not in the vocabulary"):
        pack_candidates([["a b", "a c"]], w2i, "cpu")
    with pytest.raises(ValueError, match="61 words"):
        pack_candidates([[" ".join(["a"] * 61)]], w2i, "cpu")
    with pytest.raises(ValueError, match="image 1 has 1 captions"):
        pack_candidates([["a", "b"], ["a"]], w2i, "cpu")
    with pytest.raises(ValueError, match="outside 1..8"):
        pack_candidates([["a"] * 9], w2i, "cpu")
    with pytest.raises(ValueError, match="no images"):
        pack_candidates([], w2i, "cpu")
    c = pack_candidates([["a  b a", ""], [" ".join(["b"] * 60), "b"]], w2i, "cpu")          # blanks split, empty and 60 words are legal
    assert (c.n_img, c.K) == (2, 2)
    assert c.ptr_host.tolist() == [0, 3, 3, 63, 64] and c.tok_host[:3].tolist() == [4, 5, 4] and c.tok.dtype.is_floating_point is False


def test_div_n_and_mean_pairwise_by_hand():
    from simpleimagecaptionzoo_amd.caption_sets import div_n, mean_pairwise
    # image 0: "a b a" + "a b": words 5, distinct 1-grams 2, distinct 2-grams {ab, ba} = 2; image 1: all candidates empty
    counts = np.zeros((2, 4, 2), np.int32)
    counts[0] = [[2, 5], [2, 3], [1, 1], [0, 0]]
    assert div_n(counts, 1) == (2 / 5 + 0.0) / 2 and div_n(counts, 2) == (2 / 5 + 0.0) / 2
    assert div_n(counts[:1], 3) == 1 / 5
    with pytest.raises(ValueError):
        div_n(counts, 5)
    pair = np.array([[[9.0, 1.0], [3.0, 9.0]], [[9.0, 0.0], [4.0, 9.0]]])
    assert mean_pairwise(pair) == ((1.0 + 3.0) / 2 + (0.0 + 4.0) / 2) / 2
    with pytest.raises(ValueError):
        mean_pairwise(np.zeros((2, 1, 1)))


def test_consensus_host_by_hand_and_against_the_oracle():
    from oracle import ciderd as oc
    from simpleimagecaptionzoo_amd.caption_sets import consensus_host
    from simpleimagecaptionzoo_amd.ciderd import ReferenceCooker
    w2i = {"<pad>": 0, "<sta>": 1, "<end>": 2, "<unk>": 3, "a": 4, "b": 5, "c": 6}
    df = {("a",): 1.0, ("b",): 2.0, ("a", "b"): 1.0}
    ck = ReferenceCooker(df, 4, w2i)
    caps = [["a", "a", "b"], ["a a a b", "a b", ""]]
    pair, cons, best = consensus_host(ck, caps)
    # one-word candidates: only the unigram order can match: 1 (cosine) / 4 orders * 10 = 2.5 with itself and its copy, 0 with "b"
    assert pair[0].tolist() == [[2.5, 2.5, 0.0], [2.5, 2.5, 0.0], [0.0, 0.0, 2.5]]
    assert cons[0].tolist() == [1.25, 1.25, 0.0] and best.tolist()[0] == 0              # (2.5 + 0) / 2; the tie goes to the first
    assert pair[1, 0, 1] != pair[1, 1, 0]                                              # clipping: tf 3 against tf 1
    assert (pair[1, 2] == 0).all() and (pair[1, :, 2] == 0).all()                      # the empty candidate matches nothing
    docfreq = oc.DocFreq(df, 4)
    for i, g in enumerate(caps):
        for a in range(3):
            for b in range(3):
                assert pair[i, a, b] == oc.ciderd_scores([g[a]], [[g[b]]], docfreq)[0]
            assert cons[i, a] == oc.ciderd_scores([g[a]], [[g[b] for b in range(3) if b != a]], docfreq)[0]


def test_engine_methods_reject_bad_arguments():
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, BUTDDetection_Eng, NIC_Eng
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    good = [{"image_id": i // 2, "caption": "w1 w2", "score": -1.0} for i in range(4)]
    for cls in (BUTDDetection_Eng, AoADetection_Eng, NIC_Eng):
        eng = cls.__new__(cls)
        eng.caption_vocab = synthetic_vocab(20)
        eng._cider_df, eng._scorer = None, None
        for K in (1, 9, True, 2.0, "2"):
            with pytest.raises(ValueError, match="samples_per_image"):
                eng.rerank_captions_json(good, K)
            with pytest.raises(ValueError, match="samples_per_image"):
                eng.caption_set_report(good, K, {0: ["w1"], 1: ["w1"]})
            with pytest.raises(ValueError, match="samples_per_image"):
                eng.consensus_captions_json_generation([], K)
        with pytest.raises(ValueError, match="multiple"):
            eng.rerank_captions_json(good[:3], 2)
        with pytest.raises(ValueError, match="multiple"):
            eng.rerank_captions_json([], 2)
        with pytest.raises(ValueError, match="one image"):
            eng.rerank_captions_json(good[1:3], 2)
        with pytest.raises(ValueError, match="caption"):
            eng.rerank_captions_json([{"image_id": 0}, {"image_id": 0}], 2)
        with pytest.raises(ValueError, match="vocabulary"):
            eng.rerank_captions_json([{"image_id": 0, "caption": "w1 zebra"}, {"image_id": 0, "caption": ""}], 2)
        with pytest.raises(ValueError, match="61 words"):
            eng.rerank_captions_json([{"image_id": 0, "caption": " ".join(["w1"] * 61)}, {"image_id": 0, "caption": ""}], 2)
        with pytest.raises(ValueError, match="cider_df"):
            eng.rerank_captions_json(good, 2)
        with pytest.raises(ValueError, match="cider_df"):
            eng.consensus_captions_json_generation([], 2)
        eng._cider_df = {"document_frequency": {}, "ref_len": 1}
        with pytest.raises(ValueError, match="no references"):
            eng.caption_set_report(good, 2, {0: ["w1"]})
        with pytest.raises(ValueError, match="temperature"):
            eng.consensus_captions_json_generation([], 2, temperature=0.0)
