"""CPU-only checks of the multi-sample SCST entries (no GPU): argument errors reported through icz_last_error before any device
work, and the host restatement of the leave-one-out reward against a brute-force loop."""
import ctypes

import numpy as np
import pytest


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def test_sample_n_rejects_bad_k_and_null_handle():
    L = _lib()
    for K in (1, 9):
        assert L.icz_butd_sample_n(None, None, 4, K, 20, None, None, None, None) == -1
        assert b"K=%d" % K in L.icz_last_error()
    assert L.icz_butd_sample_n(None, None, 4, 5, 20, None, None, None, None) == -1
    assert b"null handle" in L.icz_last_error()


def test_reward_loo_rejects_bad_k_and_null_handle():
    L = _lib()
    args = [None] * 10
    for K in (1, 9):
        assert L.icz_ciderd_reward_loo(None, None, 4, K, 20, *args, None) == -1
        assert b"K=%d" % K in L.icz_last_error()
    assert L.icz_ciderd_reward_loo(None, None, 4, 3, 20, *args, None) == -1
    assert b"null handle" in L.icz_last_error()
    # a live scorer handle (host-side construction only: it keeps the table pointers, touches no device memory)
    keys = (ctypes.c_int32 * 8)(*([-1] * 8))
    idf = (ctypes.c_double * 2)()
    pen = (ctypes.c_double * 64)()
    h = ctypes.c_void_p()
    assert L.icz_ciderd_create(keys, idf, 2, 0.0, pen, ctypes.byref(h)) == 0
    try:
        assert L.icz_ciderd_reward_loo(h, None, 4, 0, 20, *args, None) == -1
        assert b"K=0" in L.icz_last_error()
        assert L.icz_ciderd_reward_loo(h, None, 4, 4, 20, *args, None) == -1
        assert b"null argument" in L.icz_last_error()
    finally:
        L.icz_ciderd_destroy(h)


@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_loo_helper_matches_brute_force(K):
    from simpleimagecaptionzoo_amd.ciderd import loo_baseline_reward
    rs = np.random.RandomState(K)
    B = 7
    s = rs.rand(B * K) * 3.0
    s[:K] = 0.25                      # one image whose captions all score the same: reward 0
    got = loo_baseline_reward(s, K)
    for img in range(B):
        for k in range(K):
            i = img * K + k
            others = [float(s[img * K + j]) for j in range(K) if j != k]
            base = 0.0
            for x in others:
                base += x
            assert got[i] == np.float32(float(s[i]) - base / (K - 1))
    assert (got[:K] == 0).all()
