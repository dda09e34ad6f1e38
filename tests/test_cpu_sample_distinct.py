"""CPU tests of stochastic beam search (include/icz.h: icz_*_sample_distinct): the argument errors in their documented order, the
Python ValueErrors, the host oracle of tests/_sbs_oracle.py against exact enumeration and its own properties, and the input
condition of the GPU tests -- every kernel-alone case and the whole-decode configs are separated by more than GAP_MIN."""
import ctypes as C

import numpy as np
import pytest

import _philox
import _sbs_oracle as so


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _err(status, needle):
    assert status == -1, status
    assert needle.encode() in _lib().icz_last_error(), _lib().icz_last_error()


def test_symbols_and_python_surface():
    from simpleimagecaptionzoo_amd import stochastic_beam as sb
    from simpleimagecaptionzoo_amd.aoa import AoaHandle
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd import engine
    from simpleimagecaptionzoo_amd.nic import NicHandle
    L = _lib()
    for name in ("icz_sample_distinct_check", "icz_butd_sample_distinct", "icz_aoa_sample_distinct", "icz_nic_sample_distinct",
                 "icz_ensemble_sample_distinct", "icz_test_sbs_rowtopk", "icz_test_sbs_step", "icz_test_sbs_init", "icz_test_sbs_finalize"):
        assert getattr(L, name).argtypes is not None, name
    for cls in (ButdHandle, AoaHandle, NicHandle):
        assert cls._entries().sample_distinct.__name__ == "icz_%s_sample_distinct" % cls.family
        assert not hasattr(cls, "sample_distinct")            # a function of stochastic_beam, not a method: the surface is pinned
    assert callable(sb.sample_distinct) and callable(sb.captioner_sample_distinct)
    for m in ("sample_distinct_captions_json_generation", "consensus_distinct_captions_json_generation"):
        assert callable(getattr(engine.BUTDDetection_Eng, m))      # beside sample_captions_json_generation: AoA and NIC inherit them
    assert callable(engine.sample_distinct_ensemble_captions_json_generation)


def test_argument_errors_in_documented_order():
    L = _lib()
    chk = L.icz_sample_distinct_check
    assert chk(4, 5, 20, 1.0, 100, 64) == 0
    assert chk(4, 8, 256, 0.5, 8, 32) == 0
    # rule 1 wins over every later one
    _err(chk(0, 0, 0, float("nan"), 100, 0), "outside 1..8")
    _err(chk(4, 9, 20, 1.0, 100, 64), "outside 1..8")
    _err(chk(4, 5, 20, 1.0, 4, 64), "above the vocabulary")
    # rule 2
    for t in (0.0, -1.0, float("inf"), float("nan")):
        _err(chk(0, 5, 0, t, 100, 0), "temperature")
    # rule 3
    _err(chk(0, 5, 0, 1.0, 100, 0), "max_len")
    _err(chk(4, 5, 257, 1.0, 100, 64), "max_len")
    # rule 6
    _err(chk(0, 5, 20, 1.0, 100, 64), "row capacity")
    _err(chk(13, 5, 20, 1.0, 100, 64), "row capacity")


@pytest.mark.parametrize("family", ["butd", "aoa", "nic", "ensemble"])
def test_entries_with_null_handles(family):
    from simpleimagecaptionzoo_amd._lib import SampleDistinctOut
    L = _lib()
    entry = getattr(L, "icz_%s_sample_distinct" % family)
    one = C.c_void_p(16)          # a non-null address the entry must never dereference: every call below is refused before
    out = SampleDistinctOut(16, 16, 16, 16, 16)
    feats = (C.c_void_p * 1)(16) if family == "ensemble" else one
    call = lambda n, ml, t, f, u, r, o: entry(None, f, 2, n, ml, t, 0, 0, u, r, o, None)      # noqa: E731
    _err(call(9, 0, 0.0, None, None, None, None), "outside 1..8")
    _err(call(5, 0, 0.0, None, None, None, None), "temperature")
    _err(call(5, 0, 1.0, None, None, None, None), "max_len")
    _err(call(5, 20, 1.0, None, None, None, C.byref(out)), "null argument")
    _err(call(5, 20, 1.0, feats, None, None, None), "null argument")
    _err(call(5, 20, 1.0, feats, one, None, C.byref(out)), "both or neither")
    _err(call(5, 20, 1.0, feats, None, one, C.byref(out)), "both or neither")
    _err(call(5, 20, 1.0, feats, None, None, C.byref(SampleDistinctOut(16, 16, None, 16, 16))), "null argument")
    _err(call(5, 20, 1.0, feats, None, None, C.byref(out)), "null handle")
    _err(call(5, 20, 1.0, feats, one, one, C.byref(out)), "null handle")


def test_python_value_errors():
    from simpleimagecaptionzoo_amd import stochastic_beam as sb
    assert sb.check_args(5, 20, 1.0, 100) == (5, 20, 1.0)
    for bad in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError, match="hypotheses per image"):
            sb.check_args(bad, 20, 1.0)
    with pytest.raises(ValueError, match="above the vocabulary"):
        sb.check_args(5, 20, 1.0, 4)
    for bad in (0, -1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="temperature"):
            sb.check_args(5, 20, bad)
    for bad in (0, 257, 2.5, True):
        with pytest.raises(ValueError, match="max_len"):
            sb.check_args(5, bad, 1.0)
    assert sb.rng_args(None, 3, 2, 5, 7) == (0, 0, None, None)
    assert sb.rng_args(-1, 3, 2, 5, 7) == (0xFFFFFFFFFFFFFFFF, 0, None, None)
    assert sb.rng_args((9, 4), 3, 2, 5, 7) == (9, 4, None, None)
    for bad in ((9, -1), (9, sb.MAX_IMAGES - 1)):
        with pytest.raises(ValueError, match="first_image"):
            sb.rng_args(bad, 3, 2, 5, 7)
    for bad in (1.5, True, "x", (1, 2.0), (1, True), [None, None]):
        with pytest.raises(ValueError, match="rng must be"):
            sb.rng_args(bad, 3, 2, 5, 7)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_philox_restatement_matches_the_twin_of_rng_h():
    rs = np.random.RandomState(0)
    c = [rs.randint(0, 2 ** 32, 50, dtype=np.uint64) for _ in range(4)]
    for k0, k1 in ((0, 0), (123, 456), (0xFFFFFFFF, 0x9E3779B9)):
        for a, b in zip(so.philox(*c, k0, k1), _philox._philox4x32_10(*c, k0, k1)):
            assert np.array_equal(a, b)
    u = so.bits_to_uniform(np.array([0, 1 << 9, 0xFFFFFFFF], dtype=np.uint64))
    assert u.dtype == np.float32 and u[0] == np.float32(2.0 ** -24) and u[2] == np.float32(1.0 - 2.0 ** -24) and (u > 0).all() and (u < 1).all()
    uu, root = so.philox_uniforms(77, 2, 2, 3, 10)
    assert uu.shape == (2, 2, 3, 10) and root.shape == (2,)
    assert np.array_equal(uu[1, 1, 2], so.philox_row(77, 2, 1, 2, 10)) and root[1] == so.philox_root(77, 1)
    # the slot stride is 8, not n: the uniforms of (image, slot) do not depend on n
    assert np.array_equal(so.philox_uniforms(77, 2, 2, 2, 10)[0], uu[:, :, :2])


def test_conditioning_map():
    rs = np.random.RandomState(1)
    for _ in range(200):
        Tp, Z = rs.uniform(-20, 5), rs.uniform(-25, 8)
        g = np.sort(Z - np.concatenate([[0.0], rs.exponential(3.0, 7)]))[::-1]
        G = so.condition(Tp, g, Z)
        assert G[0] == Tp                                      # the argmax maps to exactly Tp
        assert (np.diff(G) <= 0).all() and (G <= Tp).all()     # monotone, bounded by the parent
        naive = so.condition_naive(Tp, g, Z)
        ok = np.isfinite(naive)
        assert ok.any()
        np.testing.assert_allclose(G[ok], naive[ok], rtol=0, atol=1e-9 * max(1.0, np.exp(max(0.0, Tp - Z))))
    # where the naive formula overflows the stable one stays finite
    G = so.condition(-800.0, np.array([-790.0, -795.0]), -790.0)
    assert np.isfinite(G).all() and G[0] == -800.0 and G[1] < G[0]


N_DRAWS = 20000


def test_oracle_against_exact_enumeration():
    """toy model, V = 4, depth <= 3 with <end>: over 20 000 seeds the first and the second sequence of the n = 2 search occur with the
    Plackett-Luce probabilities p_i and sum_{j != i} p_j p_i / (1 - p_j), within 5 binomial standard deviations"""
    leaves = so.toy_leaves(3)
    assert len(leaves) == 40 and abs(sum(leaves.values()) - 1.0) < 1e-12
    step, state = so.toy_closure()
    seeds = np.arange(N_DRAWS, dtype=np.uint64)
    k0, k1 = so._key(seeds)
    roots = so.philox_root(seeds, 0)
    U = np.zeros((N_DRAWS, 4, 2, so.TOY_V), np.float32)
    for s in (1, 2, 3):
        for slot in (0, 1):
            U[:, s, slot] = so.bits_to_uniform(np.stack(so.philox(0, slot, s, so.RNG_GUMBEL, k0, k1), 1))
    assert np.array_equal(U[5, 2, 1], so.philox_row(5, 2, 0, 1, so.TOY_V))
    first, second = {}, {}
    for i in range(N_DRAWS):
        h = so.search(step, state, 2, 3, 1.0, lambda s, slot: U[i, s, slot], roots[i])
        assert len(h) == 2 and h[0].tokens != h[1].tokens and h[1].G < h[0].G <= so.gumbel(roots[i])
        first[tuple(h[0].tokens)] = first.get(tuple(h[0].tokens), 0) + 1
        second[tuple(h[1].tokens)] = second.get(tuple(h[1].tokens), 0) + 1
    assert set(first) <= set(leaves) and set(second) <= set(leaves)
    for k, p in leaves.items():
        p2 = sum(q * p / (1.0 - q) for j, q in leaves.items() if j != k)
        for want, got in ((p, first.get(k, 0)), (p2, second.get(k, 0))):
            sd = np.sqrt(want * (1.0 - want) / N_DRAWS)
            assert abs(got / N_DRAWS - want) <= 5.0 * sd, (k, want, got / N_DRAWS, sd)


def test_oracle_properties():
    step, state = so.toy_closure()
    leaves5 = so.toy_leaves(5, 0.7)
    for seed in range(40):
        T = (1.0, 0.7)[seed % 2]
        runs = {}
        for n in (1, 2, 3, 5, 8):
            gaps = []
            runs[n] = so.search(step, state, n, 5, T, so.philox_noise(seed, 0, so.TOY_V), so.philox_root(seed, 0), gaps)
            h = runs[n]
            assert len(h) == n                                 # 4^5 sequences: never short of n
            assert len({tuple(x.tokens) for x in h}) == n      # distinct
            G = [x.G for x in h]
            assert all(a > b for a, b in zip(G, G[1:])) and G[0] <= so.gumbel(so.philox_root(seed, 0))
            assert all(g >= 0 for g in gaps)
            for x in h:
                assert x.frozen == (x.tokens[-1] == so.END) and (x.frozen or len(x.tokens) == 5)
                if T == 0.7:
                    assert abs(x.phi - np.log(leaves5[tuple(x.tokens)])) < 1e-9      # phi = the sum of the token log-probs
            all_steps = so.search(step, state, n, 5, T, so.philox_noise(seed, 0, so.TOY_V), so.philox_root(seed, 0), all_steps=True)
            assert all_steps == h                              # the early-out changes nothing
        for j in (1, 2, 3, 5):                                 # the first j of the n = 8 run are the n = j run
            assert [x.tokens for x in runs[8][:j]] == [x.tokens for x in runs[j]]
            np.testing.assert_allclose([x.G for x in runs[8][:j]], [x.G for x in runs[j]], rtol=0, atol=1e-12)


def test_outputs_format():
    hyps = [so.Hyp([5, 7, 2], -1.5, 0.3, True), so.Hyp([4, 4, 4, 4], -2.5, -0.1, False)]
    ids, lens, fin, phi, G = so.outputs(hyps, 3, 4)
    assert ids.tolist() == [[5, 7, 2, 0], [4, 4, 4, 4], [0, 0, 0, 0]] and lens.tolist() == [3, 4, 0] and fin.tolist() == [1, 0, 0]
    assert phi[2] == -np.inf and G[2] == -np.inf and phi[0] == -1.5 and G[1] == -0.1


# ---- the input condition of the GPU tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", so.STEP_CASES, ids=lambda c: c.name)
def test_every_step_case_is_separated(case):
    """no comparison of tests/test_gpu_sample_distinct_step.py is excused: every margin of every case is above GAP_MIN"""
    inp = so.step_inputs(case)
    gaps = []
    ref = so.step_ref(case, inp, gaps)
    assert gaps and min(gaps) > so.GAP_MIN, (case.name, min(gaps))
    live = [r for r in range(case.n_img * case.n) if r % case.n < inp["occ"][r // case.n] and not inp["frozen"][r]]
    assert sorted(ref["cand"]) == live
    x = inp["x"][np.isfinite(inp["x"])]
    assert np.abs(x).max() <= 16.0 and np.nanmax(np.abs(inp["phi"])) <= 16.0
    if case.special == "finite3":
        assert len(ref["cand"][0][0]) == 3 and ref["occ"][0] == 3 < case.n
    if case.special == "end":
        assert any(ref["frozen"][r] and not inp["frozen"][ref["src_row"][r]] for r in range(case.n_img * case.n) if r % case.n < ref["occ"][r // case.n])
    if case.special == "all_frozen":
        assert ref["occ"][0] == case.n and all(ref["frozen"][:case.n]) and (ref["src_row"][:case.n] == np.arange(case.n)).all()
    if case.special == "tie_frozen":
        assert inp["G"][1] == inp["G"][2] and inp["frozen"][1] and inp["frozen"][2]
        src = ref["src_row"][:ref["occ"][0]].tolist()
        assert 1 in src and 2 in src and src.index(1) + 1 == src.index(2)


def test_step_cases_cover_the_issue_shapes():
    cs = so.STEP_CASES
    assert {c.V for c in cs} == {53, 1000, 10102} and {c.n for c in cs} >= {1, 2, 5, 8} and {c.nsplit for c in cs} == {1, 2, 4}
    assert {c.T for c in cs} == {0.5, 1.0, 2.0} and any(c.compact for c in cs) and any(c.step == 1 and not c.compact for c in cs)
    assert any(c.ld == c.V for c in cs) and any(c.ld > c.V for c in cs)
    assert {c.special for c in cs} >= {"finite3", "end", "all_frozen", "tie_frozen", "step1"}


@pytest.mark.parametrize("name,regime", so.DECODE_GOLDENS)
def test_whole_decode_configs_are_separated(golden_dir, name, regime):
    """at least 90 % of the images of the whole-decode configs keep every margin above GAP_MIN under the float64 oracle alone"""
    ms = [so.decode_pair(golden_dir, name, regime, n, T, img)[1] for n, T in so.DECODE_NT for img in range(3)]
    assert np.mean([m > so.GAP_MIN for m in ms]) >= so.MIN_SHARE, ms
    for n, T in so.DECODE_NT:
        hyps = so.decode_pair(golden_dir, name, regime, n, T, 0)[0]
        assert len(hyps) == n and len({tuple(h.tokens) for h in hyps}) == n
    assert sorted({n for n, _ in so.DECODE_NT}) == [1, 3, 5, 8] and sorted({T for _, T in so.DECODE_NT}) == [0.7, 1.0] and len(so.DECODE_NT) == 8
    # the comparisons that take every image: the Philox runs of the prefix test, the batch and the copies comparisons
    for img in range(3):
        for n in (1, 3, 5, 8):
            assert so.philox_pair(golden_dir, name, regime, n, 1.0, img, so.PHILOX_SEEDS[name])[1] > so.GAP_MIN, (name, n, img)
        assert so.decode_pair(golden_dir, name, regime, *so.BATCH_NT, img, so.BATCH_SEED)[1] > so.GAP_MIN, (name, img)
        assert so.decode_pair(golden_dir, name, "nat", *so.COPIES_NT, img, so.COPIES_SEEDS[name])[1] > so.GAP_MIN, (name, img)
