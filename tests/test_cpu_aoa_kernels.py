"""Host-side half of the AoA kernels' own tests (tests/_aoa_kernels.py; the device half is tests/test_gpu_aoa_kernels.py):
every case takes the branch its purpose names (predicates written out from the kernels and launch helpers, the library's own route
entry where the threshold is the library's); the float64 references agree with oracle/aoa.py run in float64; the a-priori bounds hold
fp32 evaluations in two summation orders (not too tight) and reject every listed wrong reference (not too loose); and the entries
refuse on the host what their kernels cannot take.  The backward references are held to torch.autograd in float64."""
import ctypes as C

import numpy as np
import pytest
import torch

import _aoa_kernels as A
from _aoa_refiner import oracle_dtype


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _outside(val, ref, bound):
    """Elements of `val` outside the bound around `ref`."""
    return int((np.abs(val - ref) > bound).sum())


# ======================================================================================================================
# the tables hold what they are asked to hold, and every case takes its branch
def test_layer_norm_table_covers_the_branches():
    by = {(c.geometry, c.n) for c in A.LN_CASES}
    assert all((g, n) in by for g in (0, 1) for n in A.LN_N)
    assert {(c.geometry, c.rows) for c in A.LN_CASES} >= {(g, r) for g in (0, 1) for r in A.LN_ROWS}
    assert {c.stats for c in A.LN_CASES} == {True, False} and {c.live for c in A.LN_CASES} == {None, 0, 1}
    for g in (0, 1):
        assert {c.stats for c in A.LN_CASES if c.geometry == g} == {True, False}
        assert {(c.live, c.purpose["path"]) for c in A.LN_CASES if c.geometry == g and c.live is not None} == {
            (l, p) for l in (0, 1) for p in ("registers", "fallback")}
    want = {4: "registers", 8: "registers", 252: "registers", 256: "registers", 260: "registers", 1024: "registers", 2048: "registers",
            2052: "fallback", 10: "fallback"}
    for c in A.LN_CASES:
        assert c.purpose["path"] == ("registers" if c.n <= 256 * 8 and c.n % 4 == 0 else "fallback") and c.n >= 2
        if c.n in want:
            assert c.purpose["path"] == want[c.n], c.name
        nb, waves, idle = A.ln_blocks(c.geometry, c.rows)
        assert nb * waves - c.rows == idle == c.purpose["idle_waves"] and (c.geometry == 0 or idle == 0)
        assert A.ln_depth(c.n) >= (4 * -(-c.n // 256) + 6 if c.purpose["path"] == "registers" else -(-c.n // 64) + 6), c.name
    # geometry 0 with 1, 3 and 5 rows leaves waves of the last workgroup without a row; 4 rows leaves none
    assert {c.rows: c.purpose["idle_waves"] for c in A.LN_CASES if c.geometry == 0 and c.name.startswith("g0_rows")} == {1: 3, 3: 1, 4: 0, 5: 3}
    # trips of the register path: one, and both sides of one wave's 256 columns, up to all eight
    assert {c.purpose["trips"] for c in A.LN_CASES if c.purpose["path"] == "registers"} >= {1, 2, 4, 8}


def test_self_attention_cases_take_their_routes():
    from simpleimagecaptionzoo_amd.aoa_kernels import self_attn_route_for
    for c in A.SA_CASES:
        d = c.Hd // c.NH
        lens, off = A.offsets(c.counts, c.n_img, c.R)
        route, qc_lib, lds_lib = self_attn_route_for(c.R, c.Hd, c.NH, True)
        assert route == A.self_route(c.R, c.Hd, c.NH) == c.purpose["route0"], c.name
        r1, qc1, lds1 = self_attn_route_for(c.R, c.Hd, c.NH, False)
        assert r1 == 1 and qc1 == qc_lib == A.self_qc(c.R, d) and lds1 == A.self_lds(c.R, d, qc1) <= A.LDS_BUDGET, c.name
        assert lds_lib == (64 * 68 * 4 if route == 2 else lds1)
        assert (2 in c.routes) == (route == 2) and 1 in c.routes, c.name
        assert c.n_img >= 2 or c.counts == [1], c.name
        assert c.NH >= 2 and all(1 <= n <= c.R for n in lens)
        qc = c.qc or qc_lib
        assert qc == c.R or (qc % 4 == 0 and 4 <= qc < c.R), c.name
        assert A.self_lds(c.R, d, qc) <= A.LDS_BUDGET
        pp = c.purpose
        if "pitch" in pp:
            assert A.aoa_pitch(d) == pp["pitch"] and pp["pitch"] % 4 == 0 and (pp["pitch"] // 4) % 2 == 1
        if "len_mod4" in pp:
            assert {n % 4 for n in lens} == pp["len_mod4"], c.name
        if "chunks" in pp:
            assert A.sa_chunks(lens[0] if c.counts is not None else c.R, qc) == pp["chunks"], c.name
        if "lds_side" in pp:
            assert (A.self_lds(c.R, d, qc) > A.LDS_OPTIN) == (pp["lds_side"] > 0), c.name
        if "second_key" in pp:
            assert (max(lens) > 64) == pp["second_key"], c.name
        if "tiles" in pp:
            assert ((max(lens) if c.counts is not None else c.R) + 15) // 16 == pp["tiles"], c.name
    # what the table must hold: pitches, region counts, count % 4, forced chunks with a short last pass, the opt-in, the library's chunking
    r1 = [c for c in A.SA_CASES if c.purpose["route0"] == 1]
    assert {c.purpose.get("pitch") for c in r1} >= {4, 12, 60}
    assert {c.R for c in r1 if c.counts is None} >= {1, 5, 36, 49, 64, 65, 128}
    assert set().union(*[c.purpose.get("len_mod4", set()) for c in r1]) == {0, 1, 2, 3}
    assert any(c.counts is not None and list(c.counts[:1]) == [c.R] and 1 in c.counts and 17 in c.counts for c in r1)
    assert {tuple(c.purpose["chunks"]) for c in r1 if c.qc} >= {(4,) * 9, (8, 5), (8, 1)}
    assert any(c.purpose.get("lds_side") == 1 and (c.R, c.Hd // c.NH) == (128, 64) for c in r1)
    assert any(not c.qc and len(c.purpose.get("chunks", [0])) > 1 for c in r1), "no case takes the library's own chunked path"
    r2 = [c for c in A.SA_CASES if 2 in c.routes]
    assert {c.Hd // c.NH for c in r2} == {64, 128} and {c.R for c in r2 if c.counts is None} >= {1, 5, 16, 17, 36, 49, 64}
    assert {tuple(c.counts) for c in r2 if c.counts is not None} >= {(36, 5, 17), (1,), (64, 16, 33)}
    assert any(c.idx0 for c in r1) and any(c.idx0 for c in r2)


def test_decoder_attention_cases_take_their_branches():
    for c in A.DA_CASES:
        d = c.Hd // c.NH
        lens, off = A.offsets(c.counts, c.n_img, c.R)
        imgs = A.da_images(c)
        assert len(imgs) == c.rows and all(0 <= i < c.n_img for i in imgs) and A.dec_lds(c.R, d) <= A.LDS_BUDGET, c.name
        pp = c.purpose
        if "second_key" in pp:
            assert (max(lens[i] for i in imgs) > 64) == pp["second_key"], c.name
        if "j_trips" in pp:
            assert -(-d // 256) == pp["j_trips"], c.name
        if "lds_side" in pp:
            assert (A.dec_lds(c.R, d) > A.LDS_OPTIN) == (pp["lds_side"] > 0), c.name
        if "unused" in pp:
            assert sorted(set(range(c.n_img)) - set(imgs)) == pp["unused"], c.name
        if pp.get("one_key"):
            assert any(lens[i] == 1 for i in imgs), c.name
    cs = A.DA_CASES
    assert {c.R for c in cs} >= {1, 36, 63, 64, 65, 128} and {c.Hd // c.NH for c in cs} >= {4, 8, 64, 260}
    assert any(c.counts and 1 in c.counts and c.R in c.counts for c in cs)
    assert any(c.img_of_row == [0, 0, 1, 1, 2, 2] for c in cs) and any(c.img_of_row and sorted(c.img_of_row) == list(range(c.n_img)) and
                                                                    c.img_of_row != list(range(c.n_img)) for c in cs)
    assert {c.qns for c in cs} >= {1, 2, 5} and {c.p_out for c in cs} == {True, False} and {c.live for c in cs} == {None, 0, 1}
    assert any(c.purpose.get("lds_side") == 1 for c in cs) and any(c.idx0 for c in cs) and any(c.purpose.get("unused") for c in cs)


# ======================================================================================================================
# the references against oracle/aoa.py in float64
def test_layer_norm_reference_agrees_with_the_oracle():
    for c in A.LN_CASES:
        x, g, b = A.ln_inputs(c)
        ref = A.layer_norm_ref(x, g, b)
        with oracle_dtype(8, torch.float64) as oa:
            y = oa.layer_norm(torch.from_numpy(x).double(), torch.from_numpy(g).double(), torch.from_numpy(b).double(), eps=A.EPS).numpy()
        assert _rel(ref["y"][0], y) <= 1e-12, c.name
        assert (ref["y"][1] > 0).all() and np.isfinite(ref["y"][1]).all()


def _identity_block(Hd):
    """Parameters with which oracle.aoa.aoa_block returns the attention output itself: identity linear_Q, and an AoA linear whose first
    half copies x and whose gate is sigmoid(50) = 1.0 in float64."""
    W = torch.zeros(2 * Hd, 2 * Hd, dtype=torch.float64)
    W[:Hd, :Hd] = torch.eye(Hd, dtype=torch.float64)
    bias = torch.cat([torch.zeros(Hd, dtype=torch.float64), torch.full((Hd,), 50.0, dtype=torch.float64)])
    return {"linear_Q.weight": torch.eye(Hd, dtype=torch.float64), "linear_Q.bias": torch.zeros(Hd, dtype=torch.float64),
            "aoa_module.0.weight": W, "aoa_module.0.bias": bias}


def _oracle_mask(n, idx0, keep):
    """The keep flags of a draw as the multiplier mask of oracle drop(): (1 - p) in front of idx0 (times 1 / (1 - p): unchanged)."""
    return torch.from_numpy(np.concatenate([np.full(idx0, 1.0 - A.ATT_P), keep.astype(np.float64)])[:n])


@pytest.mark.parametrize("mode", (0, 1))
def test_self_attention_reference_agrees_with_the_oracle(mode):
    for c in A.SA_CASES:
        qkv = A.sa_inputs(c)
        keep = A.sa_keep(c)
        ref = A.self_attn_ref(c, qkv, mode, keep, scale=1.0 / (1.0 - A.ATT_P))[0]
        lens, off = A.offsets(c.counts, c.n_img, c.R)
        pad = np.zeros((c.n_img, c.R, 3 * c.Hd))
        for i in range(c.n_img):
            pad[i, :lens[i]] = qkv[off[i]:off[i + 1]]
        pad = torch.from_numpy(pad)
        Hd = c.Hd
        with oracle_dtype(c.NH, torch.float64) as oa:
            mask = _oracle_mask(A.sa_draws(c), c.idx0, keep).view(c.n_img, c.NH, c.R, c.R) if mode else None
            out, _ = oa.aoa_block(pad[..., :Hd], None, _identity_block(Hd), "", att_mask=mask, bu_mask=oa.key_mask(c.counts, c.R).double()
                                  if c.counts is not None else None, kv_proj=(pad[..., Hd:2 * Hd].contiguous(), pad[..., 2 * Hd:].contiguous()))
        got = np.concatenate([out[i, :lens[i]].numpy() for i in range(c.n_img)])
        assert _rel(ref, got) <= 1e-12, (c.name, mode)


@pytest.mark.parametrize("mode", (0, 1))
def test_decoder_attention_reference_agrees_with_the_oracle(mode):
    for c in A.DA_CASES:
        slabs, bias, Kd, Vd = A.da_inputs(c)
        q = A.da_query(c, slabs, bias)
        keep = A.da_keep(c)
        ref = A.dec_attn_ref(c, q, Kd, Vd, mode, keep, scale=1.0 / (1.0 - A.ATT_P))
        lens, off = A.offsets(c.counts, c.n_img, c.R)
        imgs = A.da_images(c)
        Kp, Vp = np.zeros((c.rows, c.R, c.Hd)), np.zeros((c.rows, c.R, c.Hd))
        for b, i in enumerate(imgs):
            Kp[b, :lens[i]], Vp[b, :lens[i]] = Kd[off[i]:off[i + 1]], Vd[off[i]:off[i + 1]]
        with oracle_dtype(c.NH, torch.float64) as oa:
            mask = _oracle_mask(A.da_draws(c), c.idx0, keep).view(c.rows, c.NH, 1, c.R) if mode else None
            out, alpha = oa.aoa_block(torch.from_numpy(q).double().unsqueeze(1), None, _identity_block(c.Hd), "", att_mask=mask,
                                      bu_mask=oa.key_mask([lens[i] for i in imgs], c.R).double(), kv_proj=(torch.from_numpy(Kp), torch.from_numpy(Vp)))
        assert _rel(ref["xatt"][0], out[:, 0].numpy()) <= 1e-12, (c.name, mode)
        assert _rel(ref["P"][0].mean(1), alpha[:, 0].numpy()) <= 1e-12, (c.name, mode)
        behind = np.arange(c.R)[None, None, :] >= np.array([lens[i] for i in imgs])[:, None, None]
        for k in ("P", "Pd"):
            assert not ref[k][0][np.broadcast_to(behind, ref[k][0].shape)].any() and not ref[k][1][np.broadcast_to(behind, ref[k][0].shape)].any()
        assert np.abs(ref["P"][0].sum(2) - 1.0).max() <= 1e-14


def test_query_of_slabs_is_the_fp32_sum_in_slab_order():
    c = A.DA_BY_NAME["slabs_5"]
    slabs, bias, _, _ = A.da_inputs(c)
    q = A.da_query(c, slabs, bias)
    want = ((((slabs[0] + slabs[1]) + slabs[2]) + slabs[3]) + slabs[4]) + bias
    assert q.dtype == np.float32 and np.array_equal(q, want)
    one = A.DA_BY_NAME["r36_w8"]
    s1, b1, _, _ = A.da_inputs(one)
    assert np.array_equal(A.da_query(one, s1, b1), s1[0])


# ======================================================================================================================
# the bounds are not too tight: fp32 numpy in two summation orders lies within them, on every case
def test_layer_norm_bound_holds_fp32_in_two_orders():
    worst = 0.0
    for c in A.LN_CASES:
        x, g, b = A.ln_inputs(c)
        ref = A.layer_norm_ref(x, g, b)
        for order in A.ORDERS:
            y, mean, inv = A.layer_norm_f32(x, g, b, order)
            for k, v in (("y", y), ("mean", mean), ("inv", inv)):
                assert not _outside(v.astype(np.float64), *ref[k]), (c.name, order, k)
                worst = max(worst, float((np.abs(v - ref[k][0]) / ref[k][1]).max()))
    print("layer_norm fp32 emulations: worst error / bound %.3g" % worst)


@pytest.mark.parametrize("mode", (0, 1))
def test_self_attention_bound_holds_fp32_in_two_orders(mode):
    worst = 0.0
    for c in A.SA_CASES:
        qkv, keep = A.sa_inputs(c), A.sa_keep(c)
        ref, bound = A.self_attn_ref(c, qkv, mode, keep)
        assert (bound > 0).all()
        for order in A.ORDERS:
            o = A.self_attn_f32(c, qkv, mode, keep, order).astype(np.float64)
            assert not _outside(o, ref, bound), (c.name, order)
            worst = max(worst, float((np.abs(o - ref) / bound).max()))
    print("self-attention fp32 emulations, mode %d: worst error / bound %.3g" % (mode, worst))


@pytest.mark.parametrize("mode", (0, 1))
def test_decoder_attention_bound_holds_fp32_in_two_orders(mode):
    worst = 0.0
    for c in A.DA_CASES:
        slabs, bias, Kd, Vd = A.da_inputs(c)
        q, keep = A.da_query(c, slabs, bias), A.da_keep(c)
        ref = A.dec_attn_ref(c, q, Kd, Vd, mode, keep)
        for order in A.ORDERS:
            got = dict(zip(("xatt", "P", "Pd"), A.dec_attn_f32(c, q, Kd, Vd, mode, keep, order)))
            for k, v in got.items():
                assert not _outside(v.astype(np.float64), *ref[k]), (c.name, order, k)
                pos = ref[k][1] > 0
                worst = max(worst, float((np.abs(v - ref[k][0])[pos] / ref[k][1][pos]).max()))
            if order == "pairwise":        # the kernel's tree: at most 7 additions on a path, then the division
                assert np.abs(got["P"].astype(np.float64).sum(2) - 1.0).max() <= 8 * A.U, c.name
    print("decoder attention fp32 emulations, mode %d: worst error / bound %.3g" % (mode, worst))


# ======================================================================================================================
# ... and not too loose: every listed wrong reference falls outside them, on every case it applies to
def test_layer_norm_bound_rejects_wrong_references():
    for c in A.LN_CASES:
        x, g, b = A.ln_inputs(c)
        ref = A.layer_norm_ref(x, g, b)
        for mut in A.LN_MUTATIONS:
            bad = A.layer_norm_ref(x, g, b, mut)
            assert _outside(bad["y"][0], *ref["y"]) and _outside(bad["inv"][0], *ref["inv"]), (c.name, mut)


def test_self_attention_bound_rejects_wrong_references():
    applied = {m: 0 for m in A.SA_MUTATIONS}
    for c in A.SA_CASES:
        qkv, keep = A.sa_inputs(c), A.sa_keep(c)
        qc = c.qc or A.self_qc(c.R, c.Hd // c.NH)
        for mode in (0, 1):
            ref, bound = A.self_attn_ref(c, qkv, mode, keep)
            for mut in A.SA_MUTATIONS:
                if A.sa_mutation_applies(c, mut, mode, qc):
                    applied[mut] += 1
                    assert _outside(A.self_attn_ref(c, qkv, mode, keep, qc=qc, mut=mut)[0], ref, bound), (c.name, mode, mut)
    assert all(n >= 3 for n in applied.values()), applied


def test_decoder_attention_bound_rejects_wrong_references():
    applied = {m: 0 for m in A.DA_MUTATIONS}
    for c in A.DA_CASES:
        slabs, bias, Kd, Vd = A.da_inputs(c)
        q, keep = A.da_query(c, slabs, bias), A.da_keep(c)
        for mode in (0, 1):
            ref = A.dec_attn_ref(c, q, Kd, Vd, mode, keep)
            for mut in A.DA_MUTATIONS:
                if A.da_mutation_applies(c, mut, mode):
                    applied[mut] += 1
                    bad = A.dec_attn_ref(c, q, Kd, Vd, mode, keep, mut=mut)
                    assert _outside(bad["xatt"][0], *ref["xatt"]), (c.name, mode, mut)
                    if mut != "v_neighbour_head":          # the weights themselves are wrong too
                        assert _outside(bad["Pd"][0], *ref["Pd"]), (c.name, mode, mut)
    assert all(n >= 3 for n in applied.values()), applied


# ======================================================================================================================
# refusals: returned by the host checks, before anything touches a device
FAKE = C.c_void_p(0x1000)           # a 16-byte aligned non-null pointer that a refused call never reads
ODD = C.c_void_p(0x1004)


def _refused(status, *needles):
    from simpleimagecaptionzoo_amd._lib import lib
    msg = lib().icz_last_error().decode()
    assert status == -1 and all(n in msg for n in needles), (status, msg)


def test_route_entry_refuses_what_the_handle_refuses():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.aoa_kernels import self_attn_route_for
    for R, Hd, NH in ((0, 16, 2), (129, 16, 2), (36, 12, 2), (36, 16, 3), (36, 16, 0)):
        with pytest.raises(IczError):
            self_attn_route_for(R, Hd, NH)
    # the switch between the two kernels: 64 / 65 regions, heads of 64 / 48 / 128 columns, the option off
    assert [self_attn_route_for(*a)[0] for a in ((64, 128, 2, True), (65, 128, 2, True), (36, 96, 2, True), (36, 256, 2, True), (36, 128, 2, False))] == [
        2, 1, 1, 2, 1]


def test_entries_refuse_on_the_host():
    from simpleimagecaptionzoo_amd._lib import DropPArgs, lib
    L = lib()
    for geometry, rows, n, odd in A.LN_REFUSED:
        _refused(L.icz_test_aoa_layer_norm(geometry, ODD if odd else FAKE, FAKE, FAKE, FAKE, rows, n, None, None, None), "icz_test_aoa_layer_norm")
    _refused(L.icz_test_aoa_layer_norm(0, None, FAKE, FAKE, FAKE, 3, 8, None, None, None), "null")
    for route, R, Hd, NH, qc in A.SA_REFUSED:
        _refused(L.icz_test_aoa_self_attn(route, FAKE, FAKE, 2, R, Hd, NH, None, qc, None, None, None, None), "icz_test_aoa_self_attn")
    _refused(L.icz_test_aoa_self_attn(2, FAKE, FAKE, 2, 65, 128, 2, None, 0, None, None, None, None), "mha_self_mfma_kernel", "65 regions")
    _refused(L.icz_test_aoa_self_attn(2, FAKE, FAKE, 2, 36, 96, 2, None, 0, None, None, None, None), "mha_self_mfma_kernel", "48 columns")
    _refused(L.icz_test_aoa_self_attn(1, ODD, FAKE, 2, 36, 16, 2, None, 0, None, None, None, None), "16-byte")
    for bad in (DropPArgs(3, None, None, 0, 0, 0.1, 0), DropPArgs(1, None, None, 0, 0, 0.1, 0), DropPArgs(2, None, None, 0, 0, 0.1, 0),
                DropPArgs(1, 0x1000, None, 0, 0, 1.0, 0)):
        _refused(L.icz_test_aoa_self_attn(1, FAKE, FAKE, 2, 36, 16, 2, None, 0, C.byref(bad), None, None, None), "dropout")
        _refused(L.icz_test_aoa_dec_attn(FAKE, 1, 0, None, None, FAKE, FAKE, None, FAKE, None, None, 3, 3, 36, 16, 2, None, C.byref(bad), None, None), "dropout")
    for R, Hd, NH, qns, rows, n_img in A.DA_REFUSED:
        _refused(L.icz_test_aoa_dec_attn(FAKE, qns, 0, None, None, FAKE, FAKE, None, FAKE, None, None, rows, n_img, R, Hd, NH, None, None, None, None),
                 "icz_test_aoa_dec_attn")
    _refused(L.icz_test_aoa_dec_attn(FAKE, 1, 0, None, None, FAKE, FAKE, None, FAKE, None, None, 3, 3, 128, 520, 2, None, None, None, None), "LDS")
    # slabs without a bias / a store / a stride that holds a slab
    _refused(L.icz_test_aoa_dec_attn(FAKE, 2, 3 * 16, None, FAKE, FAKE, FAKE, None, FAKE, None, None, 3, 3, 36, 16, 2, None, None, None, None), "slabs")
    _refused(L.icz_test_aoa_dec_attn(FAKE, 2, 3 * 16 - 4, FAKE, FAKE, FAKE, FAKE, None, FAKE, None, None, 3, 3, 36, 16, 2, None, None, None, None), "slabs")


# ======================================================================================================================
# aoa_dkv_kernel
def test_dkv_cases_references_and_bounds():
    """The table holds the (G, T) and tc it is asked to hold and every tc = 0 case takes the passes its purpose names; the reference is
    the plain einsum; fp32 in two orders lies within the bound; a (k, t) pair skipped at a chunk edge falls outside it."""
    assert {(c.G, c.T) for c in A.DK_CASES} >= {(1, 1), (1, 7), (3, 5)} and any(c.counts for c in A.DK_CASES)
    assert any(set(c.tcs) >= {0, 1, 4, c.G * c.T} and (c.G * c.T) % 4 for c in A.DK_CASES)
    assert any(len(c.purpose["lib_chunks"]) > 1 for c in A.DK_CASES), "no case on which the handle's own rule chunks"
    worst = 0.0
    for c in A.DK_CASES:
        d, pairs = c.Hd // c.NH, c.G * c.T
        assert A.dkv_chunks(pairs, A.dkv_tc(pairs, c.R, d)) == c.purpose["lib_chunks"], c.name
        assert all(tc == 0 or (1 <= tc <= pairs and A.dkv_lds(tc, c.R, d) <= A.DKV_LDS) for tc in c.tcs), c.name
        dS, Pd, Qp, dx = A.dk_inputs(c)
        ref = A.dkv_ref(c, dS, Pd, Qp, dx)
        lens, off = A.offsets(c.counts, c.n_img, c.R)
        for (val, bound), w, x in zip(ref, (dS, Pd), (Qp, dx)):
            wt, xt = torch.from_numpy(w).double().view(c.T, c.n_img, c.G, c.NH, c.R), torch.from_numpy(x).double().view(c.T, c.n_img, c.G, c.NH, d)
            full = torch.einsum("tighr,tighj->irhj", wt, xt).reshape(c.n_img, c.R, c.Hd).numpy()
            want = np.concatenate([full[i, :lens[i]] for i in range(c.n_img)])
            assert _rel(val, want) <= 1e-12, c.name
        for order in A.ORDERS:
            for (val, bound), got in zip(ref, A.dkv_f32(c, dS, Pd, Qp, dx, order)):
                assert not _outside(got.astype(np.float64), val, bound), (c.name, order)
                worst = max(worst, float((np.abs(got - val)[bound > 0] / bound[bound > 0]).max()))
        for tc in c.tcs:
            tc = tc or A.dkv_tc(pairs, c.R, d)
            if tc < pairs:          # the first pair of the second pass, and the last pair of the first
                for skip in (tc, tc - 1):
                    bad = A.dkv_ref(c, dS, Pd, Qp, dx, skip=skip)
                    assert all(_outside(b[0], *r) for b, r in zip(bad, ref)), (c.name, tc, skip)
    print("dkv fp32 emulations: worst error / bound %.3g" % worst)


def test_dkv_entry_refuses_on_the_host():
    from simpleimagecaptionzoo_amd._lib import lib
    L = lib()
    for n_img, B, T, tc, R, Hd, NH, G in A.DK_REFUSED:
        _refused(L.icz_test_aoa_dkv(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, n_img, B, T, tc, R, Hd, NH, None, G, None, None), "icz_test_aoa_dkv")
    _refused(L.icz_test_aoa_dkv(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 7, 5, 0, 36, 16, 2, None, 3, None, None), "7 decoder rows", "2 images x 3 rows")


# ======================================================================================================================
# aoa_dec_attn_bwd_kernel
def test_decoder_attention_backward_reference_bounds_and_refusals():
    """The analytic backward agrees with torch.autograd (float64) of the forward reference's formulas to 1e-10; fp32 in two orders lies
    within the bound; the wrong references fall outside it; the table reaches both sides of the 48 KB opt-in, the second key per lane,
    heads above 256 columns, ns 1 and 3, keep_scale 1 and 1 / 0.9; and the entry refuses on the host."""
    from simpleimagecaptionzoo_amd._lib import lib
    cs = [(b, A.DA_BY_NAME[b.fwd]) for b in A.DB_CASES]
    assert {b.ns for b, _ in cs} == {1, 3} and {b.drop for b, _ in cs} == {True, False} and {c.live for _, c in cs} == {None, 0, 1}
    assert {A.db_lds(c.R, c.Hd // c.NH) > A.LDS_OPTIN for _, c in cs} == {True, False} and all(A.db_lds(c.R, c.Hd // c.NH) <= A.LDS_BUDGET for _, c in cs)
    assert any(c.Hd // c.NH > 256 for _, c in cs) and any(c.purpose.get("second_key") for _, c in cs) and any(c.img_of_row for _, c in cs)
    assert abs(A.db_keep_scale(A.DB_CASES[1]) - 1 / 0.9) < 1e-7 and A.db_keep_scale(A.DB_CASES[0]) == 1.0
    worst, applied = 0.0, {m: 0 for m in A.DB_MUTATIONS}
    for b, c in cs:
        c, q, Kd, Vd, P32, Pd32, dxq = A.db_inputs(b)
        ks = A.db_keep_scale(b)
        d = c.Hd // c.NH
        lens, off = A.offsets(c.counts, c.n_img, c.R)
        # autograd of x = sum_r drop(softmax(q K^T / sqrt(d)))_r V_r against the analytic backward on the float64 P of that forward pass
        keep = A.da_keep(c)
        fwd = A.dec_attn_ref(c, q, Kd, Vd, 1 if b.drop else 0, keep, scale=ks)
        ref64 = A.dec_attn_bwd_ref(c, q, Kd, Vd, fwd["P"][0], fwd["Pd"][0], dxq, ks)
        fac = A.drop_factor(A.da_draws(c), 1 if b.drop else 0, keep, A.ATT_P, c.idx0, ks)
        dx = torch.from_numpy(ref64["dx"][0])
        for row, img in enumerate(A.da_images(c)):
            n, r0 = lens[img], off[img]
            for h in range(c.NH):
                qt = torch.from_numpy(q[row, h * d:(h + 1) * d]).double().requires_grad_(True)
                kt = torch.from_numpy(Kd[r0:r0 + n, h * d:(h + 1) * d]).double().requires_grad_(True)
                vt = torch.from_numpy(Vd[r0:r0 + n, h * d:(h + 1) * d]).double()
                p = torch.softmax(kt @ qt / d ** 0.5, 0) * torch.from_numpy(fac[(row * c.NH + h) * c.R + np.arange(n)])
                ((p @ vt) * dx[row, h * d:(h + 1) * d]).sum().backward()
                scale = max(float(qt.grad.abs().max()), 1e-30)
                assert np.abs(ref64["dQp"][0][row, h * d:(h + 1) * d] - qt.grad.numpy()).max() <= 1e-10 * scale, (b.name, row, h)
                want = np.outer(ref64["dS"][0][row, h, :n], q[row, h * d:(h + 1) * d].astype(np.float64))
                assert np.abs(want - kt.grad.numpy()).max() <= 1e-10 * max(float(kt.grad.abs().max()), 1e-30), (b.name, row, h)
        ref = A.dec_attn_bwd_ref(c, q, Kd, Vd, P32, Pd32, dxq, ks)
        assert not _outside(A.db_dx(c, dxq).astype(np.float64), *ref["dx"]), b.name           # the fp32 slab sum in slab order
        for order in A.ORDERS:
            got = dict(zip(("dQp", "dS", "dx"), A.dec_attn_bwd_f32(c, q, Kd, Vd, P32, Pd32, dxq, ks, order)))
            for k, v in got.items():
                assert not _outside(v.astype(np.float64), *ref[k]), (b.name, order, k)
                pos = ref[k][1] > 0
                if pos.any():
                    worst = max(worst, float((np.abs(v - ref[k][0])[pos] / ref[k][1][pos]).max()))
        for mut in A.DB_MUTATIONS:
            if A.db_mutation_applies(b, mut):
                applied[mut] += 1
                bad = A.dec_attn_bwd_ref(c, q, Kd, Vd, P32, Pd32, dxq, ks, mut=mut)
                assert _outside(bad["dQp"][0], *ref["dQp"]), (b.name, mut)
    assert all(n >= 2 for n in applied.values()), applied
    print("decoder attention backward fp32 emulations: worst error / bound %.3g" % worst)
    L = lib()
    for R, Hd, NH, ns, rows, n_img, ks in A.DB_REFUSED:
        _refused(L.icz_test_aoa_dec_attn_bwd(FAKE, ns, rows, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, n_img, R, Hd, NH, None, ks, None, None, None),
                 "icz_test_aoa_dec_attn_bwd")


# ======================================================================================================================
# LayerNorm backward (both kernels) and the refiner self-attention backward
def test_layer_norm_backward_reference_bounds_and_refusals():
    """The table holds the widths around one vector per thread and the multi-vector path, 1 and 3 slabs, each optional operand null in
    turn, 1 and 2 slabs of dq_b, live 0; the analytic backward agrees with torch.autograd (float64) of the forward formula to 1e-10;
    fp32 in two orders lies within the bound; biased std and eps inside the sqrt fall outside it; the entry refuses on the host."""
    from simpleimagecaptionzoo_amd._lib import lib
    cs = A.LB_CASES
    for form in (0, 1):
        assert {c.n for c in cs if c.form == form} >= set(A.LB_N) and {c.ns_a for c in cs if c.form == form and c.has_a} >= {1, 3}
    assert {A.lb_vectors(n) for n in A.LB_N} == {1, 2, 4} and A.lb_vectors(1024) == 1 and A.lb_vectors(1028) == 2
    assert {c.ns_b for c in cs if c.form == 0} == {1, 2} and {c.live for c in cs if c.form == 0} == {None, 0, 1}
    assert {(c.has_a, c.has_b, c.has_res) for c in cs if c.form == 1} == {(True, True, True), (False, True, True), (True, False, True), (True, True, False)}
    worst = 0.0
    for c in cs:
        x, gain, dq_a, dq_b, res, stats = A.lb_inputs(c)
        x64 = x.astype(np.float64)
        st64 = np.stack([x64.mean(1), 1.0 / (x64.std(1, ddof=1) + A.EPS)], 1)
        ref64 = A.ln_bwd_ref(c, x, gain, dq_a, dq_b, res, st64)
        xt = torch.from_numpy(x64).requires_grad_(True)
        g = torch.from_numpy(gain).double()
        y = g * (xt - xt.mean(1, keepdim=True)) / (xt.std(1, keepdim=True) + A.EPS)
        (y * torch.from_numpy(ref64["dq_tot"][0])).sum().backward()
        want = xt.grad.numpy() + (0 if res is None else res.astype(np.float64))
        assert np.abs(ref64["dx"][0] - want).max() <= 1e-10 * np.abs(want).max(), c.name
        assert _rel(ref64["prod"][0], ref64["dq_tot"][0] * (y.detach() / g).numpy()) <= 1e-10, c.name
        ref = A.ln_bwd_ref(c, x, gain, dq_a, dq_b, res, stats)
        for order in A.ORDERS:
            got = dict(zip(("dx", "dq_tot", "prod"), A.ln_bwd_f32(c, x, gain, dq_a, dq_b, res, stats, order)))
            for k, v in got.items():
                assert not _outside(v.astype(np.float64), *ref[k]), (c.name, order, k)
                pos = ref[k][1] > 0
                worst = max(worst, float((np.abs(v - ref[k][0])[pos] / ref[k][1][pos]).max()))
        for mut in A.LB_MUTATIONS:
            assert _outside(A.ln_bwd_ref(c, x, gain, dq_a, dq_b, res, stats, mut=mut)["dx"][0], *ref["dx"]), (c.name, mut)
    print("LayerNorm backward fp32 emulations: worst error / bound %.3g" % worst)
    L = lib()
    for form, n, what in A.LB_REFUSED:
        _refused(L.icz_test_aoa_ln_bwd(form, FAKE, 1, ODD if what == "odd" else FAKE, 1 if form == 0 else 0, 3, FAKE, FAKE if form == 0 or what == "stats" else None,
                                       FAKE, FAKE if what == "res" or form == 1 else None, FAKE, FAKE if form == 1 else None, FAKE, n, None, None),
                 "icz_test_aoa_ln_bwd")


@pytest.mark.parametrize("mode", (0, 1))
def test_self_attention_backward_reference_and_bounds(mode):
    """Cases on both sides of the second key per lane and of the 48 KB opt-in; the analytic backward against torch.autograd (float64) to
    1e-10; fp32 in two orders within the bound; the wrong references outside it."""
    cs = A.SB_CASES
    assert {c.R for c in cs if c.counts is None} >= {1, 5, 36, 65, 128} and any(c.counts == [36, 5, 17] for c in cs)
    assert any((c.R, c.Hd // c.NH) == (128, 4) for c in cs) and any((c.R, c.Hd // c.NH) == (36, 64) for c in cs) and any(c.idx0 for c in cs)
    worst, applied = 0.0, {m: 0 for m in A.SB_MUTATIONS}
    for c in cs:
        d = c.Hd // c.NH
        lens, off = A.offsets(c.counts, c.n_img, c.R)
        assert A.sb_lds(c.R, d) <= A.LDS_BUDGET
        if "lds_side" in c.purpose:
            assert (A.sb_lds(c.R, d) > A.LDS_OPTIN) == (c.purpose["lds_side"] > 0), c.name
        if "second_key" in c.purpose:
            assert (max(lens) > 64) == c.purpose["second_key"], c.name
        qkv, dO = A.sb_inputs(c)
        keep = A.sa_keep(c)
        ref, bound = A.self_attn_bwd_ref(c, qkv, dO, mode, keep)
        fac = A.drop_factor(A.sa_draws(c), mode, keep, A.ATT_P, c.idx0)
        xt = torch.from_numpy(qkv).double().requires_grad_(True)
        loss = 0
        for img in range(c.n_img):
            n, r0 = lens[img], off[img]
            for h in range(c.NH):
                q, k, v = (xt[r0:r0 + n, w * c.Hd + h * d:w * c.Hd + (h + 1) * d] for w in range(3))
                F = torch.from_numpy(fac[((img * c.NH + h) * c.R + np.arange(n))[:, None] * c.R + np.arange(n)[None, :]])
                o = (torch.softmax(q @ k.t() / d ** 0.5, 1) * F) @ v
                loss = loss + (o * torch.from_numpy(dO[r0:r0 + n, h * d:(h + 1) * d]).double()).sum()
        loss.backward()
        assert np.abs(ref - xt.grad.numpy()).max() <= 1e-10 * max(float(xt.grad.abs().max()), 1e-30), c.name
        for order in A.ORDERS:
            got = A.self_attn_bwd_f32(c, qkv, dO, mode, keep, order).astype(np.float64)
            assert not _outside(got, ref, bound), (c.name, order)
            pos = bound > 0
            worst = max(worst, float((np.abs(got - ref)[pos] / bound[pos]).max()))
        for mut in A.SB_MUTATIONS:
            if A.sb_mutation_applies(c, mut, mode):
                applied[mut] += 1
                assert _outside(A.self_attn_bwd_ref(c, qkv, dO, mode, keep, mut=mut)[0], ref, bound), (c.name, mut)
    assert all(n >= 1 for m, n in applied.items() if mode or m != "drop_stride_len"), applied
    print("self-attention backward fp32 emulations, mode %d: worst error / bound %.3g" % (mode, worst))


def test_self_attention_backward_entry_refuses_on_the_host():
    from simpleimagecaptionzoo_amd._lib import lib
    L = lib()
    for R, Hd, NH in A.SB_REFUSED:
        assert A.sb_lds(R, Hd // NH) > A.LDS_BUDGET or R > 128 or (Hd // NH) % 4
        _refused(L.icz_test_aoa_self_attn_bwd(FAKE, FAKE, FAKE, 2, R, Hd, NH, None, None, None))
    _refused(L.icz_test_aoa_self_attn_bwd(FAKE, FAKE, FAKE, 2, 128, 256, 2, None, None, None), "train_refiner: the self-attention backward needs",
             "128 regions and heads of 128")
    _refused(L.icz_test_aoa_self_attn_bwd(ODD, FAKE, FAKE, 2, 36, 16, 2, None, None, None), "16-byte")
