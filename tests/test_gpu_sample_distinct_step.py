"""GPU tests of the kernels of stochastic beam search alone (include/icz.h: icz_test_sbs_rowtopk / _step / _init / _finalize) on the
cases of tests/_sbs_oracle.py against its float64 statement.  tests/test_cpu_sample_distinct.py asserts that every margin of every
case is above GAP_MIN, so no comparison here is excused: indices, sources, tokens, flags and counts are exact, g and phi + lp are
within 2e-5 of float64, and G is within 1e-9 of the float64 map applied to the device's own g."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _sbs_oracle as so  # noqa: E402

G_TOL, MAP_TOL = so.OWN_ERROR_MAX, 1e-9
CASES = so.STEP_CASES


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eq_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _row_inputs(c, inp, explicit=True):
    rows = c.n_img * c.n
    d = {"logits": _dev(inp["slabs"]), "bias": _dev(inp["bias"]) if c.nsplit > 1 else None, "uniforms": _dev(inp["uniforms"]) if explicit else None,
         "occ": _dev(inp["occ"]), "frozen": _dev(inp["frozen"]), "phi": _dev(inp["phi"]),
         "cand_g": torch.full((rows, 8), float("nan"), device="cuda"), "cand_phi": torch.full((rows, 8), float("nan"), device="cuda"),
         "cand_idx": torch.full((rows, 8), so.CANARY, dtype=torch.int32, device="cuda")}
    return d


def _rowtopk(c, d, seed=0):
    from simpleimagecaptionzoo_amd import stochastic_beam as sb
    sb.entry_rowtopk(d["logits"], d["bias"], c.nsplit, c.ld, c.n_img, c.n, c.V, c.step, c.compact, c.T, d["occ"], d["frozen"], d["phi"],
                     d["uniforms"], seed, d["cand_g"], d["cand_phi"], d["cand_idx"])
    torch.cuda.synchronize()
    return d["cand_g"].cpu().numpy(), d["cand_phi"].cpu().numpy(), d["cand_idx"].cpu().numpy()


def _check_cands(c, ref, g, ph, idx):
    for row in range(c.n_img * c.n):
        if row not in ref["cand"]:                             # not scored: nothing written
            assert np.isnan(g[row]).all() and np.isnan(ph[row]).all() and (idx[row] == so.CANARY).all(), (c.name, row)
            continue
        wi, wg, wp = ref["cand"][row]
        k = len(wi)
        assert idx[row, :k].tolist() == wi.tolist(), (c.name, row)
        assert (idx[row, k:c.n] == -1).all() and np.isneginf(g[row, k:c.n]).all() and np.isneginf(ph[row, k:c.n]).all(), (c.name, row)
        assert np.isnan(g[row, c.n:]).all() and np.isnan(ph[row, c.n:]).all() and (idx[row, c.n:] == so.CANARY).all(), (c.name, row)
        assert np.abs(g[row, :k].astype(np.float64) - wg).max(initial=0.0) <= G_TOL, (c.name, row, g[row, :k], wg)
        assert np.abs(ph[row, :k].astype(np.float64) - wp).max(initial=0.0) <= G_TOL, (c.name, row, ph[row, :k], wp)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_rowtopk_against_float64(case):
    inp = so.step_inputs(case)
    ref = so.step_ref(case, inp)
    g, ph, idx = _rowtopk(case, _row_inputs(case, inp))
    _check_cands(case, ref, g, ph, idx)
    g2, ph2, idx2 = _rowtopk(case, _row_inputs(case, inp))     # two runs are bit-equal
    assert g.tobytes() == g2.tobytes() and ph.tobytes() == ph2.tobytes() and idx.tobytes() == idx2.tobytes()


@pytest.mark.parametrize("case", [c for c in CASES if c.name in ("v53_n5", "v1000_n8_s4", "v10102_n5_s2", "step1_compact_n5", "finite3")],
                         ids=lambda c: c.name)
def test_philox_path_equals_the_restated_uniforms(case):
    """the noise made inside the selection sweep is the host's restatement of it, bit for bit"""
    inp = so.step_inputs(case)
    seed = 0x1234567887654321
    inp["uniforms"] = np.stack([np.stack([so.philox_row(seed, case.step, img, slot, case.V) for slot in range(case.n)])
                                for img in range(case.n_img)])
    want = _rowtopk(case, _row_inputs(case, inp))
    got = _rowtopk(case, _row_inputs(case, inp, explicit=False), seed)
    for a, b in zip(want, got):
        assert a.tobytes() == b.tobytes(), case.name
    assert (want[2][sorted(so.step_ref(case, inp)["cand"])][:, 0] >= 0).all()


def _step_state(c, inp):
    rows, L = c.n_img * c.n, inp["L"]
    st = _row_inputs(c, inp)
    st.update({"G": _dev(inp["G"]), "len": _dev(inp["len"]), "seqs_in": _dev(inp["seqs"]),
               "seqs_out": torch.full((rows, L), so.CANARY, dtype=torch.int32, device="cuda"),
               "src_row": torch.full((rows,), so.CANARY, dtype=torch.int32, device="cuda"),
               "it_next": torch.full((rows,), so.CANARY, dtype=torch.int64, device="cuda"),
               "n_live": torch.full((1,), 100, dtype=torch.int32, device="cuda")})
    return st


def _run_step(c, inp):
    from simpleimagecaptionzoo_amd import stochastic_beam as sb
    st = _step_state(c, inp)
    sb.entry_step(st, c.nsplit, c.ld, c.n_img, c.n, c.V, c.step, inp["L"], c.compact, c.T, 0)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in st.items() if v is not None}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_step_against_float64(case):
    inp = so.step_inputs(case)
    ref = so.step_ref(case, inp)
    got = _run_step(case, inp)
    _check_cands(case, ref, got["cand_g"], got["cand_phi"], got["cand_idx"])
    assert got["occ"].tolist() == ref["occ"].tolist() and int(got["n_live"][0]) == 100 + ref["n_live"], case.name
    for row in range(case.n_img * case.n):
        img, slot = divmod(row, case.n)
        if slot >= ref["occ"][img]:                            # past the survivors: src_row = itself, <pad>, nothing else
            assert got["src_row"][row] == row and got["it_next"][row] == 0, (case.name, row)
            for k in ("phi", "G", "frozen", "len"):
                assert got[k][row].tobytes() == inp[k][row].tobytes(), (case.name, row, k)
            assert (got["seqs_out"][row] == so.CANARY).all(), (case.name, row)
            continue
        ln = int(ref["len"][row])
        assert got["src_row"][row] == ref["src_row"][row] and got["it_next"][row] == ref["it_next"][row], (case.name, row)
        assert got["frozen"][row] == ref["frozen"][row] and got["len"][row] == ln, (case.name, row)
        assert got["seqs_out"][row, :ln].tolist() == ref["seqs_out"][row, :ln].tolist(), (case.name, row)
        assert (got["seqs_out"][row, ln:] == so.CANARY).all(), (case.name, row)
        assert abs(float(got["phi"][row]) - ref["phi"][row]) <= G_TOL, (case.name, row)
        if row in ref["parent_rank"]:                          # the float64 map applied to the device's own g
            par, rk = ref["parent_rank"][row]
            want = so.condition(inp["G"][par], float(got["cand_g"][par, rk]), float(got["cand_g"][par, 0]))
            assert abs(got["G"][row] - want) <= MAP_TOL, (case.name, row, got["G"][row], want)
            assert got["phi"][row] == got["cand_phi"][par, rk]
            if rk == 0:
                assert got["G"][row] == inp["G"][par]          # the row's argmax gets exactly the parent's G
        else:                                                  # a frozen hypothesis carries G and phi unchanged
            par = int(ref["src_row"][row])
            assert got["G"][row] == inp["G"][par] and got["phi"][row] == inp["phi"][par], (case.name, row)
    Gs = [got["G"][img * case.n:img * case.n + ref["occ"][img]] for img in range(case.n_img)]
    assert all((np.diff(g) <= 0).all() for g in Gs)            # slots sorted by G descending
    again = _run_step(case, inp)                               # two runs are bit-equal
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), (case.name, k)


def test_init_and_finalize():
    from simpleimagecaptionzoo_amd import stochastic_beam as sb
    n_img, n, L, seed = 5, 3, 6, 99
    rows = n_img * n
    for explicit in (False, True):
        rs = np.random.RandomState(3)
        root = so.bits_to_uniform(rs.randint(0, 2 ** 32, n_img, dtype=np.uint64)) if explicit else so.philox_root(seed, np.arange(n_img))
        occ = torch.full((n_img,), so.CANARY, dtype=torch.int32, device="cuda")
        frozen = torch.full((rows,), 7, dtype=torch.uint8, device="cuda")
        phi = torch.full((rows,), float("nan"), device="cuda")
        G = torch.full((rows,), float("nan"), dtype=torch.float64, device="cuda")
        ln = torch.full((rows,), so.CANARY, dtype=torch.int32, device="cuda")
        it = torch.zeros(rows, dtype=torch.int64, device="cuda")
        ior = torch.full((rows,), so.CANARY, dtype=torch.int32, device="cuda")
        src = torch.full((rows,), so.CANARY, dtype=torch.int32, device="cuda")
        sb.entry_init(n_img, n, _dev(root.astype(np.float32)) if explicit else None, seed, occ, frozen, phi, G, ln, it, ior, src)
        torch.cuda.synchronize()
        assert occ.tolist() == [1] * n_img and frozen.tolist() == [0] * rows and ln.tolist() == [0] * rows and it.tolist() == [1] * rows
        assert ior.tolist() == [r // n for r in range(rows)] and src.tolist() == list(range(rows))
        Gh, ph = G.cpu().numpy().reshape(n_img, n), phi.cpu().numpy().reshape(n_img, n)
        np.testing.assert_allclose(Gh[:, 0], so.gumbel(root), rtol=0, atol=1e-12)
        assert (ph[:, 0] == 0).all() and np.isneginf(ph[:, 1:]).all() and np.isneginf(Gh[:, 1:]).all()
    # finalize: occupied slots in order, a frozen and a cut hypothesis, unoccupied slots
    rs = np.random.RandomState(4)
    occ = np.array([3, 1, 0, 2, 3], np.int32)
    frozen = (rs.rand(rows) < 0.5).astype(np.uint8)
    ln = rs.randint(1, L + 1, rows).astype(np.int32)
    seqs = rs.randint(3, 50, (rows, L)).astype(np.int32)
    phi, G = (-8 * rs.rand(rows)).astype(np.float32), -5 * rs.rand(rows)
    ids, lens, fin, po, go = [t.cpu().numpy() for t in sb.entry_finalize(n_img, n, L, _dev(occ), _dev(frozen), _dev(phi), _dev(G), _dev(ln), _dev(seqs))]
    for row in range(rows):
        img, slot = divmod(row, n)
        if slot < occ[img]:
            assert ids[row, :ln[row]].tolist() == seqs[row, :ln[row]].tolist() and (ids[row, ln[row]:] == 0).all()
            assert lens[row] == ln[row] and fin[row] == frozen[row] and po[row] == phi[row] and go[row] == G[row]
        else:
            assert (ids[row] == 0).all() and lens[row] == 0 and fin[row] == 0 and np.isneginf(po[row]) and np.isneginf(go[row])
