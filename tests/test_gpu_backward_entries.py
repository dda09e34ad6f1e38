"""The backward entries of the three decoder families against the forward pass the handle holds: every entry x stored-pass pairing
either succeeds or is refused with its text, before anything is queued, and leaves the handle usable.  Through the Python handle API
only, at the tiny golden dims with 3 images, 4 steps and K = 2.

Stored pass: none (a fresh handle), sample, sample_n, rollouts, xe_forward (training mode), xe_forward_n (BUTD).  Entries: sample_backward,
sample_backward_objective, sample_backward_dlogp (BUTD), xe_backward, xe_backward_distill, xe_backward_swor, xe_backward_dlogits.
Every refusal pinned here is decided on the host ahead of the entry's first launch (require_mode, the grouped-forward refusals and
check_swor's row count in csrc/).  Cells left out: a fresh NIC handle, and sample_backward_objective on any fresh handle -- the Python
wrappers read the tensors of the last forward call before they reach the library; the same library state (nothing stored) is pinned
for them by the second call behind a successful one.
Right pairings: the loss and every gradient of a twin handle with graphs on (BUTD, AoA) are bit-equal to the eager handle's, on its
first call (capture) and its second (replay)."""
import os

import numpy as np
import pytest
import torch

import _aoa_refiner as ar

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, T, K, L = 3, 4, 2, 5
LENGTHS = [4, 3, 2]                        # steps per caption, decreasing; T = the longest, L = T + 1 columns
LENGTHS_N = [2, 4, 3, 3, 1, 4]             # K captions per image, row img * K + k, in any order
ROLLOUT_ENTRIES = ("sample_backward", "sample_backward_objective", "sample_backward_dlogp")
XE_ENTRIES = ("xe_backward", "xe_backward_distill", "xe_backward_swor", "xe_backward_dlogits")
ENTRIES = {"butd": ROLLOUT_ENTRIES + XE_ENTRIES, "aoa": ROLLOUT_ENTRIES[:2] + XE_ENTRIES, "nic": ROLLOUT_ENTRIES[:2] + XE_ENTRIES}
STORES = {"butd": ("none", "sample", "sample_n", "rollouts", "xe", "xe_n"), "aoa": ("none", "sample", "sample_n", "rollouts", "xe"),
          "nic": ("none", "sample", "sample_n", "rollouts", "xe")}
ROLLOUT_STORES, XE_STORES = ("sample", "sample_n", "rollouts"), ("xe", "xe_n")
GROUPED = {"xe_backward_distill": "icz_butd_xe_backward_distill: the stored forward pass is a grouped one",
           "xe_backward_swor": "icz_butd_xe_backward_swor: the stored forward pass is a grouped one",
           "xe_backward_dlogits": "icz_butd_xe_backward_dlogits: the stored forward pass is a grouped one"}
_FAMILIES, _HANDLES = {}, {}


def family(golden_dir, name):
    """dims, a handle factory and the features of one family (made once, shared, never changed)"""
    if name in _FAMILIES:
        return _FAMILIES[name]
    f = {"name": name}
    if name == "butd":
        from test_gpu_butd import make_handle
        g = dict(np.load(os.path.join(golden_dir, "butd_dec_tiny.npz")))
        _, R, D, _, _, _, V = [int(x) for x in g["dims"]]
        f["make"] = lambda: make_handle(g, max_rows=8)[0]
        gen = torch.Generator(device="cpu")
        gen.manual_seed(11)
        f["feats"] = torch.relu(torch.randn(B, R, D, generator=gen)).to(DEV)
    elif name == "nic":
        from test_gpu_nic import make
        g = dict(np.load(os.path.join(golden_dir, "nic_dec_tiny.npz")))
        _, _, E, V = [int(x) for x in g["dims"]]
        f["make"] = lambda: make(g, max_rows=8)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(12)
        f["feats"] = torch.randn(B, E, generator=gen).to(DEV)
    else:
        import test_cpu_scst_multisample_families as fam
        from simpleimagecaptionzoo_amd.aoa import AoaHandle
        cfg = (B,) + fam._tiny_dims() + (T, None, None)
        R, D, Hd, E, V, NH = cfg[1:7]
        sd = ar.state_dict_of(cfg, 13)

        def make():
            h = AoaHandle(R, D, Hd, E, V, NH, 8, 20)
            h.bind({k: v.to(DEV).contiguous() for k, v in sd.items()})
            return h
        f["make"] = make
        f["feats"] = ar.feats_of(cfg, 14).to(DEV)
    f["V"] = V
    rs = np.random.RandomState(15)

    def captions(lengths):
        caps = torch.zeros(len(lengths), L, dtype=torch.int64)
        for b, n in enumerate(lengths):
            caps[b, 0] = 1
            caps[b, 1:n] = torch.from_numpy(rs.randint(4, V, size=n - 1))
            caps[b, n] = 2
        return caps.to(DEV)
    f["caps"], f["caps_n"] = captions(LENGTHS), captions(LENGTHS_N)
    _FAMILIES[name] = f
    return f


def handle(f, graphs=False):
    key = (f["name"], graphs)
    if key not in _HANDLES:
        h = f["make"]()
        if graphs:
            h.enable_graphs(True)
        _HANDLES[key] = h
    return _HANDLES[key]


def store(f, h, what):
    """the forward pass `what` on the handle, Philox seeded -> rows of the stored pass"""
    from simpleimagecaptionzoo_amd.grouped import xe_forward_n
    from simpleimagecaptionzoo_amd.multisample import sample_n
    rng = h._make_rng(4242)
    if what == "sample":
        h.sample(f["feats"], T, rng)
    elif what == "sample_n":
        sample_n(h, f["feats"], K, T, rng)
    elif what == "rollouts":
        h.rollouts(f["feats"], T, rng)
    elif what == "xe":
        h.xe_forward(f["feats"], f["caps"], LENGTHS, rng, train=True)
    elif what == "xe_n":
        xe_forward_n(h, f["feats"], f["caps_n"], LENGTHS_N, K, rng, train=True)
    else:
        assert what == "none"
    return B * K if what in ("sample_n", "xe_n") else B


def _randn(shape, seed, dtype=torch.float32):
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    return torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype).to(DEV)


def inputs(f, rows, n_tok, live_shape=None):
    """the arguments of every entry for a stored pass of `rows` rows and `n_tok` packed tokens (made once per test: a replayed graph
    reads the same addresses); live_shape: what the objective's wrapper takes for (rows, T) -- the last forward call's third tensor"""
    from simpleimagecaptionzoo_amd.scst_objective import make_objective
    from simpleimagecaptionzoo_amd.swor import SworBatch
    n = rows + 1                            # one image of `rows` samples and its threshold slot
    rs = np.random.RandomState(16)
    return {"reward": _randn((rows, 1), 17).repeat(1, T).contiguous(),
            "objective": make_objective("reinforce", 1, entropy_weight=0.05, reward=_randn(live_shape or (rows, T), 18)),
            "dlogp": _randn((rows, T), 19), "teacher": _randn((n_tok, f["V"]), 20), "dpacked": _randn((n_tok, f["V"]), 21) * 0.01,
            "batch": SworBatch(None, LENGTHS[:rows] if rows <= B else sorted(LENGTHS_N, reverse=True), torch.arange(rows, dtype=torch.int32),
                               torch.arange(rows, dtype=torch.int64).view(1, rows)),
            "phi": torch.from_numpy((-rs.rand(n) * 15.0 - 0.1).astype(np.float32)),
            "G": torch.from_numpy(np.sort(rs.rand(n) * 10.0 - 12.0)[::-1].copy()), "scores": torch.from_numpy(rs.rand(n) * 3.0)}


def call(h, entry, a, grads):
    """one backward entry -> its loss outputs as one tensor (a copy: with graphs on they are persistent buffers)"""
    from simpleimagecaptionzoo_amd.distill import xe_backward_distill, xe_backward_dlogits
    from simpleimagecaptionzoo_amd.scst_objective import sample_backward_objective
    from simpleimagecaptionzoo_amd.swor import xe_backward_swor
    if entry == "sample_backward":
        out = h.sample_backward(a["reward"], grads)[:2]
    elif entry == "sample_backward_objective":
        out = sample_backward_objective(h, a["objective"], grads)[:2]
    elif entry == "sample_backward_dlogp":
        h.sample_backward_dlogp(a["dlogp"], grads)
        out = ()
    elif entry == "xe_backward":
        out = (h.xe_backward(grads, 0.1),)
    elif entry == "xe_backward_distill":
        out = xe_backward_distill(h, grads, [a["teacher"]], alpha=0.5, temperature=2.0)[:3]
    elif entry == "xe_backward_swor":
        (loss, by_image), stats = xe_backward_swor(h, grads, a["phi"], a["G"], a["scores"], a["batch"])[:2]
        out = (loss, by_image, stats.float().view(-1))
    else:
        xe_backward_dlogits(h, a["dpacked"], grads)
        out = ()
    return torch.cat([t.view(-1) for t in out]).clone() if out else torch.zeros(0, device=DEV)


def refusal(name, what, entry):
    """the text a pairing is refused with, None for a right one"""
    if entry in ROLLOUT_ENTRIES:
        return None if what in ROLLOUT_STORES else "%s: no rollout stored" % name
    if what == "xe_n":
        return GROUPED.get(entry)
    return None if what == "xe" else "%s: no XE forward stored" % name


def n_tokens(what, h=None):
    """packed tokens of the stored XE pass; behind another store, what the distillation wrapper still holds of the handle's last one"""
    if what in XE_STORES:
        return sum(LENGTHS_N) if what == "xe_n" else sum(LENGTHS)
    return getattr(h, "_xe_tokens", None) or sum(LENGTHS)


def still_usable(f, h, what):
    """behind a refusal: the pass that was stored still is (its own entry succeeds); with none stored the handle takes a new step"""
    rows = store(f, h, "sample") if what == "none" else B * K if what in ("sample_n", "xe_n") else B
    grads = h.new_grads()
    a = inputs(f, rows, n_tokens(what))
    loss = call(h, "xe_backward" if what in XE_STORES else "sample_backward", a, grads)
    assert bool(torch.isfinite(loss).all()) and any(bool(v.any()) for v in grads.values())


def _wrapper_needs_live(name, entry):
    return name == "nic" or entry == "sample_backward_objective"


def cells(right):
    out = []
    for name in ("butd", "aoa", "nic"):
        for what in STORES[name]:
            for entry in ENTRIES[name]:
                if (refusal(name, what, entry) is None) != right or (what == "none" and _wrapper_needs_live(name, entry)):
                    continue
                out.append((name, what, entry))
    return out


@pytest.mark.parametrize("name,what,entry", cells(False))
def test_wrong_pairing_is_refused_and_leaves_the_handle_usable(golden_dir, name, what, entry):
    from simpleimagecaptionzoo_amd._lib import IczError
    f = family(golden_dir, name)
    h = f["make"]() if what == "none" else handle(f)
    rows = store(f, h, what)
    live = tuple(h._live[2].shape) if entry == "sample_backward_objective" else None
    a = inputs(f, rows, n_tokens(what, h), live)
    full = {k: torch.full_like(v, 7.5) for k, v in h.new_grads().items()}
    with pytest.raises(IczError, match=refusal(name, what, entry)):
        call(h, entry, a, full)
    torch.cuda.synchronize()
    assert all(bool((v == 7.5).all()) for v in full.values())           # nothing was queued
    still_usable(f, h, what)
    if what == "none":
        h.close()


@pytest.mark.parametrize("name", ["butd", "aoa", "nic"])
def test_swor_row_count_against_the_stored_forward(golden_dir, name):
    from simpleimagecaptionzoo_amd._lib import IczError
    f = family(golden_dir, name)
    h = handle(f)
    store(f, h, "xe")
    a = inputs(f, 2, n_tokens("xe"))                                    # one image of two samples against the three stored rows
    full = {k: torch.full_like(v, 7.5) for k, v in h.new_grads().items()}
    with pytest.raises(IczError, match="2 sample rows, the stored forward pass has 3"):
        call(h, "xe_backward_swor", a, full)
    torch.cuda.synchronize()
    assert all(bool((v == 7.5).all()) for v in full.values())
    still_usable(f, h, "xe")


@pytest.mark.parametrize("name,what,entry", cells(True))
def test_right_pairing_succeeds_once_and_graphs_equal_eager(golden_dir, name, what, entry):
    from simpleimagecaptionzoo_amd._lib import IczError
    f = family(golden_dir, name)
    h = handle(f)
    rows = store(f, h, what)
    live = tuple(h._live[2].shape) if entry == "sample_backward_objective" else None
    a = inputs(f, rows, n_tokens(what, h), live)
    grads = h.new_grads()
    loss = call(h, entry, a, grads)
    assert bool(torch.isfinite(loss).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert any(bool(v.any()) for v in grads.values())
    # the stored pass is consumed: the same call again is refused, and so is every other entry's kind
    full = {k: torch.full_like(v, 7.5) for k, v in grads.items()}
    with pytest.raises(IczError, match=refusal(name, "none", entry)):
        call(h, entry, a, full)
    torch.cuda.synchronize()
    assert all(bool((v == 7.5).all()) for v in full.values())
    if not hasattr(h, "set_option"):
        return
    g = handle(f, graphs=True)
    g_grads = g.new_grads()
    for i in range(2):                      # the capture, then the replay
        store(f, g, what)
        g_loss = call(g, entry, a, g_grads)
        assert torch.equal(g_loss, loss), "graphs, call %d" % i
        for k, v in grads.items():
            assert torch.equal(g_grads[k], v), ("graphs, call %d" % i, k)
