"""Randomised call sequences over the stateful decoder handles (VERDICT.md "Next round" item 3): the seeded sequences of
tests/_handle_sequences.py (40 - 60 operations: decodes, SCST and XE steps, option flips, parameter updates, rebinds, the gradient
callback, ensembles, calls that must raise) on BUTD at MIDWIDTH["w512"], AoA at AOA_MIDWIDTH["a512"] and NIC at the smallest width
of NIC_MIDWIDTH, every handle with 130 rows and max_len 8.

  * twin: a handle with hipGraphs on (toggled by the sequence's `graphs` flips) and a twin with graphs off get the same sequence on
    their own copies of the parameters; after every operation every output is bit-equal (torch.equal): ids, sequences, log-probs,
    scores, lens, loss, mask sum, every gradient tensor, packed logits, alphas, the stage counts of the gradient callback.
  * bursts: the same with the host synchronising only every 3 - 4 operations (the clones are stream-ordered): host-side uploads
    (the Philox seed, set_mask_sum_global) against replays.
  * fresh: at every fifth operation and at every evaluation-mode operation behind a state change, the handle that has seen the whole
    sequence against a fresh eager handle bound to the current parameter values and given the current options, which runs the two
    warm-up operations (training operations only: evaluation results must not depend on the training history) and then the
    operation alone (a backward pass: its forward pass and itself).  Bit-equal: nothing an earlier call left behind may show.
  * eviction: more distinct keys than the graph cache holds (24 BUTD, 16 AoA), then the evicted and the cached shapes again.

No operation pair needed a tolerance: every comparison in this file is torch.equal.

Wall time of this file on one MI355X, measured when it was added: 43 tests in 8.7 - 9.3 s (the slowest case 1.2 s, which also loads the
library and calibrates the <end> bias; the others 0.05 - 0.4 s).
"""
import numpy as np
import pytest
import torch

import _handle_sequences as hs
from _fullwidth import AOA_MIDWIDTH, MIDWIDTH, NIC_MIDWIDTH, _aoa_model, _nic_inputs

pytestmark = pytest.mark.gpu

BUTD_DIMS = MIDWIDTH["w512"][0]                                          # (R, D, H, E, A, V)
AOA_DIMS = AOA_MIDWIDTH["a512"][0]                                       # (R, D, Hd, E, V, NH)
NIC_DIMS = min((v[0] for v in NIC_MIDWIDTH.values()), key=lambda d: d[0] * d[1] * d[2])      # (E, H, V)
P_END = 0.5                       # a sampled step draws <end> with about this probability: rows finish inside 3 - 8 steps
BIAS_KEY = {"butd": "predict.bias", "aoa": "decoder.predict.bias", "nic": "predict.bias"}
DEV = "cuda"

_PARAMS = {}


def pristine(family):
    """The family's seeded parameters on the device, <end>-biased; never written: every handle binds clones (the ensemble partners
    bind these)."""
    if family not in _PARAMS:
        if family == "butd":
            from simpleimagecaptionzoo_amd.synth import random_butd_params
            p, V = random_butd_params(*BUTD_DIMS, DEV, seed=512), BUTD_DIMS[5]
        elif family == "aoa":
            cap = _aoa_model(AOA_DIMS, hs.MAX_ROWS, 512)
            p, V = {k: v.data.to(DEV).contiguous() for k, v in cap._named().items()}, AOA_DIMS[4]
            p["decoder.predict.weight_g"].div_(6.0)       # the maker's sharpening undone: with it one row in twelve never draws <end>
        else:
            p, V = _nic_inputs(NIC_DIMS, 1, 1, 512, 1, 1, 1.0, DEV)[0], NIC_DIMS[2]
        # <end>-biased as _fullwidth._end_biased_params does it: the bias is raised until a sampled first step draws <end> (stored
        # as 0) in about P_END of 64 rows
        bias, logit = p[BIAS_KEY[family]], lambda q: float(np.log(q / (1.0 - q)))
        bias[hs.END] += float(np.log(P_END * V / (1.0 - P_END)))
        h = new_handle(family)
        h.bind(p)
        feats = Inputs().feats(family, 64)
        for _ in range(3):
            h.refresh()
            seq, _ = h.sample(feats, hs.MAX_LEN, make_rng(family, 123))
            q = float((seq[:, 0] == 0).float().mean().clamp(1.0 / 256, 1.0 - 1.0 / 256))
            bias[hs.END] += logit(P_END) - logit(q)
        h.close()
        _PARAMS[family] = p
    return _PARAMS[family]


def new_handle(family):
    if family == "butd":
        from simpleimagecaptionzoo_amd.butd import ButdHandle
        return ButdHandle(*BUTD_DIMS, hs.MAX_ROWS, hs.MAX_LEN)
    if family == "aoa":
        from simpleimagecaptionzoo_amd.aoa import AoaHandle
        R, D, Hd, E, V, NH = AOA_DIMS
        return AoaHandle(R, D, Hd, E, V, NH, hs.MAX_ROWS, hs.MAX_LEN)
    from simpleimagecaptionzoo_amd.nic import NicHandle
    return NicHandle(*NIC_DIMS, hs.MAX_ROWS, hs.MAX_LEN)


def make_rng(family, seed):
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    from simpleimagecaptionzoo_amd.butd import make_rng as butd_rng
    return make_aoa_rng(seed) if family == "aoa" else butd_rng(seed)


def cuda_randn(shape, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV)


class Inputs:
    """Features and rewards, one tensor per shape for all handles of a test: the graph keys hold their addresses, as the Engine's do."""

    def __init__(self):
        self._feats, self._reward = {}, {}

    def feats(self, family, B, regions=36):
        key = (family == "nic", B, regions)
        if key not in self._feats:
            x = cuda_randn((B, NIC_DIMS[0]) if family == "nic" else (B, regions, BUTD_DIMS[1]), 1000 + 64 * B + regions)
            self._feats[key] = x if family == "nic" else torch.relu(x)
        return self._feats[key]

    def reward(self, rows, T, seed):
        buf = self._reward.get((rows, T))
        if buf is None:
            buf = self._reward[(rows, T)] = torch.zeros(rows, T, device=DEV)
        buf.copy_(cuda_randn((rows, 1), seed).expand(rows, T))       # stream-ordered, no host synchronisation
        return buf


def captions(B, lengths, V, seed):
    """[B, max(lengths) + 1] int64 on the device: <sta>, lengths[b] - 1 seeded words, <end>, zeros.  Built there, the lengths handed
    over from pinned memory without blocking: nothing here makes the host wait for the stream."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    n = torch.tensor(lengths, dtype=torch.int64).pin_memory().to(DEV, non_blocking=True).unsqueeze(1)
    col = torch.arange(max(lengths) + 1, device=DEV).unsqueeze(0)
    caps = torch.randint(4, V, (B, max(lengths) + 1), generator=g, device=DEV)
    caps = torch.where(col < n, caps, torch.zeros_like(caps))
    caps = torch.where(col == n, torch.full_like(caps, hs.END), caps)
    caps[:, 0] = 1
    return caps


class Runner:
    """One handle and everything a sequence does to it.  run(op) -> {name: cloned output}."""

    def __init__(self, family, inputs, graphs, params=None, config=None):
        from simpleimagecaptionzoo_amd._lib import IczError
        self.IczError = IczError
        self.family, self.inp, self.allow_graphs = family, inputs, graphs and family != "nic"
        self.params = {k: v.clone() for k, v in (params or pristine(family)).items()}
        self.h = new_handle(family)
        self.h.bind(self.params)
        self.V = self.h.V
        self.old, self.grads, self.stages, self.ens, self.partner = [], None, [], None, None
        # what a fresh handle needs to stand where this one stands: options, scheduled sampling, region count, callback, normaliser
        self.config = dict(config) if config else {"options": {}, "ss": 0.0, "regions": 36, "callback": False, "norm": None}
        self.config["options"] = dict(self.config["options"])
        if config:
            for name, value in config["options"].items():
                if name != "graphs":
                    self._set_option(name, value)
            if config["ss"] > 0:
                self.h.set_scheduled_sampling(config["ss"])
            if config["callback"]:
                self.h.set_grad_callback(self.stages.append)
            if config["norm"] is not None:
                self.h.set_mask_sum_global(torch.full((1,), config["norm"], device=DEV))
        if self.allow_graphs:
            self.h.enable_graphs(True)

    def close(self):
        if self.ens is not None:
            self.ens.close()
            self.partner.close()
        self.h.close()

    # ---- pieces -----------------------------------------------------------------------------------------------------------------
    def _set_option(self, name, value):
        from simpleimagecaptionzoo_amd._lib import check
        if name == "graphs":
            if self.allow_graphs:
                self.h.enable_graphs(bool(value))
        elif hasattr(self.h, "set_option"):
            self.h.set_option(name, value)
        else:                         # NicHandle has no set_option method (tests/test_cpu_handle_surface.py holds it to that): its entry
            check(self.h._e.set_option(self.h._h, name.encode(), int(value)))
        if name == "train_refiner":
            self.grads = None         # other gradient buffers: the refiner's are required / left out
        self.config["options"][name] = value

    def feats(self, B):
        return self.inp.feats(self.family, B, self.config["regions"])

    def _grads(self, fresh):
        if fresh or self.grads is None:
            g = self.h.new_grads()
            if not fresh:
                self.grads = g
            return g
        for v in self.grads.values():     # one persistent set, zeroed in place, as the Engine does
            v.zero_()
        return self.grads

    def _ensemble(self):
        from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
        if self.ens is None:
            other = "aoa" if self.family == "butd" else "butd"
            self.partner = new_handle(other)
            self.partner.bind(pristine(other))
            self.ens = EnsembleHandle([self.h, self.partner])
        return self.ens

    def _ens_feats(self, B):
        other = "aoa" if self.family == "butd" else "butd"
        return [self.feats(B), self.inp.feats(other, B, 36)]

    # ---- one operation ------------------------------------------------------------------------------------------------------------
    def run(self, op):
        out = self._run(op)
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}

    def _run(self, op):
        h, k, fam = self.h, op["kind"], self.family
        if k == "greedy":
            if op.get("want_alphas"):
                ids, alphas = h.greedy(self.feats(op["B"]), op["T"], want_alphas=True)
                return {"ids": ids, "alphas": alphas}
            return {"ids": h.greedy(self.feats(op["B"]), op["T"])}
        if k == "beam_search":
            seqs, lens = h.beam_search(self.feats(op["n_img"]), op["k"], op["steps"])
            return {"seqs": seqs, "lens": lens}
        if k in ("beam_search_opts", "ens_beam_search_opts"):
            args = (op["k"], op["steps"], op["n_best"], tuple(op["length_penalty"]), op["block_ngram"], op["groups"], op["diversity"])
            if k == "beam_search_opts":
                seqs, lens, scores = h.beam_search_opts(self.feats(op["n_img"]), *args)
            else:
                seqs, lens, scores = self._ensemble().beam_search_opts(self._ens_feats(op["n_img"]), *args)
            return {"seqs": seqs, "lens": lens, "scores": scores}
        if k == "ens_greedy":
            return {"ids": self._ensemble().greedy(self._ens_feats(op["B"]), op["T"])}
        if k == "sample_decode":
            ids, logp, score = h.sample_decode(self.feats(op["B"]), op["n"], op["T"], op["temperature"], op["top_k"], op["top_p"], op["seed"])
            return {"ids": ids, "logp": logp, "score": score}
        if k == "step":
            B, H = op["B"], BUTD_DIMS[2]
            g = torch.Generator(device=DEV)
            g.manual_seed(op["seed"])
            it = torch.randint(4, self.V, (B,), generator=g, device=DEV)
            st = [torch.randn(B, H, generator=g, device=DEV) * 0.5 for _ in range(4)]
            ctx, alpha, logits = h.step(self.feats(B), it, *st)
            return {"ctx": ctx, "alpha": alpha, "logits": logits, "h1": st[0], "c1": st[1], "h2": st[2], "c2": st[3]}
        if k == "sample":
            seq, lp = h.sample(self.feats(op["B"]), op["T"], make_rng(fam, op["seed"]))
            return {"seq": seq, "lp": lp}
        if k == "sample_n":
            seq, lp = h.sample_n(self.feats(op["B"]), op["n"], op["T"], make_rng(fam, op["seed"]))
            return {"seq": seq, "lp": lp}
        if k == "rollouts":
            ids, seq, lp = h.rollouts(self.feats(op["B"]), op["T"], make_rng(fam, op["seed"]))
            return {"ids": ids, "seq": seq, "lp": lp}
        if k == "sample_backward":
            grads = self._grads(op["fresh_grads"])
            n0 = len(self.stages)
            loss, msum = h.sample_backward(self.inp.reward(op["rows"], op["T"], op["reward_seed"]), grads, op["mask_sum_global"])[:2]
            out = {"loss": loss, "msum": msum, "stages": tuple(self.stages[n0:])}
            out.update({"d " + name: g for name, g in grads.items()})
            return out
        if k == "xe_forward":
            caps = captions(op["B"], op["lengths"], self.V, op["caption_seed"])
            logits = h.xe_forward(self.feats(op["B"]), caps, op["lengths"], make_rng(fam, op["seed"]) if op["train"] else None,
                                  train=op["train"], want_logits=True)
            return {"logits": logits}
        if k == "xe_backward":
            grads = self._grads(op["fresh_grads"])
            n0 = len(self.stages)
            loss = h.xe_backward(grads, 0.1, op["n_tokens_global"])
            out = {"loss": loss, "stages": tuple(self.stages[n0:])}
            out.update({"d " + name: g for name, g in grads.items()})
            return out
        if k == "set_scheduled_sampling":
            h.set_scheduled_sampling(op["prob"])
            self.config["ss"] = op["prob"]
            return {}
        if k == "set_option":
            self._set_option(op["name"], op["value"])
            return {}
        if k == "set_regions":
            self.config["regions"] = op["regions"]
            h.set_regions(op["regions"])
            return {}
        if k == "update_refresh":       # in place, relative size 1e-3, then refresh
            for i, (name, p) in enumerate(self.params.items()):
                p.add_(cuda_randn(p.shape, op["seed"] + i) * (1e-3 * p.abs().max()))
            h.refresh()
            return {}
        if k == "rebind":               # to clones; the old tensors stay alive, full of NaN: a stale pointer shows
            self.old.append(self.params)
            self.params = {name: p.clone() for name, p in self.params.items()}
            h.bind(self.params)
            for p in self.old[-1].values():
                p.fill_(float("nan"))
            return {}
        if k == "grad_callback":
            h.set_grad_callback(self.stages.append if op["on"] else None)
            self.config["callback"] = op["on"]
            return {}
        if k == "set_mask_sum_global":
            h.set_mask_sum_global(torch.full((1,), op["value"], device=DEV))
            self.config["norm"] = op["value"]
            return {}
        if k in ("raise_backward_no_rollout", "raise_second_backward"):
            grads = self.grads if self.grads is not None else self._grads(False)
            out = {"before d " + name: g.clone() for name, g in grads.items()}
            with pytest.raises(self.IczError):
                h.sample_backward(self.inp.reward(op["rows"], op["T"], 1), grads)
            out.update({"after d " + name: g for name, g in grads.items()})           # ... and change nothing: assert_unchanged
            out["raised"] = True
            return out
        if k == "raise_sample_n_capacity":
            with pytest.raises(self.IczError):
                h.sample_n(self.feats(op["B"]), op["n"], op["T"], make_rng(fam, 1))
            return {"raised": True}
        raise KeyError(k)


def assert_same(a, b, where):
    assert a.keys() == b.keys(), (where, sorted(a), sorted(b))
    for name in a:
        if torch.is_tensor(a[name]):
            assert a[name].shape == b[name].shape and torch.equal(a[name], b[name]), where + (name,)
        else:
            assert a[name] == b[name], where + (name, a[name], b[name])


def assert_unchanged(r, where):
    """the gradient buffers handed to a call that raised hold what they held (compared where the test synchronises anyway)"""
    for name in r:
        if name.startswith("before "):
            assert torch.equal(r[name], r["after " + name[7:]]), where + (name[7:],)


CASES = hs.cases()


def case_id(case):
    return "%s-%d-%s" % case


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_graph_handle_and_eager_twin_agree_after_every_operation(case):
    """Bit-equal outputs of a handle with graphs on and of its eager twin over one whole sequence; raising calls raise on both.
    Found by this test: (butd, seed 1, "fixed", operation 22, the greedy decode behind the rebind) on a library whose rebind kept its
    captured graphs -- the stale graph read the old, NaN-filled parameters, and the two-kernel argmax of a row of NaN logits
    (at most 32 or more than 64 rows) kept its initial index 0x7fffffff and read the embedding table far out of bounds; see
    test_greedy_over_nan_logits_decodes_pad."""
    family = case[0]
    ops, inp = hs.sequence(*case), Inputs()
    a, b = Runner(family, inp, True), Runner(family, inp, False)
    ended = 0
    for i, op in enumerate(ops):
        ra, rb = a.run(op), b.run(op)
        assert_same(ra, rb, case + (i, op["kind"]))
        assert_unchanged(ra, case + (i, op["kind"]))
        if "seq" in ra:
            ended += int((ra["seq"][:, -1] == 0).all())
    assert ended > 0                  # the regime does what it is for: some rollout ended before its last step
    torch.cuda.synchronize()
    a.close()
    b.close()


@pytest.mark.parametrize("case", [(f, hs.SEEDS[f][0], "fixed") for f in ("butd", "aoa")], ids=case_id)
def test_twins_agree_with_the_host_synchronising_every_few_operations(case):
    """The twin comparison in bursts of 3 - 4 operations without host synchronisation (outputs cloned in stream order, compared at
    the end of the burst), far below the cache capacity: the host-side uploads of a call (Philox seed, set_mask_sum_global) are
    ordered against the replays around it."""
    family = case[0]
    ops, inp = hs.sequence(*case), Inputs()
    a, b = Runner(family, inp, True), Runner(family, inp, False)
    i = 0
    while i < len(ops):
        n = 3 + (i // 3) % 2
        burst = ops[i:i + n]
        ra = [a.run(op) for op in burst]
        rb = [b.run(op) for op in burst]
        torch.cuda.synchronize()
        for j, (x, y) in enumerate(zip(ra, rb)):
            assert_same(x, y, case + (i + j, burst[j]["kind"]))
            assert_unchanged(x, case + (i + j, burst[j]["kind"]))
        i += n
    a.close()
    b.close()


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == "fixed"], ids=case_id)
def test_handle_with_history_agrees_with_a_fresh_handle(case):
    """The handle that has run the whole "fixed" sequence so far against a fresh eager handle (current parameter values, current
    options), at every fifth operation and at every evaluation-mode operation behind a state change.  Training operations: the
    fresh handle first runs the two warm-up operations (the same training capacity), a backward pass runs behind its own forward
    pass.  Evaluation-mode operations (greedy, beam search, sample_decode, step, ensembles): no warm-up -- their results must not
    depend on the training history.  Bit-equal.  Found by this test: nothing so far."""
    family = case[0]
    ops, inp = hs.sequence(*case), Inputs()
    a = Runner(family, inp, True)
    changed = False
    for i, op in enumerate(ops):
        ra = a.run(op)
        kind = op["kind"]
        if kind in hs.STATE_KINDS:
            changed = True
        is_eval = kind in hs.EVAL_KINDS
        assert_unchanged(ra, case + (i, kind))
        if not ra or "raised" in ra or i < 2 or not (i % 5 == 0 or (is_eval and changed)):
            continue
        f = Runner(family, inp, False, params=a.params, config=a.config)
        if not is_eval:
            f.run(ops[0])
            f.run(ops[1])
        if kind in hs.BACKWARD_KINDS:
            f.run(ops[op["fwd"]])
        rf = f.run(op)
        assert_same(ra, rf, case + (i, kind, "fresh"))
        f.close()
        if is_eval:
            changed = False
    a.close()


def _eviction(family, count, run):
    """`count` distinct keys on a cache that holds fewer, then the first three shapes (evicted: captured again) and the last three
    (still cached), a parameter update in front of each group; the eager twin gets the same calls."""
    inp = Inputs()
    a, b = Runner(family, inp, True), Runner(family, inp, False)

    def both(B):
        for i, op in enumerate(run(B)):
            ra, rb = a.run(op), b.run(op)
            torch.cuda.synchronize()
            assert_same(ra, rb, (family, "eviction", B, i, op["kind"]))
        return ra

    first = {B: both(B) for B in range(1, count + 1)}
    for seed, group in ((99, (1, 2, 3)), (100, (count - 2, count - 1, count))):
        update = {"kind": "update_refresh", "seed": seed}
        a.run(update), b.run(update)
        for B in group:
            again = both(B)
            assert not all(torch.equal(first[B][k], again[k]) for k in again if torch.is_tensor(again[k])), B     # the update shows
    a.close()
    b.close()


def test_butd_graph_cache_eviction():
    """greedy at B = 1 .. 26, T = 3 with graphs on: 26 keys on a cache of 24 (GraphCache gc{24}, butd_impl.h)."""
    _eviction("butd", 26, lambda B: [{"kind": "greedy", "B": B, "T": 3, "want_alphas": True}])


def test_aoa_graph_cache_eviction():
    """rollouts + sample_backward at B = 1 .. 18, T = 3 with graphs on: 36 keys on a cache of 16 (aoa_impl.h)."""
    def run(B):
        return [{"kind": "rollouts", "B": B, "T": 3, "seed": 7 + B},
                {"kind": "sample_backward", "fwd": 0, "rows": B, "T": 3, "reward_seed": 70 + B, "fresh_grads": False, "mask_sum_global": 0.0}]
    _eviction("aoa", 18, run)


@pytest.mark.parametrize("B", [8, 40, 70])
def test_greedy_over_nan_logits_decodes_pad(B):
    """A row whose logits are all NaN (diverged training) decodes <pad> on every row route of the greedy select: at most 32 and more
    than 64 rows take argmax_part_kernel + embed_argmax_kernel, 33 - 64 rows greedy_select_kernel.  No maximum is ever found, so the
    index stays at its initial value; both routes turn that into token 0 instead of gathering the embedding row 0x7fffffff."""
    a = Runner("butd", Inputs(), False)
    a.params["predict.bias"].fill_(float("nan"))
    a.h.refresh()
    ids = a.run({"kind": "greedy", "B": B, "T": 3})["ids"]
    assert ids.shape == (B, 3) and bool((ids == 0).all())
    a.close()
