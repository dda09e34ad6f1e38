"""Seeded call sequences for the BUTD, AoA and NIC decoder handles (not collected by pytest; no GPU, no torch).

sequence(family, seed, variant) -> a list of 40 - 60 operations, each a dict {"kind": ..., arguments}, a deterministic function of
its arguments.  tests/test_cpu_handle_sequences.py asserts from this list alone what every committed sequence covers;
tests/test_gpu_handle_sequences.py runs the list on a handle with hipGraphs on, on an eager twin and against fresh handles.

The shapes straddle the row routes of the library: decoder rows of at most 16, 17 - 32, 33 - 64 (the predict slab path) and 65 - 128
(the 128-row resident kernel), BUTD's `merge_small` on either side, beam rows n_img x k on both sides of 64 and of 128.  Rollouts and
decodes run 3 - 8 steps: the smallest range with the t == 0, the t > 0 and (on end-biased parameters) the early-out paths.

Variants: "fixed" starts with the largest SCST shape and the longest XE batch of the sequence (two forward passes whose stored pass
is dropped), so the capacity of the training buffers is constant behind them; "growing" has no warm-up and orders the training
shapes so that they tend to rise: the training buffers are re-allocated in the middle of the sequence.

What may stand between a forward pass and its backward pass (0 - 2 operations): a handle keeps ONE set of per-image tensors (BUTD:
mean features, enc_ctx; AoA: the refined features of a bank) that the backward pass reads again, so a decode over OTHER images in
between is a caller's error, as is an option that changes the layout of the stored pass.  The fillers are therefore a greedy decode
of the same images and the state changes a stored pass must survive: `graphs` flips, the gradient callback, set_mask_sum_global and
BUTD's backward-only options (`concurrent`, `small_nt`).
"""
import random

MAX_ROWS = 130                    # row capacity of every handle under test
MAX_LEN = 8                       # its max_len: an XE batch of more steps grows the training buffers
FAMILIES = ("butd", "aoa", "nic")
VARIANTS = ("fixed", "growing")
# committed seeds: every coverage condition of tests/test_cpu_handle_sequences.py holds for each (a seed that fails one is replaced)
SEEDS = {"butd": (1, 2, 3, 4, 5), "aoa": (1, 2, 3, 4, 5), "nic": (1, 2)}
ROW_CLASSES = ((1, 16), (17, 32), (33, 64), (65, 128))
MERGE_SMALL_DEFAULT = 8
REGIONS = (36, 24, 30)            # AoA: fixed region counts (the handle is created for 36)
END = 2

EVAL_KINDS = ("greedy", "beam_search", "beam_search_opts", "sample_decode", "step", "ens_greedy", "ens_beam_search_opts")
FORWARD_KINDS = ("sample", "rollouts", "sample_n", "xe_forward")
BACKWARD_KINDS = ("sample_backward", "xe_backward")
STATE_KINDS = ("set_option", "set_regions", "update_refresh", "rebind", "grad_callback", "set_mask_sum_global", "set_scheduled_sampling")
RAISE_KINDS = ("raise_backward_no_rollout", "raise_second_backward", "raise_sample_n_capacity")

KINDS = {
    "butd": ("greedy", "beam_search", "beam_search_opts", "sample_decode", "step", "sample", "rollouts", "sample_n", "sample_backward",
             "xe_forward", "xe_backward", "set_scheduled_sampling", "set_option", "update_refresh", "rebind", "grad_callback",
             "set_mask_sum_global", "ens_greedy", "ens_beam_search_opts") + RAISE_KINDS,
    "aoa": ("greedy", "beam_search", "beam_search_opts", "sample_decode", "sample", "rollouts", "sample_backward", "xe_forward",
            "xe_backward", "set_scheduled_sampling", "set_option", "set_regions", "update_refresh", "rebind", "grad_callback",
            "set_mask_sum_global", "ens_greedy", "ens_beam_search_opts", "raise_backward_no_rollout", "raise_second_backward"),
    "nic": ("greedy", "beam_search", "beam_search_opts", "sample_decode", "sample", "rollouts", "sample_backward", "xe_forward",
            "xe_backward", "set_scheduled_sampling", "set_option", "update_refresh", "rebind", "set_mask_sum_global",
            "raise_backward_no_rollout", "raise_second_backward"),
}
# the options a sequence flips, with the values it takes (the first is the handle's default)
OPTIONS = {
    "butd": {"graphs": (1, 0), "early_out": (1, 0), "merge_small": (MERGE_SMALL_DEFAULT, 0, 16, 32), "concurrent": (1, 0), "small_nt": (1, 0),
             "group_att": (0, 1)},
    "aoa": {"graphs": (1, 0), "early_out": (1, 0), "refine_pair": (1, 0), "mha_mfma": (1, 0), "train_refiner": (0, 1)},
    "nic": {"early_out": (1, 0)},
}


def row_class(rows):
    for i, (lo, hi) in enumerate(ROW_CLASSES):
        if lo <= rows <= hi:
            return i
    return len(ROW_CLASSES)


class _Gen:
    def __init__(self, family, seed, variant):
        assert family in FAMILIES and variant in VARIANTS
        self.family, self.variant = family, variant
        self.rng = random.Random("%s/%d/%s" % (family, seed, variant))
        self.state = {name: vals[0] for name, vals in OPTIONS[family].items()}
        self.callback = False
        self.regions = REGIONS[0]
        self.norm_pending = False
        self.ops = []

    # ---- single operations ----------------------------------------------------------------------------------------------------
    def seed(self):
        return self.rng.randrange(1, 1 << 30)

    def T(self):
        return self.rng.randint(3, 8)

    def emit(self, kind, **args):
        op = dict(kind=kind, **args)
        self.ops.append(op)
        return len(self.ops) - 1

    def option(self, name, value=None):
        if value is None:             # flip to another of its values
            value = self.rng.choice([v for v in OPTIONS[self.family][name] if v != self.state[name]])
        elif self.state[name] == value:
            return
        self.state[name] = value
        self.emit("set_option", name=name, value=value)

    def forward(self, kind, B, T, n=1):
        return self.emit(kind, B=B, T=T, seed=self.seed(), **({"n": n} if kind == "sample_n" else {}))

    def backward(self, fwd, fresh_grads=False):
        f = self.ops[fwd]
        rows = f["B"] * f.get("n", 1)
        self.emit("sample_backward", fwd=fwd, rows=rows, T=f["T"], reward_seed=self.seed(), fresh_grads=fresh_grads,
                  mask_sum_global=-1.0 if self.norm_pending else 0.0)
        self.norm_pending = False

    def norm_global(self):
        self.emit("set_mask_sum_global", value=float(self.rng.randint(20, 200)))
        self.norm_pending = True

    def filler(self, B, T):
        """one operation that may stand between a forward pass and its backward pass (module docstring)"""
        choices = ["greedy", "norm"]
        if self.family != "nic":
            choices += ["graphs", "callback"]
        if self.family == "butd":
            choices += ["concurrent", "small_nt"]
        c = self.rng.choice(choices)
        if c == "greedy":
            self.emit("greedy", B=B, T=T, want_alphas=False)
        elif c == "norm":
            self.norm_global()
        elif c == "callback":
            self.toggle_callback()
        else:
            self.option(c)

    def other_regions(self):
        self.regions = self.rng.choice([x for x in REGIONS if x != self.regions])
        self.emit("set_regions", regions=self.regions)

    def toggle_callback(self):
        self.callback = not self.callback
        self.emit("grad_callback", on=self.callback)

    def scst(self, kind, B, T, n=1, gap=None, fresh_grads=False, second_backward=False, norm=False):
        if norm:
            self.norm_global()
        fwd = self.forward(kind, B, T, n)
        if isinstance(gap, list):
            for name in gap:
                self.option(name)
        else:
            for _ in range(self.rng.randint(0, 2) if gap is None else gap):
                self.filler(B, T)
        self.backward(fwd, fresh_grads)
        if second_backward:
            self.emit("raise_second_backward", rows=B * n, T=T)

    def xe(self, B, max_steps, train, ss=None, gap=0, fresh_grads=False, lengths=None):
        if ss is not None:
            self.emit("set_scheduled_sampling", prob=ss)
        if lengths is None:           # caption lengths minus one, ragged, sorted descending; the longest is max_steps
            lengths = sorted([max_steps] + [self.rng.randint(2, max_steps) for _ in range(B - 1)], reverse=True)
        fwd = self.emit("xe_forward", B=B, lengths=lengths, caption_seed=self.seed(), seed=self.seed(), train=train)
        for _ in range(gap):
            self.filler(B, self.T())
        self.emit("xe_backward", fwd=fwd, fresh_grads=fresh_grads, n_tokens_global=-1.0 if self.norm_pending else 0.0)
        self.norm_pending = False

    def beam_opts(self, ens=False, diverse=False):
        k = self.rng.choice((4, 6)) if diverse else self.rng.choice((3, 5))
        n_img = self.rng.randint(2, MAX_ROWS // k)
        args = dict(n_img=n_img, k=k, steps=self.T(), n_best=self.rng.randint(2, 3), block_ngram=self.rng.choice((0, 2, 3) if diverse or ens else (2, 3)),
                    length_penalty=[self.rng.choice(("avg", "wu")), self.rng.choice((0.5, 0.7, 1.0))],
                    groups=2 if diverse else 1, diversity=self.rng.choice((0.3, 0.5, 1.0)) if diverse else 0.0)
        self.emit("ens_beam_search_opts" if ens else "beam_search_opts", **args)

    # ---- blocks: operations that stay together ----------------------------------------------------------------------------------
    def blocks(self):
        """-> [(training rows the block needs (0: none), training steps, function emitting it)]"""
        r, fam = self.rng, self.family
        # (the smallest batch is a few rows over all 8 steps: on the end-biased parameters of the GPU tests, where a step draws <end>
        # with probability 1 / 2, all of them have ended before the last step in most rollouts -- the steps behind return at entry)
        b1, b2, b3, b4 = r.randint(2, 4), r.randint(17, 32), r.randint(33, 64), r.randint(65, 128)
        t1, t2 = 8, self.T()
        out = []

        def add(rows, steps, fn):
            out.append((rows, steps, fn))

        # SCST over the four row classes
        if fam == "butd":
            # sample and the MERGED rollouts of one shape, one after the other on the same buffers: their backward passes differ in the
            # slot geometry (cur_rows, cur_row0) alone
            def pair():
                self.option("graphs", 1)
                self.option("merge_small", 16)
                self.scst("sample", b1, t1, gap=0)
                self.scst("rollouts", b1, t1, gap=0)
            add(2 * b1, t1, pair)

            # rollouts of one shape on either side of a merge_small flip: 17 - 32 rows in two chains, then 34 - 64 rows in one
            def flip():
                self.option("graphs", 1)
                self.option("merge_small", 0)
                self.scst("rollouts", b2, t2, gap=0)
                self.option("merge_small", 32)
                self.scst("rollouts", b2, t2, gap=0)
            add(2 * b2, t2, flip)
            n2 = r.randint(33, 64)
            add(2 * n2, 8, lambda: self.scst("sample_n", n2, self.T(), n=2, gap=r.randint(0, 1)))                                  # 66 - 128 rows
            n4 = r.randint(9, 16)

            def grouped():
                self.option("group_att")
                self.scst("sample_n", n4, self.T(), n=4, gap=0, fresh_grads=True)                                   # 36 - 64 rows
            add(4 * n4, 8, grouped)
            add(0, 0, lambda: self.emit("raise_sample_n_capacity", B=33, n=4, T=self.T()))                   # 132 rows > MAX_ROWS
        else:
            add(b1, t1, lambda: self.scst("sample", b1, t1))
            between = "refine_pair" if fam == "aoa" else "early_out"

            def flip():
                if fam == "aoa":
                    self.option("graphs", 1)
                self.scst("rollouts", b2, t2, gap=0)
                self.option(between)
                self.scst("rollouts", b2, t2, gap=0)
            add(b2, t2, flip)
        if fam == "butd":               # its backward-only options, flipped between a forward pass and its backward pass
            add(b3, 8, lambda: self.scst("rollouts", b3, self.T(), gap=["concurrent", "small_nt"], second_backward=True))
        else:
            add(b3, 8, lambda: self.scst("rollouts", b3, self.T(), gap=r.randint(1, 2), second_backward=True))

        def dropped():                  # a rollout with no backward pass before the next forward pass: the stored pass is dropped
            self.forward("rollouts", b1, self.T())
            self.scst(r.choice(("sample", "rollouts")), b4, self.T(), gap=0, fresh_grads=fam != "butd", norm=True)
        add(b4, 8, dropped)

        # parameters: update + refresh, rebind (in front of and behind it the same call, which a stale graph would answer)
        if fam == "aoa":                # its captured calls are rollouts and sample_backward
            def rebind():
                T = self.T()
                self.option("graphs", 1)
                self.scst("rollouts", b1, T, gap=0)
                self.emit("rebind")
                self.scst("rollouts", b1, T, gap=0)
            add(b1, 8, rebind)
        else:
            def rebind():
                B, T = r.randint(33, 64), self.T()      # 33 - 64 rows: the one-launch greedy select
                if fam == "butd":
                    self.option("graphs", 1)
                self.emit("greedy", B=B, T=T, want_alphas=False)
                self.emit("rebind")
                self.emit("greedy", B=B, T=T, want_alphas=False)
            add(0, 0, rebind)

        def update():
            B, T = r.randint(65, 128), self.T()
            self.emit("update_refresh", seed=self.seed())
            self.emit("greedy", B=B, T=T, want_alphas=fam == "butd")
        add(0, 0, update)

        # decode
        for k in (1, 3, 5):
            rows = {1: r.randint(2, 60), 3: r.randint(66, 126), 5: MAX_ROWS}[k]                          # beam rows: < 64, 65 - 128, > 128
            add(0, 0, lambda k=k, rows=rows: self.emit("beam_search", n_img=rows // k, k=k, steps=self.T()))
        add(0, 0, lambda: self.beam_opts())
        add(0, 0, lambda: self.beam_opts(diverse=True))
        add(0, 0, lambda: self.emit("sample_decode", B=r.randint(2, 32), n=r.randint(1, 4), T=self.T(), seed=self.seed(),
                                    temperature=r.choice((0.7, 1.3)), top_k=r.choice((5, 50)), top_p=r.choice((0.9, 0.6))))      # all three set
        if fam == "butd":
            add(0, 0, lambda: self.emit("step", B=r.choice((b1, b3)), seed=self.seed()))
        # greedy decodes over the three routes of the select tail: at most 32 rows here, 33 - 64 (the rebind pair; AoA: here), more
        # than 64 (behind the update)
        if fam != "nic":
            add(0, 0, lambda: self.emit("greedy", B=r.randint(2, 32), T=self.T(), want_alphas=False))
        if fam == "aoa":
            add(0, 0, lambda: self.emit("greedy", B=r.randint(33, 64), T=self.T(), want_alphas=False))
        if fam != "nic":
            add(0, 0, lambda: self.emit("ens_greedy", B=r.randint(2, 64), T=self.T()))
            add(0, 0, lambda: self.beam_opts(ens=True))

        # XE: scheduled sampling on and off; the growing variant's captions rise past MAX_LEN
        xa, xb = (MAX_LEN + 2, MAX_LEN + 5) if self.variant == "growing" else (r.randint(4, 7), r.randint(9, 12))
        xB1, xB2 = r.randint(3, 16), r.randint(33, 64)
        add(xB1, xa, lambda: self.xe(xB1, xa, True, ss=0.25, gap=r.randint(0, 1)))
        add(xB2, xb, lambda: self.xe(xB2, xb, bool(r.getrandbits(1)), ss=0.0, fresh_grads=True))

        # state changes on their own
        names = {"butd": ("early_out", "graphs"), "aoa": ("early_out", "mha_mfma", "graphs"),
                 "nic": ("early_out",)}[fam]
        for name in names:
            add(0, 0, lambda name=name: self.option(name))
        if fam != "nic":
            add(0, 0, self.toggle_callback)
            add(0, 0, self.toggle_callback)
        if fam == "aoa":
            for _ in range(2):
                add(0, 0, self.other_regions)
            rB = r.randint(2, 12)

            def refiner():              # the opt-in refiner backward: other gradient buffers, xs / ref_feats / bank pointers in the key
                self.option("train_refiner", 1)
                self.scst("rollouts", rB, self.T(), gap=0, fresh_grads=True)
                self.xe(rB, r.randint(3, 6), True)
                self.option("train_refiner", 0)
            add(rB, 8, refiner)
        add(0, 0, lambda: self.emit("raise_backward_no_rollout", rows=b1, T=t1))
        if fam == "nic":                # fewer kinds: more SCST steps and decodes to reach the length
            for _ in range(3):
                B = r.randint(2, 64)
                add(B, 8, lambda B=B: self.scst(r.choice(("sample", "rollouts")), B, self.T()))
            add(0, 0, lambda: self.emit("greedy", B=r.randint(2, 32), T=self.T(), want_alphas=False))
        return out

    def build(self):
        blocks = self.blocks()
        self.rng.shuffle(blocks)
        train = [i for i, b in enumerate(blocks) if b[0]]
        if self.variant == "growing":   # training shapes tend to rise: the blocks that train, ordered by their rows with some noise
            ordered = sorted((blocks[i] for i in train), key=lambda b: b[0] + self.rng.uniform(-6, 6))
            for i, b in zip(train, ordered):
                blocks[i] = b
        else:                           # warm-up: the largest SCST shape and the longest XE batch (filled in below)
            self.emit("sample", B=1, T=1, seed=self.seed())
            self.emit("xe_forward", B=1, lengths=[1], caption_seed=self.seed(), seed=self.seed(), train=False)
        for _, _, fn in blocks:
            fn()
        if self.variant == "fixed":
            rows, steps, xB, xT = training_extent(self.ops[2:], self.family)
            self.ops[0].update(B=rows, T=steps)
            self.ops[1].update(B=xB, lengths=[xT] * xB)
        assert 40 <= len(self.ops) <= 60, len(self.ops)
        return self.ops


def training_need(op, merge_small):
    """(rows, steps) the training buffers must hold for a forward operation (Butd / Aoa / Nic::ensure_train), None for any other"""
    k = op["kind"]
    if k == "sample":
        return op["B"], op["T"]
    if k == "sample_n":
        return op["B"] * op["n"], op["T"]
    if k == "rollouts":
        return (2 * op["B"] if op["B"] <= merge_small else op["B"]), op["T"]
    if k == "xe_forward":
        return op["B"], max(op["lengths"])
    return None


def walk_training(ops, family):
    """yields (index, rows, steps) of every forward operation, BUTD's merge_small followed through the option flips"""
    merge = MERGE_SMALL_DEFAULT if family == "butd" else 0
    for i, op in enumerate(ops):
        if op["kind"] == "set_option" and op["name"] == "merge_small":
            merge = op["value"]
        need = training_need(op, merge)
        if need:
            yield i, need[0], need[1]


def training_extent(ops, family):
    """(largest rows of an SCST forward pass, its most steps, largest XE batch, most XE steps) of `ops`"""
    rows = steps = xB = xT = 1
    for i, n_rows, n_steps in walk_training(ops, family):
        if ops[i]["kind"] == "xe_forward":
            xB, xT = max(xB, n_rows), max(xT, n_steps)
        else:
            rows, steps = max(rows, n_rows), max(steps, n_steps)
    return rows, steps, xB, xT


def training_growths(ops, family):
    """indices of the forward operations at which ensure_train re-allocates (the first allocation is not a growth)"""
    cap_B = cap_T = 0
    out = []
    for i, rows, steps in walk_training(ops, family):
        if rows > cap_B or steps > cap_T:
            if cap_B:
                out.append(i)
            cap_B, cap_T = max(cap_B, rows), max(cap_T, steps, MAX_LEN)
    return out


def sequence(family, seed, variant):
    return _Gen(family, seed, variant).build()


def cases():
    """every (family, seed, variant) the GPU tests run"""
    return [(f, s, v) for f in FAMILIES for s in SEEDS[f] for v in VARIANTS]
