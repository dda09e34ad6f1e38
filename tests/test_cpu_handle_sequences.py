"""What the committed call sequences of tests/_handle_sequences.py cover, asserted from the generator alone (no GPU): every
(family, seed, variant) tests/test_gpu_handle_sequences.py runs is a deterministic function of its arguments, holds every operation
kind of its family, has row counts on both sides of every route threshold, an option flip between two SCST steps of one shape, a
refresh behind an update, a rebind, two re-allocations of the training buffers ("growing") or none ("fixed"), and a raising call.
These are conditions on the committed seeds: a seed that fails one is replaced in _handle_sequences.SEEDS."""
import copy

import pytest

import _handle_sequences as hs

CASES = hs.cases()


def ids(case):
    return "%s-%d-%s" % case


def scst_steps(ops, family):
    """[(forward index, backward index, kind, images, samples per image, steps, decoder rows per step slot)]"""
    need = {i: rows for i, rows, _ in hs.walk_training(ops, family)}
    return [(op["fwd"], i, ops[op["fwd"]]["kind"], ops[op["fwd"]]["B"], ops[op["fwd"]].get("n", 1), ops[op["fwd"]]["T"], need[op["fwd"]])
            for i, op in enumerate(ops) if op["kind"] == "sample_backward"]


def test_the_committed_list_is_long_enough():
    assert len(hs.SEEDS["butd"]) >= 5 and len(hs.SEEDS["aoa"]) >= 5 and len(hs.SEEDS["nic"]) >= 2
    assert all(len(set(s)) == len(s) for s in hs.SEEDS.values())


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_sequence_is_deterministic_and_well_formed(case):
    family = case[0]
    a, b = hs.sequence(*case), hs.sequence(*case)
    assert a == b and a is not b
    assert copy.deepcopy(a) == hs.sequence(*case)
    assert 40 <= len(a) <= 60
    other = hs.sequence(case[0], case[1] + 1000, case[2])
    assert other != a
    assert all(op["kind"] in hs.KINDS[family] for op in a)
    for i, op in enumerate(a):                       # a backward pass names its forward pass, 0 - 2 operations in front of it
        if op["kind"] in hs.BACKWARD_KINDS:
            assert 1 <= i - op["fwd"] <= 3, (i, op)
            want = ("xe_forward",) if op["kind"] == "xe_backward" else ("sample", "rollouts", "sample_n")
            assert a[op["fwd"]]["kind"] in want
            between = a[op["fwd"] + 1:i]
            assert not any(o["kind"] in hs.FORWARD_KINDS + hs.BACKWARD_KINDS + hs.RAISE_KINDS for o in between)
        if op["kind"] in ("sample", "rollouts", "sample_n", "greedy", "sample_decode") and not (case[2] == "fixed" and i == 0):
            assert 3 <= op["T"] <= 8, op
        if "B" in op:
            assert 1 <= op["B"] * op.get("n", 1) <= hs.MAX_ROWS or op["kind"] == "raise_sample_n_capacity", op
        if "n_img" in op:
            assert op["n_img"] * op["k"] <= hs.MAX_ROWS and op["k"] % op.get("groups", 1) == 0 and op.get("n_best", 1) <= op["k"], op
        if op["kind"] == "xe_forward":
            assert op["lengths"] == sorted(op["lengths"], reverse=True) and len(op["lengths"]) == op["B"] and min(op["lengths"]) >= 1


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_sequence_holds_every_operation_kind_of_its_family(case):
    family = case[0]
    ops = hs.sequence(*case)
    kinds = {op["kind"] for op in ops}
    assert kinds == set(hs.KINDS[family]), set(hs.KINDS[family]) ^ kinds
    # and the forms of the kinds the issue lists
    assert {op["k"] for op in ops if op["kind"] == "beam_search"} == {1, 3, 5}
    opts = [op for op in ops if op["kind"] == "beam_search_opts"]
    assert any(o["n_best"] > 1 and o["length_penalty"] for o in opts) and any(o["groups"] > 1 and o["diversity"] > 0 for o in opts)
    assert any(o["block_ngram"] > 0 for o in opts)
    assert any(o["temperature"] != 1.0 and o["top_k"] > 0 and o["top_p"] < 1.0 and isinstance(o["seed"], int) for o in ops if o["kind"] == "sample_decode")
    flipped = {op["name"] for op in ops if op["kind"] == "set_option"}
    assert flipped == set(hs.OPTIONS[family]), set(hs.OPTIONS[family]) ^ flipped
    if family == "butd":
        assert any(op["want_alphas"] for op in ops if op["kind"] == "greedy")
        assert {op["n"] for op in ops if op["kind"] == "sample_n"} == {2, 4}
        assert {0, 16, 32} <= {op["value"] for op in ops if op["kind"] == "set_option" and op["name"] == "merge_small"}
    if family == "aoa":
        assert len({op["regions"] for op in ops if op["kind"] == "set_regions"} | {36}) >= 2
    if family != "nic":
        assert {op["on"] for op in ops if op["kind"] == "grad_callback"} == {True, False}
    xe = [op for op in ops if op["kind"] == "xe_forward"]
    assert any(len(set(op["lengths"])) > 1 for op in xe)                                                  # ragged
    assert {op["prob"] > 0 for op in ops if op["kind"] == "set_scheduled_sampling"} == {True, False}
    backs = [op for op in ops if op["kind"] == "sample_backward"]
    assert any(op["fresh_grads"] for op in backs) and any(not op["fresh_grads"] for op in backs)
    assert any(op["mask_sum_global"] == -1.0 for op in backs)
    for i, op in enumerate(ops):                     # a backward pass with -1 has a set_mask_sum_global since the backward pass before it
        if op["kind"] in hs.BACKWARD_KINDS and -1.0 in (op.get("mask_sum_global"), op.get("n_tokens_global")):
            j = i - 1
            while ops[j]["kind"] not in hs.BACKWARD_KINDS and ops[j]["kind"] != "set_mask_sum_global":
                j -= 1
            assert ops[j]["kind"] == "set_mask_sum_global", (i, op)
    # a rollout whose stored pass is dropped by the next forward pass
    fwd_with_backward = {op["fwd"] for op in ops if op["kind"] in hs.BACKWARD_KINDS}
    assert any(op["kind"] in ("sample", "rollouts", "sample_n") and i not in fwd_with_backward for i, op in enumerate(ops) if i > 1)
    # distances 0, and 1 or 2, between a forward pass and its backward pass
    gaps = {i - op["fwd"] - 1 for i, op in enumerate(ops) if op["kind"] == "sample_backward"}
    assert 0 in gaps and gaps & {1, 2}, gaps


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_sequence_straddles_the_row_routes(case):
    family = case[0]
    ops = hs.sequence(*case)
    steps = [s for s in scst_steps(ops, family) if s[0] > 1 or case[2] == "growing"]
    assert {hs.row_class(s[6]) for s in steps} >= {0, 1, 2, 3}, sorted(s[6] for s in steps)          # <= 16, 17 - 32, 33 - 64, 65 - 128 rows
    decode = [op["B"] for op in ops if op["kind"] == "greedy"]
    assert min(decode) <= 32 and any(33 <= b <= 64 for b in decode) and max(decode) > 64      # the routes of the greedy select tail
    beams = [op["n_img"] * op["k"] for op in ops if op["kind"] in ("beam_search", "beam_search_opts")]
    assert min(beams) < 64 and any(64 < b <= 128 for b in beams) and max(beams) > 128, beams
    if family == "butd":                             # merge_small on either side
        merged = {s[6] == 2 * s[3] for s in steps if s[2] == "rollouts"}
        assert merged == {True, False}


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_sequence_flips_an_option_between_two_scst_steps_of_one_shape(case):
    family = case[0]
    ops = hs.sequence(*case)
    steps = scst_steps(ops, family)
    found = False
    for a, b in zip(steps, steps[1:]):
        if a[2:6] == b[2:6] and any(o["kind"] == "set_option" and o["name"] != "graphs" for o in ops[a[1] + 1:b[0]]):
            found = True
    assert found
    if family == "butd":
        # sample and merged rollouts of one shape back to back (their backward passes differ in the slot geometry alone), and
        # rollouts of one shape in two chains and then merged
        assert any(a[2] == "sample" and b[2] == "rollouts" and a[3:6] == b[3:6] and b[6] == 2 * b[3] and b[0] == a[1] + 1 for a, b in zip(steps, steps[1:]))
        assert any(a[2] == b[2] == "rollouts" and a[3:6] == b[3:6] and a[6] == a[3] and b[6] == 2 * b[3] for a, b in zip(steps, steps[1:]))


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_sequence_refreshes_rebinds_grows_and_raises(case):
    family, _, variant = case
    ops = hs.sequence(*case)
    kinds = [op["kind"] for op in ops]
    assert "update_refresh" in kinds                 # the operation is the in-place update followed by refresh
    i = kinds.index("rebind")                        # the same captured call in front of the rebind and behind it
    same = ("greedy",) if family != "aoa" else ("rollouts",)
    before = [o for o in ops[:i] if o["kind"] in same][-1]
    after = [o for o in ops[i + 1:] if o["kind"] in same][0]
    assert {k: v for k, v in before.items() if k != "seed"} == {k: v for k, v in after.items() if k != "seed"}
    growths = hs.training_growths(ops, family)
    if variant == "growing":
        assert len([g for g in growths if g >= 5]) >= 2, growths                                      # in the middle of the sequence
        assert max(max(op["lengths"]) for op in ops if op["kind"] == "xe_forward") > hs.MAX_LEN
    else:
        assert growths in ([], [1]), growths         # the warm-up pair allocates (and may grow once between its two calls), nothing after
        rows, steps, xB, xT = hs.training_extent(ops[2:], family)
        assert (ops[0]["kind"], ops[0]["B"], ops[0]["T"]) == ("sample", rows, steps)
        assert (ops[1]["kind"], ops[1]["B"], max(ops[1]["lengths"])) == ("xe_forward", xB, xT)
    raising = {k for k in kinds if k in hs.RAISE_KINDS}
    assert raising == {k for k in hs.KINDS[family] if k in hs.RAISE_KINDS} and raising
