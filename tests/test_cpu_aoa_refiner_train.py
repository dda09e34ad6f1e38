"""Host side of the AoA option "train_refiner" (no GPU): what the optimizer sees, the option-name error, the optimizer-state
checkpoint rule and the layout of the flat gradient buffer."""
import ctypes as C

import pytest
import torch

from simpleimagecaptionzoo_amd import _lib
from simpleimagecaptionzoo_amd._lib import AOA_DECODER_KEYS, AOA_PARAM_KEYS
from simpleimagecaptionzoo_amd.aoa import AoADetection_Captioner, AoaHandle
from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, FusedAdam

REFINER_KEYS = tuple(k for k in AOA_PARAM_KEYS if k not in AOA_DECODER_KEYS)


def captioner():
    return AoADetection_Captioner(23, 4, 32, 16, num_regions=5, enc_dim=24, max_batch=4, max_beam=1)


def test_param_groups_and_trainable_follow_the_attribute():
    cap = captioner()
    assert cap.train_refiner is False and len(REFINER_KEYS) == 64
    named = dict(cap.named_parameters())
    groups = cap.get_param_groups({"lr": 1e-3})
    assert len(groups) == 1 and groups[0]["lr"] == 1e-3
    assert [id(p) for p in groups[0]["params"]] == [id(p) for p in cap.decoder.parameters()]
    assert tuple(cap._trainable()) == AOA_DECODER_KEYS
    cap.train_refiner = True
    groups = cap.get_param_groups({"lr": 1e-3})
    assert len(groups) == 1 and len(groups[0]["params"]) == len(AOA_PARAM_KEYS) == 82
    assert {id(p) for p in groups[0]["params"]} == {id(p) for p in cap.parameters()}
    # the decoder's parameters keep the leading places: a decoder-only optimizer state is a prefix
    assert tuple(cap._trainable()) == AOA_DECODER_KEYS + REFINER_KEYS
    assert all(cap._trainable()[k] is named[k] for k in AOA_PARAM_KEYS)
    cap.train_refiner = False
    assert tuple(cap._trainable()) == AOA_DECODER_KEYS


def test_handle_unfreezes_the_refiner_keys_with_the_option():
    """AoaHandle._option_set (called by set_option once the library took the option): new_grads / _grad_struct cover every key."""
    h = AoaHandle.__new__(AoaHandle)
    assert h._frozen_keys == frozenset(REFINER_KEYS)
    h._option_set("train_refiner", 1)
    assert h._frozen_keys == frozenset()
    h._params = {k: torch.zeros(2) for k in AOA_PARAM_KEYS}
    assert set(h.new_grads()) == set(AOA_PARAM_KEYS)
    h._option_set("graphs", 1)
    assert h._frozen_keys == frozenset()
    h._option_set("train_refiner", 0)
    assert h._frozen_keys == frozenset(REFINER_KEYS) and set(h.new_grads()) == set(AOA_DECODER_KEYS)
    h._h = None          # never created: nothing for close() to destroy


def test_unknown_option_and_bad_value_texts():
    """The argument checks of icz_aoa_set_option come before anything touches the device."""
    L = _lib.lib()
    fake = C.c_void_p(8)          # never dereferenced on these paths
    assert L.icz_aoa_set_option(fake, b"train_refine", 1) != 0
    assert L.icz_last_error().decode() == "icz_aoa_set_option: unknown option 'train_refine'"
    assert L.icz_aoa_set_option(fake, b"train_refiner", 2) != 0
    assert "train_refiner takes 0 or 1, got 2" in L.icz_last_error().decode()
    assert L.icz_aoa_set_option(None, b"train_refiner", 1) != 0


def test_decoder_only_optimizer_state_does_not_load_into_a_train_refiner_optimizer():
    """The rule: it fails with a clear message, in both directions; equal groupings load."""
    cap = captioner()
    dec = FusedAdam(cap.get_param_groups({"lr": 1e-3}), 1e-3)
    saved = dec.state_dict()
    cap.train_refiner = True
    full = FusedAdam(cap.get_param_groups({"lr": 1e-3}), 1e-3)
    with pytest.raises(ValueError, match=r"different parameter grouping: the checkpoint holds \[18\] parameters per group, this optimizer \[82\].*train_refiner"):
        full.load_state_dict(saved)
    with pytest.raises(ValueError, match=r"holds \[82\] parameters per group, this optimizer \[18\]"):
        dec.load_state_dict(full.state_dict())
    full.load_state_dict(full.state_dict())
    dec.load_state_dict(saved)


class _Eng(AoADetection_Eng):
    """The engine's gradient-buffer logic over a CPU captioner (no handle, no device)."""

    def __init__(self, train_refiner=False):
        self.model = captioner()
        self.device = torch.device("cpu")
        self._flat = torch.zeros(1)         # a stale buffer the setter must drop
        self.train_refiner = train_refiner


@pytest.mark.parametrize("on", [False, True])
def test_flat_buffer_layout(on):
    """The decoder's stages and remainder lie where they lay; the refiner's slice is contiguous and last."""
    eng = _Eng(on)
    assert eng.train_refiner is on and eng.model.train_refiner is on
    assert (eng._flat is None) == on
    eng._flat = None
    views = eng._grads()
    ref = _Eng(False)
    ref._flat = None
    base = ref._grads()
    assert tuple(base) == AOA_DECODER_KEYS and len(ref._stage_slices) == 3
    off = lambda e, k: (e._gviews[k].data_ptr() - e._flat.data_ptr()) // 4
    for k in AOA_DECODER_KEYS:
        assert off(eng, k) == off(ref, k) and views[k].shape == base[k].shape, k
    assert eng._stage_slices[:2] == ref._stage_slices[:2] and eng._stage_slices[2][0] == ref._stage_slices[2][0]
    if not on:
        assert set(views) == set(AOA_DECODER_KEYS) and eng._flat.numel() == ref._flat.numel()
        return
    assert set(views) == set(AOA_PARAM_KEYS)
    named = dict(eng.model.named_parameters())
    lo = ref._flat.numel()                  # the refiner's slice starts where the decoder-only buffer ends
    for k in REFINER_KEYS:                  # in key order, each padded to 64 floats, nothing in between
        assert off(eng, k) == lo and views[k].shape == named[k].shape, k
        lo += (named[k].numel() + 63) // 64 * 64
    assert lo == eng._flat.numel() and eng._stage_slices[2] == (ref._stage_slices[2][0], lo)      # reduced with the remainder
    eng.train_refiner = False               # the flag changed: the cached buffer is dropped
    assert eng._flat is None and set(eng._grads()) == set(AOA_DECODER_KEYS)
