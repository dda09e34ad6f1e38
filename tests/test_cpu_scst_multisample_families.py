"""CPU-only checks of the multi-sample SCST rollout of the AoA and NIC families (icz_aoa_sample_n, icz_nic_sample_n,
multisample.sample_n, Engine.SCST_multisample_training_epoch): argument errors before any device work, the Python signatures, and --
for tests/test_gpu_scst_multisample_families.py, which imports the case table below -- that the fp32 and the float64 oracle draw the
same tokens on every row of every AoA case, so that a row the GPU test excuses (a draw at a CDF edge) can only be the device's."""
import inspect
import os

import numpy as np
import pytest
import torch

import _aoa_refiner as ar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _tiny_dims():
    g = np.load(os.path.join(GOLDEN, "aoa_tiny.npz"))
    return tuple(int(x) for x in g["dims"])[1:]          # (R, D, Hd, E, V, NH)


# name -> (cfg = (B images, R, D, Hd, E, V, NH, T, region counts or None, <end> bias or None), K, seed).  The smallest shapes at which
# each piece of the rollout and its backward pass can go wrong:
#   tiny_*   the tiny golden's dims: one image (no second image to confuse a row with), K = 5 odd, K = 8 the most rows per image
#   packed   'adaptive' region counts, 5 and 36 among them: rows of one image share its packed offset and count
#   w64      the AOA_MIDWIDTH shape a256 (head width 64, 4 heads, odd V = 2051) at few rows
#   chunk    head width 256, 49 regions, 24 steps: 49152 / (8 (49 + 256)) = 20 (k, t) pairs per LDS chunk of the grouped d K / d V kernel
#   early    an <end> bias: every row has finished by step 3 (early-out counters count rows)
def aoa_cases():
    t = _tiny_dims()
    return {
        "tiny_1x2": ((1,) + t + (5, None, None), 2, 601),
        "tiny_3x5": ((3,) + t + (5, None, None), 5, 602),
        "tiny_2x8": ((2,) + t + (5, None, None), 8, 603),
        "packed": ((3, 36, 128, 512, 64, 53, 8, 4, [36, 5, 17], None), 3, 604),
        "w64": ((2, 36, 1024, 256, 192, 2051, 4, 4, None, None), 3, 605),
        "chunk": ((2, 49, 128, 512, 64, 53, 2, 24, None, None), 2, 606),
        "early": ((2, 36, 128, 512, 64, 53, 8, 6, None, 7.0), 4, 610),
    }


def aoa_inputs(name):
    """-> dict: cfg, K, sd (CPU fp32 state dict), feats [B, R, D], masks (decoder sites [T, B K, ...], refiner sites per image), u [T, B K]"""
    cfg, K, seed = aoa_cases()[name]
    B, R, D, Hd, E, V, NH, T = cfg[:8]
    sd = ar.state_dict_of(cfg, seed)
    feats = ar.feats_of(cfg, seed + 1)
    per_img, _ = ar.masks_of(cfg, seed + 2, B, T)
    per_row, u = ar.masks_of(cfg, seed + 3, B * K, T)
    masks = {k: (per_img if k in ("proj", "ref_att", "ref_aoa", "ref_sc") else per_row)[k] for k in ar.MASKS}
    return {"cfg": cfg, "K": K, "sd": sd, "feats": feats, "masks": masks, "u": u}


def repeated(c):
    """the case as the route that exists without sample_n sees it: features, region counts and the refiner's masks repeated K times"""
    cfg, K = c["cfg"], c["K"]
    rep = (cfg[0] * K,) + cfg[1:8] + (None if cfg[8] is None else [n for n in cfg[8] for _ in range(K)], cfg[9])
    masks = dict(c["masks"])
    masks["proj"] = np.repeat(masks["proj"], K, 0)
    for k in ("ref_att", "ref_aoa", "ref_sc"):
        masks[k] = np.repeat(masks[k], K, 1)
    return rep, c["feats"].repeat_interleave(K, 0), masks


def oracle_rollout(c, dt, grad=False):
    """The oracle's sampled rollout on the repeated inputs -> (params, seq, logprobs, logits [rows, steps run, V]); early exit as the
    reference's loop (and the library's)."""
    rep, feats, masks = repeated(c)
    with ar.oracle_dtype(rep[6], dt) as oa:
        p = {k: v.detach().to(dt).requires_grad_(grad) for k, v in c["sd"].items()}
        lg = []
        with torch.set_grad_enabled(grad):
            seq, lp = oa.sample_rl(feats.to(dt), p, c["u"].astype(np.float64), masks, rep[7], early_exit=True, lens=rep[8], logits_out=lg)
        return p, seq, lp, torch.stack(lg, 1)


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


@pytest.mark.parametrize("entry", ["icz_aoa_sample_n", "icz_nic_sample_n"])
def test_sample_n_rejects_bad_k_and_null_handle(entry):
    L = _lib()
    fn = getattr(L, entry)
    for K in (1, 9):
        assert fn(None, None, 4, K, 20, None, None, None, None) == -1
        assert b"K=%d" % K in L.icz_last_error() and b"outside 2..8" in L.icz_last_error()
    assert fn(None, None, 4, 5, 20, None, None, None, None) == -1
    assert b"null handle" in L.icz_last_error()


def test_signatures():
    from simpleimagecaptionzoo_amd import multisample
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, BUTDDetection_Eng, Engine, NIC_Eng
    assert str(inspect.signature(multisample.sample_n)) == "(handle, feats, n, max_len=20, rng=None)"
    want = "(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None, samples_per_image=5)"
    assert str(inspect.signature(Engine.SCST_multisample_training_epoch)) == want
    for cls in (BUTDDetection_Eng, AoADetection_Eng, NIC_Eng):
        assert cls.SCST_multisample_training_epoch is Engine.SCST_multisample_training_epoch


def test_entry_tables_hold_sample_n():
    from simpleimagecaptionzoo_amd.aoa import AoaHandle
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.nic import NicHandle
    L = _lib()
    for cls in (ButdHandle, AoaHandle, NicHandle):
        assert cls._entries().sample_n is getattr(L, "icz_%s_sample_n" % cls.family)


@pytest.mark.parametrize("k", [1, 9, 0, -3, True, False, 2.0, "4", None])
def test_engine_rejects_bad_k_before_anything_is_touched(k):
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, BUTDDetection_Eng, NIC_Eng
    for cls in (BUTDDetection_Eng, AoADetection_Eng, NIC_Eng):
        fake = cls.__new__(cls)                  # no constructor: the check comes before the model, the stream or the loader is looked at
        with pytest.raises(ValueError, match="samples_per_image"):
            cls.SCST_multisample_training_epoch(fake, [], None, None, samples_per_image=k)


def test_old_entry_refuses_aoa_and_nic_and_names_the_new_method():
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, NIC_Eng
    for cls in (AoADetection_Eng, NIC_Eng):
        with pytest.raises(ValueError, match="samples_per_image.*SCST_multisample_training_epoch"):
            cls.SCST_training_epoch(cls.__new__(cls), [], None, None, samples_per_image=4)


@pytest.mark.parametrize("name", list(aoa_cases()))
def test_fp32_and_float64_oracle_agree_on_every_row(name):
    """with the committed seeds no draw of any case sits at a CDF edge of the oracle itself"""
    c = aoa_inputs(name)
    cfg, K = c["cfg"], c["K"]
    _, s32, _, _ = oracle_rollout(c, torch.float32)
    _, s64, _, _ = oracle_rollout(c, torch.float64)
    assert s32.shape == (cfg[0] * K, cfg[7]) and torch.equal(s32, s64)
    if name == "early":
        assert bool((s64[:, 3:] == 0).all()) and bool(s64[:, 2].any())      # the last <end> falls at step 3
    else:
        assert bool(s64[:, -1].any())            # the last step ran
    # the K rows of an image are different captions (their dropout masks and draws differ)
    assert any(not torch.equal(s64[i * K], s64[i * K + 1]) for i in range(cfg[0]))
