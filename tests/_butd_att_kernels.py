"""Case tables, float64 references and a-priori bounds of the twelve kernels in csrc/butd_kernels.h, each on its own: mean_feats(_counts),
att_scores / att_scores_group / att_scores_group_train, att_ctx / att_ctx_group, saved_alphas, att_bwd_dalpha, att_bwd_ddec,
att_bwd_denc / att_bwd_denc_group (tests/test_cpu_butd_att_kernels.py holds every case to its stated purpose and every reference to a
scalar loop and to torch.autograd; tests/test_gpu_butd_att_kernels.py runs the tables through the icz_test_att_* entries).  Plain numpy,
no pytest, no torch; not collected by pytest.

A case is a named shape with `tags`: what it is in the table for, as data.  TAGS maps each tag to a predicate on the shape and on the
kernels' constants (read out of the source by the CPU test), so a retuned constant turns a claim red instead of quietly emptying a case.

Two things are discontinuous and are taken exactly, never excused: the relu / keep "on" bits of the backward kernels, decided on ONE
fp32 addition of two given fp32 numbers (the reference forms the same np.float32 sum; zp of dwaff_part is that sum too), and dec_ctx
inside the score kernels, fp32 additions only (slab 0, slabs 1.. in order, then b_dec: dec_ctx_twin gives the kernel's bits).

Bounds are derived, never fitted (u = 2^-24 per fp32 operation; the rules of tests/_support_kernels.py and tests/_lstm_kernels.py):
  a sum            (additions on an element's path + 2) u sum|addends|, + 1 where every addend is itself a rounded product
  scores           the path: 16 per 1024 columns in the lane, 6 in the wave, 1 for b_aff; the addends w (1|2) relu(x + d) carry 2 u more
                   (the addition x + d, through the 1-Lipschitz relu, and the product)
  alpha            e^(s - max) / sum: u |s - max| from the subtraction, expf 3 ulp = 6 u, the sum of positive terms over 7 additions
                   9 u, the division 2.5 ulp = 5 u: (20 + |s - max|) u relative
  ctx              alpha's bound times |feats|, and a sum over ceil(c / 2) + 1 additions of rounded products
  mean             c additions, the division 5 u
  dalpha_part      the slab sum's bound (ns + 1) u sum|slabs| times |feats|, and a dot product of 8 products per lane + 6 in the wave
  ds               al (da - al . da): da over nparts - 1 additions, the dot over 7, one subtraction, one product
  ddec             ds's bound times |w| (1|2), and a sum over ceil(c / 4) + 3 additions of rounded products
  denc             a sum over T additions of rounded products ds w (1|2); grouped: + G additions over the rows' sums
  dwaff_part       a sum over (regions of the part) T additions of rounded products zp (1|2) ds
First order, times SECOND = 1 + 2^-10.  Where an output must be exact the bound is 0.  Every reference returns float64 (value, bound)."""
import collections

import numpy as np

from _lstm_kernels import SECOND, SEED, row_keep
from _philox import RNG_ATT
from _support_kernels import GUARD, U, seeded  # noqa: F401

EXP_U, DIV_U = 6.0, 5.0
NAN = np.float32(np.nan)
MASK_BYTES = (0, 1, 2, 255)
# the kernels' constants as this table assumes them (tests/test_cpu_butd_att_kernels.py reads them out of the source and compares)
CONST = {"ATT_PARTS": 4, "NB": 3, "RB": 9, "NR": 5, "TT": 20, "DALPHA_COLS": 512, "DENC_GROUP_REGS": 16, "ATT_CTX_MAX_G": 8, "ATT_MAX_R": 128}
DCTX_PAD = 8              # ldc = D + 8, NaN in the padding
ALPHA2_PAD = 3            # alpha_out2's row stride R + 3
STEP = 3                  # Philox step of the per-step kernels


def cdiv(a, b):
    return -(-a // b)


def f32(x):
    return np.asarray(x, dtype=np.float32)


# ======================================================================================================================
# cases
def _case(kind, fields, defaults):
    T = collections.namedtuple(kind, "name " + fields + " tags")

    def make(name, tags, **kw):
        d = dict(defaults)
        assert not set(kw) - set(d), set(kw) - set(d)
        d.update(kw)
        return T(name=name, tags=tuple(tags), **d)
    return make


# img: None = identity, else a tuple (image of each row); counts: None or a tuple per image; live: None, 1 or 0
_sc = _case("ScoreCase", "route rows n_img R A nsplit parts G mode row0 counts img live",
            dict(route=0, rows=3, n_img=3, R=5, A=20, nsplit=2, parts=0, G=0, mode=0, row0=0, counts=None, img=None, live=None))
AD_COUNTS = (1, 63, 64, 65, 100, 128)


def _score_cases():
    out = []
    a_tags = {4: ("one_float4", "lt_keep_word"), 20: ("lt_keep_word",), 132: ("tail_in_first_strip",), 256: ("whole_strips", "passes=1"),
              1028: ("passes=2", "pass_of_one_float4"), 1280: ("whole_strips", "passes=2"), 2304: ("whole_strips", "passes=3")}
    for A, tags in a_tags.items():
        for mode in (0, 1, 2):
            out.append(_sc("A%d_mode%d" % (A, mode), tags + (("shared_words",) if mode == 2 and "whole_strips" in tags else ()), A=A, mode=mode))
    r_tags = {1: ("one_region",), 2: ("R<=slots",), 16: ("R=slots",), 17: ("R>slots", "one_group"), 48: ("R=group",), 49: ("two_groups",),
              64: ("two_groups", "R=64")}
    for R, tags in r_tags.items():
        out.append(_sc("R%d" % R, tags + ("tail_in_first_strip",), R=R, A=132, mode=2))
    out.append(_sc("ad_mask", ("adaptive", "counts_around_64"), rows=6, n_img=6, R=128, A=132, mode=1, counts=AD_COUNTS))
    out.append(_sc("ad_philox", ("adaptive", "counts_around_64", "shared_words"), rows=6, n_img=6, R=128, A=256, mode=2, counts=AD_COUNTS))
    out.append(_sc("ad_nocounts_R100", ("adaptive",), rows=2, n_img=2, R=100, A=20, mode=1))
    for ns in (1, 5):
        out.append(_sc("nsplit%d" % ns, ("nsplit=%d" % ns,), nsplit=ns, A=132, mode=1))
    for p in (1, 4, 7):
        out.append(_sc("parts%d" % p, ("parts=%d" % p, "R<=slots" if p == 7 else "R>slots"), R=17, A=132, parts=p, mode=2))
    out.append(_sc("permuted", ("permuted_images", "unused_image"), rows=5, n_img=4, img=(2, 0, 2, 1, 0), A=132, mode=1))
    out.append(_sc("permuted_ad", ("permuted_images", "adaptive"), rows=5, n_img=3, R=70, img=(2, 0, 2, 1, 0), counts=(70, 3, 65), A=132, mode=2))
    for mode in (1, 2):
        out.append(_sc("row0_mode%d" % mode, ("row0",), rows=4, n_img=4, row0=2, A=256, mode=mode))
    out.append(_sc("dead", ("dead",), A=132, mode=2, live=0))
    out.append(_sc("live1", ("live",), A=132, mode=2, live=1))
    for G in (1, 2, 5, 8):
        out.append(_sc("group_G%d" % G, ("grouped", "G=%d" % G), route=1, G=G, n_img=2, rows=2 * G, R=17, A=132))
        for mode in (0, 1, 2):
            out.append(_sc("gtrain_G%d_mode%d" % (G, mode), ("grouped", "G=%d" % G), route=2, G=G, n_img=2, rows=2 * G, R=17, A=256 if mode == 2 else 132,
                           mode=mode))
    out.append(_sc("group_ad", ("grouped", "adaptive"), route=1, G=2, n_img=3, rows=6, R=128, A=132, counts=(65, 3, 128)))
    out.append(_sc("gtrain_ad", ("grouped", "adaptive"), route=2, G=2, n_img=3, rows=6, R=128, A=1028, mode=1, counts=(65, 3, 128)))
    out.append(_sc("gtrain_dead", ("grouped", "dead"), route=2, G=2, n_img=2, rows=4, A=132, mode=1, live=0))
    return out


SCORE_CASES = _score_cases()

_cc = _case("CtxCase", "rows n_img R D G counts img alpha2 live", dict(rows=3, n_img=3, R=37, D=36, G=0, counts=None, img=None, alpha2=False, live=None))


def _ctx_cases():
    out = []
    d_tags = {4: ("one_float4",), 36: (), 512: ("blocks=1", "full_block"), 516: ("blocks=2", "block_of_one_float4"), 1028: ("blocks=3",)}
    for D, tags in d_tags.items():
        out.append(_cc("D%d" % D, tags + ("third_loop",), D=D))
    r_tags = {1: ("halves=1|0",), 2: ("halves=1|1",), 19: ("halves=10|9", "second_batch"), 37: ("halves=19|18", "third_loop"), 64: ("third_loop", "R=64")}
    for R, tags in r_tags.items():
        out.append(_cc("R%d" % R, tags, R=R))
    out.append(_cc("ad", ("adaptive", "counts_around_64", "counts_around_128"), rows=7, n_img=7, R=128, counts=(63, 64, 65, 127, 128, 1, 2)))
    out.append(_cc("ad_D516", ("adaptive", "blocks=2"), rows=3, n_img=3, R=128, D=516, counts=(65, 128, 37)))
    out.append(_cc("alpha2", ("alpha2",), alpha2=True, D=516))
    out.append(_cc("alpha2_ad", ("alpha2", "adaptive"), alpha2=True, rows=2, n_img=2, R=100, counts=(100, 7)))
    out.append(_cc("permuted", ("permuted_images", "unused_image"), rows=5, n_img=4, img=(2, 0, 2, 1, 0)))
    out.append(_cc("dead", ("dead",), live=0))
    out.append(_cc("live1", ("live",), live=1))
    for G in (1, 2, 5, 8):
        out.append(_cc("group_G%d" % G, ("grouped", "G=%d" % G, "blocks=2"), G=G, n_img=2, rows=2 * G, R=19, D=516))
    out.append(_cc("group_R37", ("grouped", "third_loop"), G=2, n_img=2, rows=4, R=37))
    out.append(_cc("group_ad", ("grouped", "adaptive"), G=2, n_img=3, rows=6, R=128, counts=(65, 3, 128)))
    out.append(_cc("group_dead", ("grouped", "dead"), G=2, n_img=2, rows=4, R=19, live=0))
    return out


CTX_CASES = _ctx_cases()

_dac = _case("DalphaCase", "rows n_img R D ns counts img live", dict(rows=3, n_img=3, R=21, D=516, ns=3, counts=None, img=None, live=None))


def _dalpha_cases():
    out = []
    d_tags = {4: ("one_float4", "parts=1"), 512: ("parts=1", "full_block"), 516: ("parts=2", "block_of_one_float4"), 1028: ("parts=3",)}
    for D, tags in d_tags.items():
        out.append(_dac("D%d" % D, tags, D=D))
    for ns in (1, 3, 16):
        out.append(_dac("ns%d" % ns, ("ns=%d" % ns,), ns=ns, D=36))
    r_tags = {1: ("one_region",), 20: ("R=pass",), 21: ("second_pass",), 64: ("R=64", "fourth_pass")}
    for R, tags in r_tags.items():
        out.append(_dac("R%d" % R, tags, R=R))
    out.append(_dac("ad", ("adaptive", "counts_around_64"), rows=6, n_img=6, R=128, D=36, counts=AD_COUNTS))
    out.append(_dac("ad_D516", ("adaptive", "parts=2"), rows=3, n_img=3, R=128, counts=(65, 128, 21)))
    out.append(_dac("permuted", ("permuted_images", "unused_image"), rows=5, n_img=4, img=(2, 0, 2, 1, 0)))
    out.append(_dac("dead", ("dead",), live=0))
    return out


DALPHA_CASES = _dalpha_cases()

_ddc = _case("DdecCase", "rows n_img R A nparts mode counts img live",
             dict(rows=3, n_img=3, R=37, A=132, nparts=3, mode=0, counts=None, img=None, live=None))


def _ddec_cases():
    out = []
    a_tags = {4: ("one_float4",), 20: ("lt_keep_word",), 132: ("blocks=1",), 256: ("whole_strips", "blocks=1"), 1280: ("whole_strips", "blocks=5")}
    for A, tags in a_tags.items():
        for mode in (0, 1, 2):
            out.append(_ddc("A%d_mode%d" % (A, mode), tags + (("shared_words",) if mode == 2 and "whole_strips" in tags else ()), A=A, mode=mode))
    out.append(_ddc("nparts1", ("nparts=1",), nparts=1, mode=1))
    r_tags = {1: ("one_region",), 36: ("R=pass",), 37: ("second_pass",), 64: ("R=64", "second_pass")}
    for R, tags in r_tags.items():
        out.append(_ddc("R%d" % R, tags, R=R, A=256, mode=2))
    out.append(_ddc("ad_mask", ("adaptive", "dot_both_forms"), rows=4, n_img=4, R=128, counts=(64, 65, 128, 1), mode=1))
    out.append(_ddc("ad_philox", ("adaptive", "dot_both_forms", "shared_words"), rows=4, n_img=4, R=128, A=256, counts=(64, 65, 128, 1), mode=2))
    out.append(_ddc("permuted", ("permuted_images", "unused_image"), rows=5, n_img=4, img=(2, 0, 2, 1, 0), mode=1))
    out.append(_ddc("dead", ("dead",), mode=1, live=0))
    out.append(_ddc("dead_ad", ("dead", "adaptive"), rows=2, n_img=2, R=100, counts=(100, 7), mode=2, live=0))
    return out


DDEC_CASES = _ddec_cases()

# bs2: dec_all / ds_all hold 2 B rows per step and the pointers start at the second half
_dec = _case("DencCase", "B n_img R A T mode bs2 parts G counts img", dict(B=3, n_img=3, R=5, A=132, T=21, mode=2, bs2=False, parts=0, G=0, counts=None, img=None))


def _denc_cases():
    out = []
    t_tags = {1: ("one_step", "passes=1"), 20: ("T=TT", "passes=1"), 21: ("pass_of_one_step", "passes=2"), 41: ("passes=3",)}
    for G in (0, 2):
        g = "g_" if G else ""
        kw = dict(G=G, B=4, n_img=2) if G else {}
        for T, tags in t_tags.items():
            for mode in ((1, 2) if T in (21, 41) else (2,)):
                out.append(_dec(g + "T%d_mode%d" % (T, mode), tags + (("grouped",) if G else ()), T=T, mode=mode, **kw))
        a_tags = {4: ("one_float4",), 20: ("lt_keep_word",), 128: ("whole_strips",), 132: ("col_tail",), 1028: ("col_passes=2", "pass_of_one_float4"),
                  1280: ("col_passes=2", "whole_strips")}
        for A, tags in a_tags.items():
            for mode in (0, 1, 2):
                out.append(_dec(g + "A%d_mode%d" % (A, mode), tags + (("shared_words",) if mode == 2 and "whole_strips" in tags else ()) + (("grouped",) if G else ()),
                                A=A, mode=mode, **kw))
        out.append(_dec(g + "bs2", ("bs2",) + (("grouped",) if G else ()), bs2=True, mode=1, **kw))
        out.append(_dec(g + "parts1", ("parts=1",) + (("grouped",) if G else ()), parts=1, mode=1, R=7, **kw))
        out.append(_dec(g + "parts4", ("parts=4",) + (("grouped",) if G else ()), parts=4, mode=1, R=7, **kw))
    for G in (1, 5):
        out.append(_dec("g_G%d" % G, ("grouped", "G=%d" % G), G=G, B=2 * G, n_img=2, mode=1))
    out.append(_dec("ad", ("adaptive",), B=3, n_img=3, R=128, T=21, mode=1, counts=(65, 3, 128)))
    out.append(_dec("ad_philox", ("adaptive", "shared_words"), B=3, n_img=3, R=128, A=128, T=21, mode=2, counts=(65, 3, 128)))
    out.append(_dec("g_ad", ("adaptive", "grouped", "gparts>ATT_PARTS"), G=2, B=4, n_img=2, R=128, T=21, mode=1, counts=(65, 128)))
    out.append(_dec("g_ad_philox", ("adaptive", "grouped", "gparts>ATT_PARTS", "shared_words"), G=2, B=4, n_img=2, R=128, A=128, T=21, mode=2, counts=(3, 100)))
    out.append(_dec("permuted", ("permuted_images", "unused_image"), B=5, n_img=4, img=(2, 0, 2, 1, 0), mode=1))
    return out


DENC_CASES = _denc_cases()

MeanCase = collections.namedtuple("MeanCase", "name n_img R D counts")
MEAN_CASES = [MeanCase("R%d_D%d" % (R, D), 3, R, D, None) for R in (1, 36, 64) for D in (4, 516)] + \
             [MeanCase("counts_D%d" % D, 4, 64, D, (1, 36, 64, 17)) for D in (4, 516)] + [MeanCase("counts_R128", 3, 128, 1028, (128, 65, 2))]
SavedCase = collections.namedtuple("SavedCase", "name T B NH R")
SAVED_CASES = [SavedCase("NH%d_R%d" % (NH, R), 3, 2, NH, R) for NH in (1, 8) for R in (1, 36, 64)]


def _groups(R, parts, K):
    """passes of a wave of att_scores_kernel over the regions of its part: (part, wave) slots = 4 parts, NB regions per wave and pass"""
    return cdiv(cdiv(R, parts), 4 * K["NB"])


# tag -> predicate(case, K): what the tag claims, recomputed from the shape and the constants K
TAGS = {
    "one_float4": lambda c, K: getattr(c, "A", getattr(c, "D", 0)) == 4,
    "lt_keep_word": lambda c, K: c.A < 32,
    "tail_in_first_strip": lambda c, K: c.A < 256 and c.A % 256 != 0 and c.A > 128,
    "whole_strips": lambda c, K: c.A % (128 if type(c).__name__ == "DencCase" else 256) == 0,
    "shared_words": lambda c, K: c.mode == 2 and c.A % (128 if type(c).__name__ == "DencCase" else 256) == 0,
    "passes=1": lambda c, K: (cdiv(c.T, K["TT"]) if hasattr(c, "T") else cdiv(c.A, 1024)) == 1,
    "passes=2": lambda c, K: (cdiv(c.T, K["TT"]) if hasattr(c, "T") else cdiv(c.A, 1024)) == 2,
    "passes=3": lambda c, K: (cdiv(c.T, K["TT"]) if hasattr(c, "T") else cdiv(c.A, 1024)) == 3,
    "pass_of_one_float4": lambda c, K: c.A % 1024 == 4 and c.A > 1024,
    "col_tail": lambda c, K: c.A > 128 and c.A % 128 != 0 and c.A < 1024,
    "col_passes=2": lambda c, K: cdiv(c.A, 1024) == 2,
    "one_region": lambda c, K: c.R == 1,
    "R<=slots": lambda c, K: c.R < 4 * (c.parts or K["ATT_PARTS"]),
    "R=slots": lambda c, K: c.R == 4 * (c.parts or K["ATT_PARTS"]),
    "R>slots": lambda c, K: c.R > 4 * (c.parts or K["ATT_PARTS"]),
    "one_group": lambda c, K: _groups(c.R, c.parts or K["ATT_PARTS"], K) == 1,
    "R=group": lambda c, K: c.R == 4 * K["NB"] * (c.parts or K["ATT_PARTS"]),
    "two_groups": lambda c, K: _groups(c.R, c.parts or K["ATT_PARTS"], K) == 2,
    "R=64": lambda c, K: c.R == 64 and c.counts is None,
    "adaptive": lambda c, K: (c.counts is not None or c.R > 64) and c.R <= K["ATT_MAX_R"],
    "counts_around_64": lambda c, K: {63, 64, 65} <= set(c.counts),
    "counts_around_128": lambda c, K: {127, 128} <= set(c.counts) and K["ATT_MAX_R"] == 128,
    "nsplit=1": lambda c, K: c.nsplit == 1, "nsplit=5": lambda c, K: c.nsplit == 5,
    "parts=1": lambda c, K: (c.parts == 1) if hasattr(c, "parts") else cdiv(c.D, K["DALPHA_COLS"]) == 1,
    "parts=2": lambda c, K: cdiv(c.D, K["DALPHA_COLS"]) == 2, "parts=3": lambda c, K: cdiv(c.D, K["DALPHA_COLS"]) == 3,
    "parts=4": lambda c, K: c.parts == 4 and K["ATT_PARTS"] == 4, "parts=7": lambda c, K: c.parts == 7,
    "permuted_images": lambda c, K: c.img is not None and len(c.img) > c.n_img - 1 and list(c.img) != sorted(c.img) and len(set(c.img)) < len(c.img),
    "unused_image": lambda c, K: set(range(c.n_img)) - set(c.img) != set(),
    "row0": lambda c, K: 0 < c.row0 < c.rows and c.mode != 0,
    "dead": lambda c, K: c.live == 0, "live": lambda c, K: c.live == 1,
    "grouped": lambda c, K: (c.route in (1, 2) if hasattr(c, "route") else c.G >= 1) and (c.G <= K["ATT_CTX_MAX_G"] or hasattr(c, "T")),
    "G=1": lambda c, K: c.G == 1, "G=2": lambda c, K: c.G == 2, "G=5": lambda c, K: c.G == 5, "G=8": lambda c, K: c.G == 8 == K["ATT_CTX_MAX_G"],
    "blocks=1": lambda c, K: (cdiv(c.D, 512) if hasattr(c, "D") else cdiv(c.A, 256)) == 1,
    "blocks=2": lambda c, K: cdiv(c.D, 512) == 2, "blocks=3": lambda c, K: cdiv(c.D, 512) == 3,
    "blocks=5": lambda c, K: cdiv(c.A, 256) == 5,
    "full_block": lambda c, K: c.D == 512,
    "block_of_one_float4": lambda c, K: c.D % 512 == 4 and c.D > 512,
    "halves=1|0": lambda c, K: ((c.R + 1) // 2, c.R // 2) == (1, 0), "halves=1|1": lambda c, K: ((c.R + 1) // 2, c.R // 2) == (1, 1),
    "halves=10|9": lambda c, K: ((c.R + 1) // 2, c.R // 2) == (10, 9) and K["RB"] < 10 <= 2 * K["RB"],
    "halves=19|18": lambda c, K: ((c.R + 1) // 2, c.R // 2) == (19, 18) and 18 <= 2 * K["RB"] < 19,
    "second_batch": lambda c, K: K["RB"] < (c.R + 1) // 2 <= 2 * K["RB"],
    "third_loop": lambda c, K: (c.R + 1) // 2 > 2 * K["RB"],
    "alpha2": lambda c, K: c.alpha2 and ALPHA2_PAD > 0,
    "ns=1": lambda c, K: c.ns == 1, "ns=3": lambda c, K: c.ns == 3, "ns=16": lambda c, K: c.ns == 16,
    "R=pass": lambda c, K: c.R == 4 * (K["NR"] if hasattr(c, "D") else K["RB"]),
    "second_pass": lambda c, K: c.R > 4 * (K["NR"] if hasattr(c, "D") else K["RB"]),
    "fourth_pass": lambda c, K: cdiv(c.R, 4 * K["NR"]) == 4,
    "nparts=1": lambda c, K: c.nparts == 1,
    "dot_both_forms": lambda c, K: min(c.counts) <= 64 < max(c.counts),
    "one_step": lambda c, K: c.T == 1, "T=TT": lambda c, K: c.T == K["TT"], "pass_of_one_step": lambda c, K: c.T == K["TT"] + 1,
    "bs2": lambda c, K: c.bs2,
    "gparts>ATT_PARTS": lambda c, K: c.G >= 1 and cdiv(c.R, K["DENC_GROUP_REGS"]) > K["ATT_PARTS"] and K["ATT_PARTS"] * K["DENC_GROUP_REGS"] < c.R,
}
ALL_CASES = {"scores": SCORE_CASES, "ctx": CTX_CASES, "dalpha": DALPHA_CASES, "ddec": DDEC_CASES, "denc": DENC_CASES}
# what the issue's list asks of each table: (field, values) that must occur
REQUIRED = {
    "scores": [("A", (4, 20, 132, 256, 1028, 1280, 2304)), ("R", (1, 2, 16, 17, 48, 49, 64, 128)), ("nsplit", (1, 2, 5)), ("parts", (1, 4, 7)),
               ("G", (1, 2, 5, 8))],
    "ctx": [("D", (4, 36, 512, 516, 1028)), ("R", (1, 2, 19, 37, 64)), ("G", (1, 2, 5, 8))],
    "dalpha": [("D", (4, 512, 516, 1028)), ("ns", (1, 3, 16)), ("R", (1, 20, 21, 64))],
    "ddec": [("A", (4, 20, 132, 256, 1280)), ("nparts", (1, 3)), ("R", (1, 36, 37, 64)), ("mode", (0, 1, 2))],
    "denc": [("T", (1, 20, 21, 41)), ("A", (4, 20, 128, 132, 1028, 1280)), ("parts", (1, 4)), ("G", (1, 2, 5)), ("mode", (0, 1, 2))],
}


def images(c):
    """image of each row"""
    rows = c.B if hasattr(c, "B") else c.rows
    if c.img is not None:
        return list(c.img)
    G = getattr(c, "G", 0) or 1
    return [r // G for r in range(rows)]


def count_of(c, img):
    return c.R if c.counts is None else c.counts[img]


def ad_of(c):
    return c.counts is not None or c.R > 64


# ======================================================================================================================
# inputs: seeded, of the model's magnitudes (enc_ctx + dec_ctx of order 1 with both signs: about half of the relus are on).  Pad regions
# (r >= the image's count) and images no row refers to are NaN: a kernel has no business reading them.
def region_tensor(c, W, what, scale=0.8):
    """[n_img, R, W] fp32"""
    x = (seeded("%s %s %s" % (type(c).__name__, c.name, what)).standard_normal((c.n_img, c.R, W)) * scale).astype(np.float32)
    used = set(images(c))
    for i in range(c.n_img):
        x[i, count_of(c, i):] = NAN
        if i not in used:
            x[i] = NAN
    return x


def rand(c, what, shape, scale=1.0):
    return (seeded("%s %s %s" % (type(c).__name__, c.name, what)).standard_normal(shape) * scale).astype(np.float32)


def plant_zeros(c, enc, dec, rows):
    """exact zeros and -0.0 among the pre-activations enc[img, r, a] + dec[row, a], both of which must count as off: for the first row
    of each image enc = -dec in column 1 (+0.0) of its last valid region, and enc = dec = -0.0 in the last column of region 0 (-0.0; the
    column is -0.0 in every row of dec)."""
    A = enc.shape[2]
    dec[..., A - 1] = np.float32(-0.0)
    seen = set()
    for row, img in enumerate(images(c)[:rows]):
        if img in seen:
            continue
        seen.add(img)
        enc[img, 0, A - 1] = np.float32(-0.0)
        r = count_of(c, img) - 1
        src = dec[row] if dec.ndim == 2 else dec[0, row]
        enc[img, r, 1 % A] = -src[1 % A]
    return enc, dec


def keep3(mode, row0, rows, R, A, mask, step, stream=RNG_ATT):
    """[rows, R, A] int8: -1 passes unchanged, 0 dropped, 1 kept and doubled; element index ((row - row0) R + r) A + a"""
    return row_keep(mode, row0, rows, R * A, mask, SEED, stream, step).reshape(rows, R, A)


def mask_bytes(c, what, n):
    return seeded("%s %s mask %s" % (type(c).__name__, c.name, what)).choice(MASK_BYTES, size=n).astype(np.uint8)


def gain(keep):
    """1 where the element passes, 0 where dropped, 2 where kept"""
    return np.where(keep < 0, 1.0, np.where(keep > 0, 2.0, 0.0))


# ---- scores
def score_inputs(c):
    slab = rand(c, "slab", (c.nsplit, c.rows, c.A), 0.6)
    b_dec = rand(c, "b_dec", (c.A,), 0.3)
    slab[..., c.A - 1] = np.float32(-0.0)
    b_dec[c.A - 1] = np.float32(-0.0)
    dec = dec_ctx_twin(slab, b_dec)
    enc = region_tensor(c, c.A, "enc")
    enc, _ = plant_zeros(c, enc, dec.copy(), c.rows)
    w = rand(c, "w_aff", (c.A,), 0.3)
    b_aff = f32([0.37])
    n_drop = c.rows * c.R * c.A                       # (row r >= row0 takes the flags of row r - row0: the last row0 rows' are unused)
    mask = mask_bytes(c, "att", n_drop) if c.mode == 1 else None
    keep = keep3(c.mode, c.row0, c.rows, c.R, c.A, mask, STEP)
    return dict(slab=slab, b_dec=b_dec, dec=dec, enc=enc, w=w, b_aff=b_aff, mask=mask, keep=keep)


def dec_ctx_twin(slab, b_dec):
    """the kernel's bits: slab 0, then slabs 1 .. nsplit - 1 in order, then b_dec, fp32 additions"""
    s = slab[0].copy()
    for z in range(1, slab.shape[0]):
        s = (s + slab[z]).astype(np.float32)
    return (s + b_dec[None]).astype(np.float32)


def scores_ref(c, x):
    """scores [rows, R] float64 and bound; exact zeros behind the count"""
    val, bnd = np.zeros((c.rows, c.R)), np.zeros((c.rows, c.R))
    n_add = 16 * cdiv(c.A, 1024) + 6 + 1
    w, b = x["w"].astype(np.float64), float(x["b_aff"][0])
    for row, img in enumerate(images(c)):
        n = count_of(c, img)
        z = np.maximum(x["enc"][img, :n].astype(np.float64) + x["dec"][row].astype(np.float64)[None], 0.0)
        t = z * gain(x["keep"][row, :n]) * w[None]
        val[row, :n] = t.sum(1) + b
        bnd[row, :n] = SECOND * U * ((n_add + 2) * (np.abs(t).sum(1) + abs(b)) + 2 * np.abs(t).sum(1))
    return val, bnd


# ---- softmax and context
def ctx_inputs(c):
    feats = region_tensor(c, c.D, "feats", 1.0)
    scores = rand(c, "scores", (c.rows, c.R), 1.5)
    for row, img in enumerate(images(c)):
        scores[row, count_of(c, img):] = NAN           # the scores behind an image's count
    return dict(feats=feats, scores=scores)


def softmax_ref(s32):
    s = s32.astype(np.float64)
    e = np.exp(s - s.max())
    a = e / e.sum()
    return a, SECOND * U * a * (EXP_U + 9.0 + DIV_U + np.abs(s - s.max()))


def ctx_ref(c, x):
    """alpha [rows, R] (exact zeros behind the count; exactly 1 with one region) and ctx [rows, D], each with its bound"""
    al, alb = np.zeros((c.rows, c.R)), np.zeros((c.rows, c.R))
    cx, cxb = np.zeros((c.rows, c.D)), np.zeros((c.rows, c.D))
    for row, img in enumerate(images(c)):
        n = count_of(c, img)
        a, ab = softmax_ref(x["scores"][row, :n])
        if n == 1:
            a, ab = np.ones(1), np.zeros(1)
        al[row, :n], alb[row, :n] = a, ab
        f = x["feats"][img, :n].astype(np.float64)
        t = a[:, None] * f
        cx[row] = t.sum(0)
        cxb[row] = SECOND * ((ab[:, None] * np.abs(f)).sum(0) + U * (cdiv(n, 2) + 1 + 2 + 1) * np.abs(t).sum(0))
    return al, alb, cx, cxb


# ---- mean and saved alphas
def mean_inputs(c):
    x = (seeded("mean " + c.name).standard_normal((c.n_img, c.R, c.D))).astype(np.float32)
    if c.counts is not None:
        for i, n in enumerate(c.counts):
            x[i, n:] = NAN
    return x


def mean_ref(c, feats):
    val, bnd = np.zeros((c.n_img, c.D)), np.zeros((c.n_img, c.D))
    for i in range(c.n_img):
        n = c.R if c.counts is None else c.counts[i]
        f = feats[i, :n].astype(np.float64)
        val[i] = f.sum(0) / n
        bnd[i] = SECOND * U * ((n + 2) * np.abs(f).sum(0) / n + DIV_U * np.abs(val[i]))
    return val, bnd


def saved_alphas_twin(src):
    """[T, B, NH, R] -> [B, T, R], the fp32 mean over the heads added in head order: the kernel's bits"""
    T, B, NH, R = src.shape
    s = np.zeros((T, B, R), dtype=np.float32)
    for h in range(NH):
        s = (s + src[:, :, h]).astype(np.float32)
    return np.ascontiguousarray((s / np.float32(NH)).astype(np.float32).transpose(1, 0, 2))


# ---- d alpha
def dalpha_inputs(c):
    ldc = c.D + DCTX_PAD
    slab = rand(c, "dctx", (c.ns, c.rows, ldc), 0.5)
    slab[..., c.D:] = NAN
    return dict(slab=slab, feats=region_tensor(c, c.D, "feats", 1.0), ldc=ldc)


def dalpha_ref(c, x, K=CONST):
    """dalpha_part [rows, parts, R] with its bound and `written` (False behind the count: the kernel leaves those alone)"""
    P = cdiv(c.D, K["DALPHA_COLS"])
    val, bnd, wr = np.zeros((c.rows, P, c.R)), np.zeros((c.rows, P, c.R)), np.zeros((c.rows, P, c.R), dtype=bool)
    s = x["slab"][:, :, :c.D].astype(np.float64)
    g, gb = s.sum(0), (c.ns + 1) * U * np.abs(s).sum(0)
    for row, img in enumerate(images(c)):
        n = count_of(c, img)
        f = x["feats"][img, :n].astype(np.float64)
        for p in range(P):
            cols = slice(p * K["DALPHA_COLS"], min(c.D, (p + 1) * K["DALPHA_COLS"]))
            t = f[:, cols] * g[row, cols][None]
            val[row, p, :n] = t.sum(1)
            bnd[row, p, :n] = SECOND * ((np.abs(f[:, cols]) * gb[row, cols][None]).sum(1) + U * (8 + 6 + 2 + 1) * np.abs(t).sum(1))
            wr[row, p, :n] = True
    return val, bnd, wr


# ---- d dec
def ddec_inputs(c):
    dec = rand(c, "dec", (c.rows, c.A), 0.8)
    enc = region_tensor(c, c.A, "enc")
    enc, dec = plant_zeros(c, enc, dec, c.rows)
    alpha = np.zeros((c.rows, c.R), dtype=np.float32)
    parts = rand(c, "dalpha", (c.rows, c.nparts, c.R), 1.0)
    for row, img in enumerate(images(c)):
        n = count_of(c, img)
        a = np.exp(rand(c, "al%d" % row, (n,), 1.5).astype(np.float64))
        alpha[row, :n] = (a / a.sum()).astype(np.float32)
        if n == 1:
            alpha[row, 0] = 1.0
        alpha[row, n:] = NAN
        parts[row, :, n:] = NAN                        # dalpha_part behind the count is neither written nor read
    mask = mask_bytes(c, "att", c.rows * c.R * c.A) if c.mode == 1 else None
    return dict(enc=enc, dec=dec, w=rand(c, "w_aff", (c.A,), 0.3), alpha=alpha, parts=parts, mask=mask,
                keep=keep3(c.mode, 0, c.rows, c.R, c.A, mask, STEP))


def on_bits(enc_rows, dec_row, keep):
    """relu and keep of [n, A] elements: the fp32 sum of the two given fp32 numbers is > 0 (+0.0 and -0.0 are off) and the element is kept.
    -> (on, zp): zp the fp32 sum"""
    zp = (enc_rows + dec_row[None]).astype(np.float32)
    return (zp > np.float32(0)) & (keep != 0), zp


def ds_ref(alpha, parts):
    """ds [n] and bound from alpha [n] fp32 and the dalpha parts [nparts, n] fp32; exactly 0 with one region (alpha = 1)"""
    a, p = alpha.astype(np.float64), parts.astype(np.float64)
    npar = parts.shape[0]
    da, dab = p.sum(0), (npar + 1) * U * np.abs(p).sum(0) * (npar > 1)
    dot = (a * da).sum()
    dotb = (a * dab).sum() + (7 + 2 + 1) * U * np.abs(a * da).sum()
    ds = a * (da - dot)
    dsb = SECOND * (a * (dab + dotb + U * np.abs(da - dot)) + U * np.abs(ds))
    if len(a) == 1:
        ds, dsb = np.zeros(1), np.zeros(1)
    return ds, dsb


def ddec_ref(c, x):
    """ds [rows, R] (zeros behind the count) and ddec [rows, A], each with its bound"""
    ds, dsb = np.zeros((c.rows, c.R)), np.zeros((c.rows, c.R))
    dd, ddb = np.zeros((c.rows, c.A)), np.zeros((c.rows, c.A))
    w = np.abs(x["w"].astype(np.float64))
    for row, img in enumerate(images(c)):
        n = count_of(c, img)
        ds[row, :n], dsb[row, :n] = ds_ref(x["alpha"][row, :n], x["parts"][row, :, :n])
        on, _ = on_bits(x["enc"][img, :n], x["dec"][row], x["keep"][row, :n])
        sc = 2.0 if c.mode else 1.0
        t = on * ds[row, :n, None] * x["w"].astype(np.float64)[None] * sc
        dd[row] = t.sum(0)
        ddb[row] = SECOND * ((on * dsb[row, :n, None] * w[None] * sc).sum(0) + U * (cdiv(n, 4) + 3 + 2 + 1) * np.abs(t).sum(0))
    return ds, dsb, dd, ddb


# ---- d enc_ctx
def denc_inputs(c):
    Bs = 2 * c.B if c.bs2 else c.B
    dec_all = rand(c, "dec", (c.T, Bs, c.A), 0.8)
    ds_all = rand(c, "ds", (c.T, Bs, c.R), 0.1)
    if c.R > 2:
        ds_all[:, :, 0] = 0.0                           # some exact zeros among the ds
    off = c.B if c.bs2 else 0
    dec_all[:, :off] = NAN                              # the first half of a merged chain's rows: not this launch's
    ds_all[:, :off] = NAN
    enc = region_tensor(c, c.A, "enc")
    dv = dec_all[:, off:off + c.B]
    enc, dv = plant_zeros(c, enc, dv, c.B)
    dec_all[:, off:off + c.B] = dv
    for row, img in enumerate(images(c)):
        ds_all[:, off + row, count_of(c, img):] = 0.0  # what att_bwd_ddec_kernel writes behind the count
    n = c.B * c.R * c.A
    mask = np.stack([mask_bytes(c, "t%d" % t, n) for t in range(c.T)]) if c.mode == 1 else None
    keep = np.stack([keep3(c.mode, 0, c.B, c.R, c.A, None if mask is None else mask[t], t) for t in range(c.T)])
    return dict(enc=enc, dec_all=dec_all, ds_all=ds_all, w=rand(c, "w_aff", (c.A,), 0.3), mask=mask, keep=keep, Bs=Bs, off=off)


def denc_parts(c, K=CONST):
    if c.parts:
        return c.parts
    if c.G:
        return K["ATT_PARTS"] if K["ATT_PARTS"] * K["DENC_GROUP_REGS"] >= c.R else cdiv(c.R, K["DENC_GROUP_REGS"])
    return K["ATT_PARTS"]


def denc_ref(c, x, parts):
    """per row: denc [B, R, A] (zeros behind the count) and dwaff_part [B, parts, A], each with its bound"""
    de, deb = np.zeros((c.B, c.R, c.A)), np.zeros((c.B, c.R, c.A))
    dw, dwb = np.zeros((c.B, parts, c.A)), np.zeros((c.B, parts, c.A))
    sc = 2.0 if c.mode else 1.0
    w = x["w"].astype(np.float64)
    for row, img in enumerate(images(c)):
        n = count_of(c, img)
        te, tw = np.zeros((n, c.A)), np.zeros((n, c.A))
        ae, aw = np.zeros((n, c.A)), np.zeros((n, c.A))
        for t in range(c.T):
            on, zp = on_bits(x["enc"][img, :n], x["dec_all"][t, x["off"] + row], x["keep"][t, row, :n])
            ds = x["ds_all"][t, x["off"] + row, :n].astype(np.float64)[:, None]
            e, v = on * ds * w[None] * sc, on * zp.astype(np.float64) * sc * ds
            te, tw, ae, aw = te + e, tw + v, ae + np.abs(e), aw + np.abs(v)
        de[row, :n], deb[row, :n] = te, SECOND * U * (c.T + 2 + 1) * ae
        for p in range(parts):
            nr = len(range(p, n, parts))
            dw[row, p] = tw[p::parts].sum(0)
            dwb[row, p] = SECOND * U * (nr * c.T + 2 + 1) * aw[p::parts].sum(0)
    return de, deb, dw, dwb


def group_fold(val, bnd, G):
    """the G rows of an image added in k order: [n_img G, ...] -> [n_img, ...]; G more additions over the rows' sums"""
    v = val.reshape((-1, G) + val.shape[1:])
    b = bnd.reshape((-1, G) + bnd.shape[1:])
    return v.sum(1), b.sum(1) + SECOND * U * (G + 1) * np.abs(v).sum(1)
