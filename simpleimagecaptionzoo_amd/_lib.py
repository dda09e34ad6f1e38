"""ctypes binding of libicz.so (the C ABI declared in include/icz.h).

The HIP library is the product: there is no CPU or eager-PyTorch fallback.  Loading fails loudly if the
shared object is missing (build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C simpleimagecaptionzoo_amd/csrc`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libicz.so")


class IczError(RuntimeError):
    pass


GRAD_READY_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int32)       # icz_grad_ready_cb


class ButdDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("R", "D", "H", "E", "A", "V", "max_rows", "max_len")]


BUTD_PARAM_FIELDS = (
    "embed_weight",
    "td_w_ih", "td_w_hh", "td_b_ih", "td_b_hh",
    "lm_w_ih", "lm_w_hh", "lm_b_ih", "lm_b_hh",
    "enc_att_v", "enc_att_g", "enc_att_b",
    "dec_att_v", "dec_att_g", "dec_att_b",
    "affine_v", "affine_g", "affine_b",
    "predict_v", "predict_g", "predict_b",
)
# reference state_dict key (without the "decoder." prefix) of each field, Models/BUTD_Model.py:75-84
BUTD_PARAM_KEYS = (
    "embed.0.weight",
    "TD_atten.weight_ih", "TD_atten.weight_hh", "TD_atten.bias_ih", "TD_atten.bias_hh",
    "language_model.weight_ih", "language_model.weight_hh", "language_model.bias_ih", "language_model.bias_hh",
    "atten.enc_att.weight_v", "atten.enc_att.weight_g", "atten.enc_att.bias",
    "atten.dec_att.weight_v", "atten.dec_att.weight_g", "atten.dec_att.bias",
    "atten.affine.weight_v", "atten.affine.weight_g", "atten.affine.bias",
    "predict.weight_v", "predict.weight_g", "predict.bias",
)


class NicDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("E", "H", "V", "max_rows", "max_len")]


NIC_PARAM_FIELDS = ("embed_weight", "w_ih", "w_hh", "b_ih", "b_hh", "predict_v", "predict_g", "predict_b")
# reference state_dict keys of Models/NIC_Model.py DecoderRNN (:47-49)
NIC_PARAM_KEYS = ("embed.weight", "lstm.weight_ih", "lstm.weight_hh", "lstm.bias_ih", "lstm.bias_hh",
                  "predict.weight_v", "predict.weight_g", "predict.bias")


class AoaDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("R", "D", "Hd", "E", "V", "NH", "max_rows", "max_len")]


def _aoa_block_keys(block, norm):
    return tuple(block + n for n in ("linear_Q.weight", "linear_Q.bias", "linear_K.weight", "linear_K.bias", "linear_V.weight",
                                     "linear_V.bias", "aoa_module.0.weight", "aoa_module.0.bias")) + (norm + "gain", norm + "bias")


# reference state_dict keys of AoADetection_Captioner (Models/AoA_Model.py:657-667) in the pointer order of icz_aoa_params
AOA_PARAM_KEYS = (("img_feats_porjection.0.weight", "img_feats_porjection.0.bias")
                  + sum((_aoa_block_keys("aoa_refine.aoa_layers.%d.aoa_block." % l, "aoa_refine.aoa_layers.%d.sublayer.norm." % l)
                         for l in range(6)), ())
                  + ("aoa_refine.norm.gain", "aoa_refine.norm.bias",
                     "decoder.lstm.weight_ih", "decoder.lstm.weight_hh", "decoder.lstm.bias_ih", "decoder.lstm.bias_hh")
                  + _aoa_block_keys("decoder.aoa_block.", "decoder.h_norm.")
                  + ("decoder.embed.0.weight", "decoder.predict.weight_v", "decoder.predict.weight_g", "decoder.predict.bias"))
AOA_DECODER_KEYS = tuple(k for k in AOA_PARAM_KEYS if k.startswith("decoder."))


class AoaParams(C.Structure):      # icz_aoa_params is 82 pointers with no padding: addressed here as a flat table
    _fields_ = [("p%d" % i, C.c_void_p) for i in range(len(AOA_PARAM_KEYS))]


class AoaRng(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("uniforms", C.c_void_p)] + [(n, C.c_void_p) for n in (
        "proj_mask", "ref_att_mask", "ref_aoa_mask", "ref_sc_mask", "emb_mask", "ctx_mask", "att_mask", "out_mask")]


class NicParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in NIC_PARAM_FIELDS]


class ButdParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in BUTD_PARAM_FIELDS]


class Rng(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("uniforms", C.c_void_p), ("emb_mask", C.c_void_p),
                ("att_mask", C.c_void_p), ("out_mask", C.c_void_p)]


class BeamOpts(C.Structure):       # icz_beam_opts
    _fields_ = [("n_best", C.c_int32), ("block_ngram", C.c_int32), ("lp_kind", C.c_int32), ("lp_alpha", C.c_float)]


class BeamDiversity(C.Structure):  # icz_beam_diversity
    _fields_ = [("groups", C.c_int32), ("diversity", C.c_float)]


BEAM_STEP_FIELDS = ("logits", "n_act", "run", "seqs_in", "seqs_out", "src_row", "it_next", "best_score", "best_len", "best_seq",
                    "has_complete", "n_live", "hyp_seq", "hyp_score", "hyp_len", "hyp_cnt", "cand_val", "cand_idx")


class BeamStepState(C.Structure):  # icz_beam_step_state
    _fields_ = [(n, C.c_void_p) for n in BEAM_STEP_FIELDS]


class BeamConstraints(C.Structure):  # icz_beam_constraints
    _fields_ = [("max_constraints", C.c_int32), ("max_alts", C.c_int32), ("words_dev", C.c_void_p), ("words_host", C.c_void_p)]


BEAM_CONSTRAINED_FIELDS = ("logits", "words", "n_act", "cap", "run", "seqs_in", "seqs_out", "src_row", "it_next", "n_live", "hyp_seq",
                           "hyp_score", "hyp_len", "hyp_state", "hyp_cnt", "cand_val", "cand_idx", "force_val")


class BeamConstrainedState(C.Structure):  # icz_beam_constrained_state
    _fields_ = [(n, C.c_void_p) for n in BEAM_CONSTRAINED_FIELDS]


class SampleSelectArgs(C.Structure):   # icz_sample_select_args
    _fields_ = [("logits", C.c_void_p), ("V", C.c_int32), ("ldl", C.c_int32), ("ns", C.c_int32), ("slab_stride", C.c_int64),
                ("bias", C.c_void_p), ("logits_store", C.c_void_p), ("uniforms", C.c_void_p), ("seed", C.c_void_p), ("t", C.c_int32),
                ("T", C.c_int32), ("unfinished", C.c_void_p), ("n_unfinished", C.c_void_p), ("seq_out", C.c_void_p), ("logp_out", C.c_void_p),
                ("it_next", C.c_void_p), ("draw_out", C.c_void_p), ("lse_out", C.c_void_p), ("emb_table", C.c_void_p), ("emb_next", C.c_void_p),
                ("E", C.c_int32), ("emb_mode", C.c_int32), ("emb_mask", C.c_void_p), ("live_rows", C.c_void_p), ("row0", C.c_int32),
                ("ids_out", C.c_void_p), ("g_unfinished", C.c_void_p), ("n_any", C.c_void_p)]


class SampleOpts(C.Structure):     # icz_sample_opts
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float)]


class SampleDistinctOut(C.Structure):  # icz_sample_distinct_out
    _fields_ = [(n, C.c_void_p) for n in ("ids", "lens", "finished", "phi", "g")]


SBS_STEP_FIELDS = ("logits", "bias", "uniforms", "occ", "frozen", "phi", "G", "len", "seqs_in", "seqs_out", "src_row", "it_next", "n_live",
                   "cand_g", "cand_phi", "cand_idx")


class SbsStepState(C.Structure):   # icz_sbs_step_state
    _fields_ = [(n, C.c_void_p) for n in SBS_STEP_FIELDS]


class DistillOpts(C.Structure):    # icz_distill_opts
    _fields_ = [("M", C.c_int32), ("teacher", C.POINTER(C.c_void_p)), ("ld", C.POINTER(C.c_int32)), ("weights", C.POINTER(C.c_float)),
                ("alpha", C.c_float), ("temperature", C.c_float), ("smoothing", C.c_float)]


class ScstObjective(C.Structure):  # icz_scst_objective
    _fields_ = [("kind", C.c_int32), ("K", C.c_int32), ("risk_alpha", C.c_float), ("entropy_weight", C.c_float), ("n_img_global", C.c_float),
                ("reward", C.c_void_p), ("scores", C.c_void_p)]


class SworOpts(C.Structure):       # icz_swor_opts
    _fields_ = [("n", C.c_int32), ("estimator", C.c_int32), ("n_img_global", C.c_float), ("phi", C.c_void_p), ("G", C.c_void_p),
                ("scores", C.c_void_p), ("perm", C.c_void_p), ("stats_out", C.c_void_p)]


class DropPArgs(C.Structure):      # icz_test_dropp
    _fields_ = [("mode", C.c_int32), ("mask", C.c_void_p), ("seed", C.c_void_p), ("stream", C.c_uint32), ("step", C.c_uint32),
                ("p", C.c_float), ("idx0", C.c_uint64)]


class DropArgs(C.Structure):       # icz_test_drop
    _fields_ = [("mode", C.c_int32), ("mask", C.c_void_p), ("seed", C.c_void_p), ("stream", C.c_uint32), ("step", C.c_uint32),
                ("row0", C.c_int32)]


LSTM_POINT_POINTERS = ("slab", "pre", "pre_row", "b_ih", "b_hh", "c_prev", "h_out", "c_out", "gates_out", "hdrop_out", "live")


class LstmPointArgs(C.Structure):  # icz_test_lstm_point_args
    _fields_ = [("slab", C.c_void_p), ("ns", C.c_int32), ("pre", C.c_void_p), ("n_pre", C.c_int32), ("pre_row", C.c_void_p),
                ("b_ih", C.c_void_p), ("b_hh", C.c_void_p), ("c_prev", C.c_void_p), ("h_out", C.c_void_p), ("c_out", C.c_void_p),
                ("gates_out", C.c_void_p), ("hdrop_out", C.c_void_p), ("rows", C.c_int32), ("H", C.c_int32), ("live", C.c_void_p)]


LSTM_BWD_POINTERS = ("dh_a", "dh_b", "dh_c", "dhdrop", "dc_in", "gates", "c_prev", "c_cur", "dgates", "dc_prev", "live", "carry_live")


class LstmBwdArgs(C.Structure):    # icz_test_lstm_bwd_args
    _fields_ = [("dh_a", C.c_void_p), ("ns_a", C.c_int32), ("lda_a", C.c_int32), ("rows_a", C.c_int32),
                ("dh_b", C.c_void_p), ("ns_b", C.c_int32), ("lda_b", C.c_int32), ("rows_b", C.c_int32),
                ("dh_c", C.c_void_p), ("ns_c", C.c_int32), ("lda_c", C.c_int32), ("rows_c", C.c_int32),
                ("dhdrop", C.c_void_p), ("dc_in", C.c_void_p), ("dc_in_rows", C.c_int32), ("gates", C.c_void_p), ("c_prev", C.c_void_p),
                ("c_cur", C.c_void_p), ("dgates", C.c_void_p), ("dc_prev", C.c_void_p), ("rows", C.c_int32), ("H", C.c_int32),
                ("live", C.c_void_p), ("carry_live", C.c_void_p)]


ATT_SCORES_POINTERS = ("enc_ctx", "img_of_row", "dec_slab", "b_dec", "w_aff", "b_aff", "dec_ctx_out", "scores", "live", "counts")


class AttScoresArgs(C.Structure):  # icz_test_att_scores_args
    _fields_ = [("enc_ctx", C.c_void_p), ("n_img", C.c_int32), ("img_of_row", C.c_void_p), ("dec_slab", C.c_void_p), ("nsplit", C.c_int32),
                ("b_dec", C.c_void_p), ("w_aff", C.c_void_p), ("b_aff", C.c_void_p), ("dec_ctx_out", C.c_void_p), ("scores", C.c_void_p),
                ("rows", C.c_int32), ("R", C.c_int32), ("A", C.c_int32), ("live", C.c_void_p), ("counts", C.c_void_p)]


ATT_DDEC_POINTERS = ("enc_ctx", "dec_ctx", "w_aff", "alpha", "dalpha", "ddec", "ds_out", "live", "img_of_row", "counts")


class AttDdecArgs(C.Structure):    # icz_test_att_ddec_args
    _fields_ = [("enc_ctx", C.c_void_p), ("n_img", C.c_int32), ("dec_ctx", C.c_void_p), ("w_aff", C.c_void_p), ("alpha", C.c_void_p),
                ("dalpha", C.c_void_p), ("ddec", C.c_void_p), ("ds_out", C.c_void_p), ("rows", C.c_int32), ("R", C.c_int32), ("A", C.c_int32),
                ("nparts", C.c_int32), ("live", C.c_void_p), ("img_of_row", C.c_void_p), ("counts", C.c_void_p)]


ATT_DENC_POINTERS = ("enc_ctx", "dec_all", "ds_all", "w_aff", "denc", "dwaff_part", "mask", "seed", "img_of_row", "counts")


class AttDencArgs(C.Structure):    # icz_test_att_denc_args
    _fields_ = [("enc_ctx", C.c_void_p), ("n_img", C.c_int32), ("dec_all", C.c_void_p), ("ds_all", C.c_void_p), ("w_aff", C.c_void_p),
                ("denc", C.c_void_p), ("dwaff_part", C.c_void_p), ("B", C.c_int32), ("R", C.c_int32), ("A", C.c_int32), ("T", C.c_int32),
                ("mode", C.c_int32), ("mask", C.c_void_p), ("mask_step", C.c_int64), ("seed", C.c_void_p), ("stream", C.c_uint32),
                ("Bs", C.c_int32), ("img_of_row", C.c_void_p), ("counts", C.c_void_p)]


_lib = None


def lib():
    """Load libicz.so once; raise IczError (never fall back) if it is missing or lacks a symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IczError("libicz.so not found at %s -- the HIP extension is required (no fallback); run "
                       "__graft_entry__.build()" % LIB_PATH)
    # torch first: its wheel carries its own libamdhip64.so, and libicz.so (linked against the same soname) must bind to THAT runtime --
    # loaded the other way round the process holds two HIP runtimes and the second one finds no device ("no ROCm-capable device is
    # detected" from the first hipMalloc; seen with __graft_entry__.build() followed by smoke() in one process)
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    sig = {
        "icz_last_error": (C.c_char_p, []),
        "icz_version": (C.c_char_p, []),
        "icz_butd_create": (C.c_int, [C.POINTER(ButdDims), C.POINTER(vp)]),
        "icz_butd_create_regions": (C.c_int, [C.POINTER(ButdDims), C.POINTER(vp)]),
        "icz_butd_destroy": (C.c_int, [vp]),
        "icz_butd_bind_params": (C.c_int, [vp, C.POINTER(ButdParams)]),
        "icz_butd_set_option": (C.c_int, [vp, C.c_char_p, i32]),
        "icz_butd_set_grad_callback": (C.c_int, [vp, GRAD_READY_CB, vp]),
        "icz_aoa_set_grad_callback": (C.c_int, [vp, GRAD_READY_CB, vp]),
        "icz_butd_set_mask_sum_global": (C.c_int, [vp, vp, vp]),
        "icz_butd_refresh_weights": (C.c_int, [vp, vp]),
        "icz_butd_set_regions": (C.c_int, [vp, i32, vp, vp, i32]),
        "icz_butd_greedy": (C.c_int, [vp, vp, i32, i32, vp, vp, vp]),
        "icz_butd_step": (C.c_int, [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "icz_butd_sample": (C.c_int, [vp, vp, i32, i32, C.POINTER(Rng), vp, vp, vp]),
        "icz_butd_scst_rollouts": (C.c_int, [vp, vp, i32, i32, C.POINTER(Rng), vp, vp, vp, vp]),
        "icz_butd_sample_n": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(Rng), vp, vp, vp]),
        "icz_butd_sample_backward": (C.c_int, [vp, vp, C.POINTER(ButdParams), vp, vp, f32, vp]),
        "icz_butd_sample_backward_dlogp": (C.c_int, [vp, vp, C.POINTER(ButdParams), vp]),
        "icz_butd_xe_backward_dlogits": (C.c_int, [vp, vp, C.POINTER(ButdParams), vp]),
        "icz_butd_beam_search": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp]),
        "icz_butd_beam_search_opts": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(BeamOpts), vp, vp, vp, vp]),
        "icz_butd_beam_search_diverse": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(BeamOpts), C.POINTER(BeamDiversity), vp, vp, vp, vp]),
        "icz_butd_beam_search_constrained": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(BeamOpts), C.POINTER(BeamConstraints), vp, vp, vp, vp, vp]),
        "icz_butd_sample_mask_sum": (C.c_int, [vp, vp, vp]),
        "icz_butd_xe_forward": (C.c_int, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(Rng), i32, vp, vp]),
        "icz_butd_xe_backward": (C.c_int, [vp, f32, C.POINTER(ButdParams), vp, f32, vp]),
        "icz_butd_xe_forward_n": (C.c_int, [vp, vp, vp, i32, i32, i32, C.POINTER(i32), C.POINTER(Rng), i32, vp, vp]),
        "icz_butd_set_scheduled_sampling": (C.c_int, [vp, f32, vp, vp]),
        "icz_nic_set_scheduled_sampling": (C.c_int, [vp, f32, vp, vp]),
        "icz_aoa_set_scheduled_sampling": (C.c_int, [vp, f32, vp, vp]),
        "icz_adam_clamp_step": (C.c_int, [vp, vp, vp, vp, i64, f32, f32, i32, vp]),
        "icz_nic_create": (C.c_int, [C.POINTER(NicDims), C.POINTER(vp)]),
        "icz_nic_destroy": (C.c_int, [vp]),
        "icz_nic_bind_params": (C.c_int, [vp, C.POINTER(NicParams)]),
        "icz_nic_refresh_weights": (C.c_int, [vp, vp]),
        "icz_nic_greedy": (C.c_int, [vp, vp, i32, i32, vp, vp]),
        "icz_nic_sample": (C.c_int, [vp, vp, i32, i32, C.POINTER(Rng), vp, vp, vp]),
        "icz_nic_sample_n": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(Rng), vp, vp, vp]),
        "icz_nic_sample_backward": (C.c_int, [vp, vp, C.POINTER(NicParams), vp, vp, vp, f32, vp]),
        "icz_nic_xe_forward": (C.c_int, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(Rng), i32, vp, vp]),
        "icz_nic_xe_backward": (C.c_int, [vp, f32, C.POINTER(NicParams), vp, vp, f32, vp]),
        "icz_butd_saved_alphas": (C.c_int, [vp, vp, vp]),
        "icz_aoa_saved_alphas": (C.c_int, [vp, vp, vp]),
        "icz_nic_set_norm_global": (C.c_int, [vp, vp, vp]),
        "icz_aoa_set_norm_global": (C.c_int, [vp, vp, vp]),
        "icz_nic_beam_search": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp]),
        "icz_nic_beam_search_opts": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(BeamOpts), vp, vp, vp, vp]),
        "icz_nic_beam_search_diverse": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(BeamOpts), C.POINTER(BeamDiversity), vp, vp, vp, vp]),
        "icz_nic_beam_search_constrained": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(BeamOpts), C.POINTER(BeamConstraints), vp, vp, vp, vp, vp]),
        "icz_aoa_create": (C.c_int, [C.POINTER(AoaDims), C.POINTER(vp)]),
        "icz_aoa_destroy": (C.c_int, [vp]),
        "icz_aoa_bind_params": (C.c_int, [vp, C.POINTER(AoaParams)]),
        "icz_aoa_refresh_weights": (C.c_int, [vp, vp]),
        "icz_aoa_set_regions": (C.c_int, [vp, i32, vp, vp, i32]),
        "icz_aoa_set_option": (C.c_int, [vp, C.c_char_p, i32]),
        "icz_nic_set_option": (C.c_int, [vp, C.c_char_p, i32]),
        "icz_aoa_refine": (C.c_int, [vp, vp, i32, vp, vp]),
        "icz_aoa_greedy": (C.c_int, [vp, vp, i32, i32, vp, vp]),
        "icz_aoa_beam_search": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp]),
        "icz_aoa_beam_search_opts": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(BeamOpts), vp, vp, vp, vp]),
        "icz_aoa_beam_search_diverse": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(BeamOpts), C.POINTER(BeamDiversity), vp, vp, vp, vp]),
        "icz_aoa_beam_search_constrained": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(BeamOpts), C.POINTER(BeamConstraints), vp, vp, vp, vp, vp]),
        "icz_ensemble_create": (C.c_int, [C.POINTER(i32), C.POINTER(vp), C.POINTER(f32), i32, C.POINTER(vp)]),
        "icz_ensemble_destroy": (C.c_int, [vp]),
        "icz_ensemble_greedy": (C.c_int, [vp, C.POINTER(vp), i32, i32, vp, vp]),
        "icz_ensemble_beam_search_diverse": (C.c_int, [vp, C.POINTER(vp), i32, i32, i32, C.POINTER(BeamOpts), C.POINTER(BeamDiversity), vp, vp,
                                                       vp, vp]),
        "icz_ensemble_beam_search_constrained": (C.c_int, [vp, C.POINTER(vp), i32, i32, i32, C.POINTER(BeamOpts), C.POINTER(BeamConstraints), vp,
                                                           vp, vp, vp, vp]),
        "icz_ensemble_logprob": (C.c_int, [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(f32), i32, i32, vp, i32,
                                           vp, vp]),
        "icz_ensemble_sample_decode": (C.c_int, [vp, C.POINTER(vp), i32, i32, i32, C.POINTER(SampleOpts), C.c_uint64, vp, vp, vp, vp, vp]),
        "icz_ensemble_sample_filter_draw": (C.c_int, [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(f32), i32, i32,
                                                      C.POINTER(SampleOpts), vp, vp, vp, vp, vp]),
        "icz_sample_decode_check": (C.c_int, [C.POINTER(SampleOpts), i32, i32, i32, i32]),
        "icz_butd_sample_decode": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(SampleOpts), C.c_uint64, vp, vp, vp, vp, vp]),
        "icz_aoa_sample_decode": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(SampleOpts), C.c_uint64, vp, vp, vp, vp, vp]),
        "icz_nic_sample_decode": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(SampleOpts), C.c_uint64, vp, vp, vp, vp, vp]),
        "icz_sample_filter_draw": (C.c_int, [vp, vp, i32, i32, i32, i32, C.POINTER(SampleOpts), vp, vp, vp, vp, vp]),
        "icz_sample_distinct_check": (C.c_int, [i32, i32, i32, f32, i32, i32]),
        "icz_butd_sample_distinct": (C.c_int, [vp, vp, i32, i32, i32, f32, C.c_uint64, i32, vp, vp, C.POINTER(SampleDistinctOut), vp]),
        "icz_aoa_sample_distinct": (C.c_int, [vp, vp, i32, i32, i32, f32, C.c_uint64, i32, vp, vp, C.POINTER(SampleDistinctOut), vp]),
        "icz_nic_sample_distinct": (C.c_int, [vp, vp, i32, i32, i32, f32, C.c_uint64, i32, vp, vp, C.POINTER(SampleDistinctOut), vp]),
        "icz_ensemble_sample_distinct": (C.c_int, [vp, C.POINTER(vp), i32, i32, i32, f32, C.c_uint64, i32, vp, vp, C.POINTER(SampleDistinctOut), vp]),
        "icz_test_sbs_rowtopk": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, C.c_uint64, i32, vp, vp, vp, vp]),
        "icz_test_sbs_step": (C.c_int, [C.POINTER(SbsStepState), i32, i32, i32, i32, i32, i32, i32, i32, f32, C.c_uint64, i32, vp]),
        "icz_test_sbs_init": (C.c_int, [i32, i32, vp, C.c_uint64, i32] + [vp] * 9),
        "icz_test_sbs_finalize": (C.c_int, [i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(SampleDistinctOut), vp]),
        "icz_score_captions_check": (C.c_int, [i32, i32, i32, i32]),
        "icz_butd_score_captions": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp, vp]),
        "icz_aoa_score_captions": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp, vp]),
        "icz_nic_score_captions": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp, vp]),
        "icz_ensemble_score_captions": (C.c_int, [vp, C.POINTER(vp), i32, i32, i32, vp, vp, vp, vp]),
        "icz_score_tokens": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "icz_ensemble_score_tokens": (C.c_int, [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(f32), i32, i32, vp,
                                                vp, vp]),
        "icz_distill_check": (C.c_int, [C.POINTER(DistillOpts), i32]),
        "icz_butd_xe_backward_distill": (C.c_int, [vp, C.POINTER(DistillOpts), C.POINTER(ButdParams), vp, f32, vp]),
        "icz_aoa_xe_backward_distill": (C.c_int, [vp, C.POINTER(DistillOpts), C.POINTER(AoaParams), vp, f32, vp]),
        "icz_nic_xe_backward_distill": (C.c_int, [vp, C.POINTER(DistillOpts), C.POINTER(NicParams), vp, vp, f32, vp]),
        "icz_distill_loss": (C.c_int, [vp, i32, C.POINTER(DistillOpts), vp, i32, i32, f32, vp, i32, vp, vp]),
        "icz_scst_objective_check": (C.c_int, [C.POINTER(ScstObjective), i32, i32]),
        "icz_butd_sample_backward_objective": (C.c_int, [vp, C.POINTER(ScstObjective), C.POINTER(ButdParams), vp, vp, vp, f32, vp]),
        "icz_aoa_sample_backward_objective": (C.c_int, [vp, C.POINTER(ScstObjective), C.POINTER(AoaParams), vp, vp, vp, f32, vp]),
        "icz_nic_sample_backward_objective": (C.c_int, [vp, C.POINTER(ScstObjective), C.POINTER(NicParams), vp, vp, vp, vp, f32, vp]),
        "icz_test_scst_objective": (C.c_int, [C.POINTER(ScstObjective), vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, vp]),
        "icz_swor_check": (C.c_int, [C.POINTER(SworOpts), i32, C.POINTER(i32), C.POINTER(i32)]),
        "icz_butd_xe_backward_swor": (C.c_int, [vp, C.POINTER(SworOpts), i32, C.POINTER(ButdParams), vp, vp]),
        "icz_aoa_xe_backward_swor": (C.c_int, [vp, C.POINTER(SworOpts), i32, C.POINTER(AoaParams), vp, vp]),
        "icz_nic_xe_backward_swor": (C.c_int, [vp, C.POINTER(SworOpts), i32, C.POINTER(NicParams), vp, vp, vp]),
        "icz_test_swor_objective": (C.c_int, [C.POINTER(SworOpts), vp, i32, i32, vp, i32, i32, i32, C.POINTER(i32), vp, vp, vp, vp]),
        "icz_aoa_xe_backward_dlogits": (C.c_int, [vp, vp, C.POINTER(AoaParams), vp]),
        "icz_nic_xe_backward_dlogits": (C.c_int, [vp, vp, C.POINTER(NicParams), vp, vp]),
        "icz_aoa_sample": (C.c_int, [vp, vp, i32, i32, C.POINTER(AoaRng), vp, vp, vp]),
        "icz_aoa_sample_n": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(AoaRng), vp, vp, vp]),
        "icz_aoa_scst_rollouts": (C.c_int, [vp, vp, i32, i32, C.POINTER(AoaRng), vp, vp, vp, vp]),
        "icz_aoa_sample_backward": (C.c_int, [vp, vp, C.POINTER(AoaParams), vp, vp, f32, vp]),
        "icz_aoa_xe_forward": (C.c_int, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(AoaRng), i32, vp, vp]),
        "icz_aoa_xe_backward": (C.c_int, [vp, f32, C.POINTER(AoaParams), vp, f32, vp]),
        "icz_ciderd_create": (C.c_int, [vp, vp, i64, C.c_double, vp, C.POINTER(vp)]),
        "icz_ciderd_destroy": (C.c_int, [vp]),
        "icz_ciderd_reward": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "icz_ciderd_cook_host": (C.c_int, [vp, vp, i64, C.c_double, vp, vp, i32, i64, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]),
        "icz_ciderd_vocab_create": (C.c_int, [C.c_char_p, vp, vp, i32, i32, C.POINTER(vp)]),
        "icz_ciderd_vocab_destroy": (C.c_int, [vp]),
        "icz_ciderd_vocab_oov_id": (C.c_int, [vp, C.c_char_p, i32, C.POINTER(i32)]),
        "icz_ciderd_cook_text": (C.c_int, [vp, vp, vp, i64, C.c_double, C.c_char_p, i64, i32, i64, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]),
        "icz_ciderd_reward_indexed": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "icz_ciderd_reward_loo": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "icz_ciderd_cook_device": (C.c_int, [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
        "icz_ciderd_pairwise_workspace_bytes": (C.c_size_t, [i32, i32]),
        "icz_ciderd_pairwise": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp, vp, C.c_size_t, vp]),
        "icz_ciderd_scores_csr": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "icz_ngram_diversity": (C.c_int, [vp, vp, i32, i32, vp, vp]),
        "icz_bleu_stats": (C.c_int, [vp, vp, vp, vp, vp, i32, vp, vp]),
        "icz_rouge_lcs": (C.c_int, [vp, vp, vp, vp, vp, i32, vp, vp]),
        "icz_prof_begin": (C.c_int, []),
        "icz_prof_select": (C.c_int, [i32]),
        "icz_prof_pair_overhead": (C.c_int, [vp, i32, C.POINTER(C.c_double)]),
        "icz_prof_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
        "icz_kprof_begin": (C.c_int, []),
        "icz_kprof_end": (C.c_int, [i32, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
        "icz_prof_stream_rate": (C.c_int, [vp, C.c_size_t, i32, vp, C.POINTER(C.c_double)]),
        "icz_adam_clamp_multi": (C.c_int, [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), f32, f32, i32, vp]),
        "icz_gemm_f32": (C.c_int, [i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, C.c_size_t, vp]),
        "icz_gemm_f32_seg": (C.c_int, [i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, C.c_size_t, C.POINTER(i32), vp]),
        "icz_gemm_resident_pair": (C.c_int, [i32, vp, vp, vp, vp, vp, i32, i32, vp, C.c_size_t, C.POINTER(i32)] * 2 + [vp, vp]),
        "icz_gemm_workspace_floats": (C.c_size_t, [i32, i32]),
        "icz_gemm_set_big_cfg": (C.c_int, [i32]),
        "icz_gemm_big_cfg_for": (C.c_int, [i32, i32, i32, i32, i32]),
        "icz_gemm_tn_grouped": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "icz_gemm_tn_split_pick": (C.c_int, [i32, i32, i32]),
        "icz_gemm_tn_split": (C.c_int, [vp, i32, i32, vp, i32, i32, i32, vp, i32, vp, C.c_size_t, vp, vp]),
        "icz_gemm_route_for": (C.c_int, [i32, i32, i32, i32, vp, i32]),
        "icz_gemm_split_for": (C.c_int, [i32, i32, i32, i32, vp, C.c_size_t]),
        "icz_gemm_tn_grouped_fits": (C.c_int, [i32, i32, i32, vp]),
        "icz_test_side_branch": (C.c_int, [i32, i32, vp, vp]),
        "icz_test_embed_grad": (C.c_int, [vp, i32, vp, i32, i64, vp, f32, i32, vp, i32, i32, vp, i32, vp]),
        "icz_embed_grad_route_for": (C.c_int, [i32, i32, C.POINTER(C.c_size_t)]),
        "icz_test_weight_norm": (C.c_int, [i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "icz_test_weight_norm_bwd": (C.c_int, [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "icz_test_transpose": (C.c_int, [i32, vp, vp, vp, vp, vp, vp]),
        "icz_test_colsum": (C.c_int, [i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "icz_test_timesum": (C.c_int, [vp, i32, i64, vp, vp]),
        "icz_test_rowgroup_sum": (C.c_int, [vp, i32, i32, i64, vp, vp]),
        "icz_test_bptt_dh1_step": (C.c_int, [i32, i32, i32, i32, vp, vp, vp, i32, i32, vp, i32, i32] + [vp] * 9 + [C.c_size_t, C.POINTER(i32), C.POINTER(i32), vp]),
        "icz_beam_rowtopk_route_for": (C.c_int, [i32, i32, i32]),
        "icz_test_beam_rowtopk": (C.c_int, [i32, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp]),
        "icz_test_beam_step": (C.c_int, [i32, C.POINTER(BeamStepState), i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
        "icz_test_beam_finalize": (C.c_int, [i32, i32, i32, i32, i32, i32, i32, f32, i32] + [vp] * 15),
        "icz_test_beam_rowtopk_constrained": (C.c_int, [i32, vp, i32, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp]),
        "icz_test_beam_constrained_step": (C.c_int, [i32, C.POINTER(BeamConstrainedState), i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "icz_test_beam_finalize_states": (C.c_int, [i32, i32, i32, i32, i32, i32, i32, f32] + [vp] * 13),
        "icz_test_greedy_select": (C.c_int, [i32, vp, i32, i32, i32, i32, i64, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "icz_sample_select_max_vocab": (C.c_int, []),
        "icz_test_sample_select": (C.c_int, [C.POINTER(SampleSelectArgs), i32, vp]),
        "icz_test_ss_select": (C.c_int, [vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp]),
        "icz_test_xe_loss": (C.c_int, [vp, i32, i32, vp, i32, i32, i32, C.POINTER(i32), f32, f32, vp, vp, vp, vp]),
        "icz_test_xe_group_loss": (C.c_int, [vp, i32, i32, vp, i32, i32, i32, vp, f32, f32, vp, vp, vp, vp]),
        "icz_test_reinforce": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, vp]),
        "icz_test_aoa_layer_norm": (C.c_int, [i32, vp, vp, vp, vp, i32, i32, vp, vp, vp]),
        "icz_aoa_self_attn_route_for": (C.c_int, [i32, i32, i32, i32, C.POINTER(i32), C.POINTER(C.c_size_t)]),
        "icz_test_aoa_self_attn": (C.c_int, [i32, vp, vp, i32, i32, i32, i32, vp, i32, C.POINTER(DropPArgs), C.POINTER(i32), C.POINTER(i32), vp]),
        "icz_test_aoa_dec_attn_bwd": (C.c_int, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, f32, vp, vp, vp]),
        "icz_test_aoa_ln_bwd": (C.c_int, [i32, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
        "icz_test_aoa_self_attn_bwd": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, vp, C.POINTER(DropPArgs), vp]),
        "icz_test_aoa_dkv": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, i32, C.POINTER(i32), vp]),
        "icz_test_aoa_dec_attn": (C.c_int, [vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, C.POINTER(DropPArgs), vp, vp]),
        "icz_test_embed": (C.c_int, [vp, i32, i32, vp, i32, vp, i32, C.POINTER(DropArgs), vp, vp]),
        "icz_test_embed_steps": (C.c_int, [vp, i32, i32, vp, i32, i32, C.POINTER(i32), vp, C.POINTER(DropArgs), vp]),
        "icz_test_lstm_point": (C.c_int, [i32, C.POINTER(LstmPointArgs), C.POINTER(DropArgs), C.POINTER(i32), vp]),
        "icz_test_lstm_bwd_point": (C.c_int, [C.POINTER(LstmBwdArgs), C.POINTER(DropArgs), vp]),
        "icz_test_att_mean": (C.c_int, [vp, i32, i32, i32, vp, vp, vp]),
        "icz_test_att_scores": (C.c_int, [i32, C.POINTER(AttScoresArgs), C.POINTER(DropArgs), i32, i32, vp]),
        "icz_test_att_ctx": (C.c_int, [vp, i32, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp]),
        "icz_test_att_saved_alphas": (C.c_int, [vp, i32, i32, i32, i32, vp, vp]),
        "icz_test_att_bwd_dalpha": (C.c_int, [vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
        "icz_test_att_bwd_ddec": (C.c_int, [C.POINTER(AttDdecArgs), C.POINTER(DropArgs), vp]),
        "icz_test_att_bwd_denc": (C.c_int, [C.POINTER(AttDencArgs), i32, i32, C.POINTER(i32), vp]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:
            raise IczError("libicz.so lacks symbol %s (stale build?)" % name) from e
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def check(status):
    if status != 0:
        raise IczError("libicz status %d: %s" % (status, lib().icz_last_error().decode()))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
