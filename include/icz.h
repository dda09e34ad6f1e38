/* libicz -- C ABI of the MI355X-native caption-decoding hot path (BUTD / SCST).
 *
 * The reference (zyj0021200/simpleImageCaptionZoo) is pure Python on PyTorch and has no FFI of its own; its
 * extension point for this path is the duck-typed Captioner nn.Module that Engine calls
 * (Engine.py:179-182, 258-262, 284-286) plus the loss / reward helpers in Utils.py.  Each entry point below
 * names the reference function it replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions: every pointer is a DEVICE pointer unless the name ends in _host; tensors are dense row-major
 * fp32 unless stated; ids are int64 (torch.LongTensor); `stream` is a hipStream_t passed as void* (0 = null
 * stream).  Calls are asynchronous on `stream`; nothing synchronises the device unless documented.  The
 * library never frees caller memory.  Return value: ICZ_OK (0) or a negative icz_status; icz_last_error()
 * gives the text (thread-local).  A handle is not thread-safe; distinct handles are independent.
 */
#ifndef ICZ_H_
#define ICZ_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    ICZ_OK = 0,
    ICZ_ERR_INVALID = -1,   /* bad argument / shape / alignment */
    ICZ_ERR_HIP = -2,       /* a HIP runtime call failed        */
    ICZ_ERR_STATE = -3,     /* call order violated (e.g. backward before sample) */
    ICZ_ERR_NOMEM = -4
} icz_status;

const char* icz_last_error(void);
/* library version and the gfx target it was built for ("gfx950") */
const char* icz_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * BUTD top-down attention decoder (Models/BUTD_Model.py:64-318, DecoderRNN + SoftAttention)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct icz_butd icz_butd_t;

typedef struct {
    int32_t R;        /* regions per image (36 bottom-up boxes, 49 for the 7x7 spatial grid): 1..64 through icz_butd_create; a
                         capacity of 1..128 through icz_butd_create_regions (100 for the 'adaptive' bottom-up sets), where the
                         layout of a batch is set by icz_butd_set_regions */
    int32_t D;        /* region feature size (2048)                                          */
    int32_t H;        /* LSTM hidden size (Configs/Models/BUTDDetection.json: 1024)          */
    int32_t E;        /* embedding size                                                      */
    int32_t A;        /* attention size                                                      */
    int32_t V;        /* vocabulary size                                                     */
    int32_t max_rows; /* capacity in decoder rows: batch for greedy/sample/XE, images*beam for beam search */
    int32_t max_len;  /* capacity in time steps kept for backward (>= max_len of sample / XE length)        */
} icz_butd_dims;

/* Parameter block in the reference's state_dict layout (keys "decoder.<name>", BUTD_Model.py:75-84;
 * weight_norm'd Linear layers are the old-style (weight_g, weight_v) pairs).  The same struct type carries
 * gradients (one buffer per parameter, same shapes). */
typedef struct {
    float* embed_weight;                          /* embed.0.weight          [V, E]            */
    float *td_w_ih, *td_w_hh, *td_b_ih, *td_b_hh; /* TD_atten.*              [4H, H+D+E] [4H, H] [4H] [4H] */
    float *lm_w_ih, *lm_w_hh, *lm_b_ih, *lm_b_hh; /* language_model.*        [4H, D+H]   [4H, H] [4H] [4H] */
    float *enc_att_v, *enc_att_g, *enc_att_b;     /* atten.enc_att.weight_v [A, D], weight_g [A,1], bias [A] */
    float *dec_att_v, *dec_att_g, *dec_att_b;     /* atten.dec_att.*        [A, H], [A,1], [A]               */
    float *affine_v, *affine_g, *affine_b;        /* atten.affine.*         [1, A], [1,1], [1]               */
    float *predict_v, *predict_g, *predict_b;     /* predict.*              [V, H], [V,1], [V]               */
} icz_butd_params;

int icz_butd_create(const icz_butd_dims* dims, icz_butd_t** out);
/* The same handle with dims.R as a region capacity of up to 128 (icz_butd_create keeps refusing R > 64): for the 'adaptive' bottom-up
 * sets of 10..100 boxes and any fixed set of 65..128 regions.  Every other entry takes either handle. */
int icz_butd_create_regions(const icz_butd_dims* dims, icz_butd_t** out);
int icz_butd_destroy(icz_butd_t* h);
/* Bind the (caller-owned, device-resident) parameters; pointers must stay valid while the handle is used. */
int icz_butd_bind_params(icz_butd_t* h, const icz_butd_params* params);
/* Options.  "graphs" = 1: greedy / sample / sample_backward are captured into hipGraphs on first use and replayed
 * afterwards; the cache is keyed by every pointer and size in the call, so enable it only when buffers are reused.
 * "concurrent" = 0: independent chains (greedy vs sampled rollout, predict gradients vs BPTT) run on ONE stream instead
 * of side streams (default 1); used by bench.py to time single kernels with events.
 * "early_out" (default 1, ICZ_EARLY_OUT): DecoderRNN.sample_rl breaks out of its loop once no row is unfinished
 * (BUTD_Model.py:233); on the device every kernel of a rollout step behind that point -- and of its BPTT step -- returns at entry
 * (a per-step count of unfinished rows in device memory, written by the token-choice kernel), the GEMMs over all (t, b) rows stop
 * there, and the greedy baseline of icz_butd_scst_rollouts stops once EVERY row has emitted <end>.  0 = run every step as rounds
 * 1 - 4 did: the same results, an A/B switch.
 * "merge_small" = n (default 8, 0..32, ICZ_MERGE_SMALL): icz_butd_scst_rollouts of <= n images runs the greedy baseline and the
 * sampled rollout as ONE chain of 2 B decoder rows (evaluation-mode rows in front: per-row dropout / argmax-vs-multinomial in the
 * kernels), so that the weights are streamed once per step pair; same tokens, log-probs, loss as the two chains.
 * "small_nt" (default 1): BPTT steps of <= 32 rows (small batches, the short tail of an XE batch) take their per-step dgrad products on
 * the transposed LSTM weight copies through the fp32 NT kernel instead of NN products on the weights (which stream at half the rate
 * at so few rows); 0 = the NN products of rounds 1 - 4.  Gradients agree to fp32 rounding.
 * "fused_dh1" (default 1, ICZ_BPTT_FUSED_DH1): BPTT steps of <= 64 rows whose widths the kernel takes (H in whole groups of 16, A of 64)
 * form X2 = d dec . w_dec inside the TD-LSTM backward launch instead of writing it as split-K slabs for that launch to read back: six
 * launches per step, not seven; 0 = the two launches.  Every gradient and the loss are bitwise the same: an A/B switch.
 * "group_att" (default 0): 1 = icz_butd_sample_n's attention runs on the grouped kernels (the K rows of an image in one workgroup:
 * scores, context and, in its backward, d enc_ctx read each image's features / projected features once); 0 = the per-row kernels,
 * which find the image of each row through an index (measured faster).  Ids and log-probs are bitwise the same;
 * gradients too except enc_att.*, affine.* and TD_atten.weight_ih, which may differ by fp32 rounding. */
int icz_butd_set_option(icz_butd_t* h, const char* name, int32_t value);
/* Data-parallel overlap hook (no reference counterpart: the reference is single-process).  While a backward call is
 * being enqueued, `cb(user, stage)` is invoked each time a group of gradient tensors is complete in stream order:
 *   stage 0: predict.{weight_v, weight_g, bias};  stage 1: embed.0.weight, TD_atten.weight_{ih,hh};
 *   stage 2: language_model.weight_{ih,hh};  everything else is complete when the call returns.
 * The host side starts the all-reduce of that group on the same stream (it then runs beside the remaining weight-gradient
 * GEMMs).  NULL removes the hook. */
/* Data-parallel: the global (all-reduced) loss normaliser as a DEVICE scalar, so that no host round trip separates the
 * forward pass from the backward pass: the mask sum of the rollout (then call icz_butd_sample_backward with
 * mask_sum_global < 0, "use the device value") or the token count of the XE batch (icz_butd_xe_backward with
 * n_tokens_global < 0).  icz_nic_set_norm_global / icz_aoa_set_norm_global are the same for the other two decoders. */
int icz_butd_set_mask_sum_global(icz_butd_t* h, const float* mask_sum_global_dev, void* stream);
typedef void (*icz_grad_ready_cb)(void* user, int32_t stage);
int icz_butd_set_grad_callback(icz_butd_t* h, icz_grad_ready_cb cb, void* user);
/* Re-materialise w = g * v / ||v|| for the four weight-normed layers; call after every parameter update.  The transposed copies of
 * the LSTM weights that the per-step dgrad products of BPTT read (117 MB at the BASELINE sizes, 33 us) are NOT rebuilt here but by the
 * first backward call after it (icz_butd_sample_backward / icz_butd_xe_backward*, in front of their captured graph): evaluation
 * loops refresh per batch and never need them. */
int icz_butd_refresh_weights(icz_butd_t* h, void* stream);

/* Region layout of the batches that follow (sticky; a new handle has regions = dims.R and no counts): `feats` of every
 * later call is [B, regions, D] with regions <= dims.R (the handle's capacity), and every alpha output is [.., regions].
 * counts = the number of valid leading regions of each image, i.e. bu_masks.sum(1) of the prefix masks the reference's engine
 * builds (BUTD_Engine.py:35-46), in device memory (read by the kernels of the following calls -- keep it alive until they
 * have run) and in host memory (validated here: 1 <= counts[i] <= regions); both NULL = every region valid.  Beyond the
 * reference (whose model drops the mask and attends over the zero padding): image i behaves exactly as it would alone at
 * R = counts[i] -- regions r >= counts[i] get attention weight 0 (alphas come back with zeros there), the mean feature
 * averages the valid rows, pad rows are never loaded and take no part in any gradient.  The rows of one image (beam rows, the
 * K rows of icz_butd_sample_n, both halves of a merged SCST chain) share its count.  The explicit attention-dropout mask and
 * the Philox keep-bit index stay ((row * regions + r) * A + c).  A later call with more images than n_img while counts are
 * set returns ICZ_ERR_INVALID.  Calls made while counts are set run eagerly (option "graphs" does not capture them); the
 * captured graphs of fixed region sets are keyed by `regions`.  A forward pass stored for a backward call is dropped. */
int icz_butd_set_regions(icz_butd_t* h, int32_t regions, const int32_t* counts_dev, const int32_t* counts_host, int32_t n_img);

/* DecoderRNN.sample (BUTD_Model.py:153-189): greedy decode.
 * feats [B,R,D]; ids_out [B,max_len] int64; alphas_out [B,max_len,R] or NULL (R = the regions of icz_butd_set_regions). */
int icz_butd_greedy(icz_butd_t* h, const float* feats, int32_t B, int32_t max_len, int64_t* ids_out,
                    float* alphas_out, void* stream);

/* Randomness for the training-mode paths.  Either explicit arrays (parity tests; layouts below) or, for any
 * NULL pointer, an in-kernel counter-based generator (Philox4x32-10) keyed by `seed` -- reproduced
 * bit-for-bit by the matching backward call, so nothing is stored. */
typedef struct {
    uint64_t seed;
    const float* uniforms;     /* [T, B]        one draw per row per step (multinomial), in [0,1) */
    const uint8_t* emb_mask;   /* [T, B, E]     keep-masks (1 = keep) of nn.Dropout(0.5) on the embedding, */
    const uint8_t* att_mask;   /* [T, B, R, A]  on relu(enc_ctx + dec_ctx) in SoftAttention,               */
    const uint8_t* out_mask;   /* [T, B, H]     and on h2 before `predict`                                 */
} icz_rng;

/* DecoderRNN.sample_rl (BUTD_Model.py:191-234), training mode (dropout active).
 * seq_out [B,max_len] int64 (0 at and after a sampled <end>), logprobs_out [B,max_len].  Activations needed by
 * icz_butd_sample_backward are kept inside the handle until the next sample/XE call. */
int icz_butd_sample(icz_butd_t* h, const float* feats, int32_t B, int32_t max_len, const icz_rng* rng,
                    int64_t* seq_out, float* logprobs_out, void* stream);

/* Both rollouts of one SCST step (Engine.py:258-262: greedy baseline in eval mode + sampled rollout in train mode)
 * in one call; the two decode chains share the per-image prologue and run concurrently on two streams.  Results are
 * identical to icz_butd_greedy + icz_butd_sample. */
/* (greedy_ids_out: the reference's greedy ids up to and including every row's first <end> -- all the reward reads, Utils.py:354;
 * columns behind the step at which the LAST row emitted it are 0, see option "early_out".) */
int icz_butd_scst_rollouts(icz_butd_t* h, const float* feats, int32_t B, int32_t max_len, const icz_rng* rng,
                           int64_t* greedy_ids_out, int64_t* seq_out, float* logprobs_out, void* stream);
/* Beyond the reference (which draws ONE sampled caption per image, Engine.py:258-262): the multi-sample rollout of the "new
 * self-critical" SCST variant -- K = 2..8 sampled captions per image for B images, decoder row = img * K + k, B K <= max_rows.  The
 * per-image work (mean features, enc_att(feats), the mean part of the TD gates) runs once per image, the sampled chain over the B K
 * rows.  Dropout keep-bits and draws are indexed by the row in the B K space (explicit icz_rng arrays are laid out for B K rows):
 * row img * K + k gets the draws row img * K + k of icz_butd_sample on the features repeated K times gets (the ids agree with that
 * call up to draws at a CDF edge; the per-image GEMMs run at another M, so their rounding may differ).  feats [B,R,D]; seq_out
 * [B K, max_len] int64, logprobs_out [B K, max_len].  icz_butd_sample_backward / _dlogp then take rewards [B K, max_len]. */
int icz_butd_sample_n(icz_butd_t* h, const float* feats, int32_t B, int32_t K, int32_t max_len, const icz_rng* rng,
                      int64_t* seq_out, float* logprobs_out, void* stream);

/* RewardCriterion.forward + loss.backward() for the rollout kept by the last icz_butd_sample
 * (Utils.py:295-317, Engine.py:266-270).  reward [B,max_len]; grads receives d loss / d parameter (overwritten,
 * not accumulated); loss_out (1 float, device) receives the loss.
 * Data-parallel use: pass mask_sum_global > 0 to normalise by the all-rank sum of the mask instead of the
 * local one; mask_sum_out (1 float, device, may be NULL) always receives the local mask sum. */
int icz_butd_sample_backward(icz_butd_t* h, const float* reward, const icz_butd_params* grads, float* loss_out,
                             float* mask_sum_out, float mask_sum_global, void* stream);
/* Same backward, driven by an arbitrary upstream gradient d loss / d logprobs [B,max_len] (what autograd hands to
 * the sampler_rl output when the reference's own RewardCriterion + loss.backward() are used, Engine.py:266-270). */
int icz_butd_sample_backward_dlogp(icz_butd_t* h, const float* dlogp, const icz_butd_params* grads, void* stream);
/* local sum of the REINFORCE mask of the last rollout (1 float, device) without running backward */
int icz_butd_sample_mask_sum(icz_butd_t* h, float* mask_sum_out, void* stream);

/* DecoderRNN.forward + LabelSmoothingLoss + backward (BUTD_Model.py:97-151, Utils.py:268-286,
 * Engine.py:178-186).  captions [B,L] int64, rows sorted by length descending; lengths_host[b] = len-1 as in
 * Engine.py:178 (host array).  packed_logits_out [sum(lengths), V] in pack_padded_sequence order or NULL.
 * n_tokens_global > 0 replaces the local token count as the loss normaliser (data-parallel); < 0: the device scalar set by
 * icz_butd_set_mask_sum_global. */
int icz_butd_xe_forward(icz_butd_t* h, const float* feats, const int64_t* captions, int32_t B, int32_t L,
                        const int32_t* lengths_host, const icz_rng* rng, int32_t train,
                        float* packed_logits_out, void* stream);
int icz_butd_xe_backward(icz_butd_t* h, float smoothing, const icz_butd_params* grads, float* loss_out,
                         float n_tokens_global, void* stream);
/* Beyond the reference (whose loader hands every annotation over as a row of its own, Datasets.py:47-51): teacher-forced XE on K = 2..8
 * captions per image, the regime of seq_per_img = 5, in the layout of icz_butd_sample_n.  feats [B, R, D], one feature set per image;
 * captions [B K, L] int64, row = img * K + k, each with its leading <sta> and zero padded, in ANY length order (nothing is sorted);
 * lengths_host [B K] = len - 1 as for icz_butd_xe_forward, each in 1..L-1; T = max(lengths); B K <= max_rows.  The per-image work
 * (enc_att(feats), the mean features, the hoisted part of the TD gates) runs once over the B images, the teacher-forced chain over the
 * B K rows (grouped attention kernels where option "group_att" is on).  A row that has ended is fed <pad> and its later steps carry no
 * loss.  Dropout keep-bits and Philox indices are those of row img * K + k in the B K space: explicit icz_rng arrays are laid out
 * [T, B K, ...], and row r gets what row r of icz_butd_sample_n gets.  Region counts (icz_butd_set_regions) are per image, as there.
 * logits_out: NULL, or [B K, T, V] with zeros at t >= the row's length.  The call is eager (no graph capture), as icz_butd_xe_forward.
 * Refused, in this order, each before anything is queued and with the handle left as it was:
 *   1 null feats, captions or lengths_host;  2 K outside 2..8;  3 B < 1, L < 2 or a length outside 1..L-1;  (a null handle);
 *   4 B K above the row capacity, or more images than region counts were set for;  5 weights not refreshed;  6 train without an rng;
 *   7 scheduled sampling switched on (icz_butd_set_scheduled_sampling).
 * icz_butd_xe_backward then runs the same loss over the image-major rows (mask t < length of the row) and the backward pass with the
 * image-side products folded onto the B images; n_tokens_global as above in all three forms.  icz_butd_saved_alphas returns [B K, T, R]
 * (the steps behind a row's end hold the attention of its <pad> steps).  icz_butd_xe_backward_dlogits, icz_butd_xe_backward_distill and
 * icz_butd_xe_backward_swor work on packed, length-sorted rows and refuse a stored grouped forward by name; it stays stored. */
int icz_butd_xe_forward_n(icz_butd_t* h, const float* feats, const int64_t* captions, int32_t B, int32_t K, int32_t L,
                          const int32_t* lengths_host, const icz_rng* rng, int32_t train, float* logits_out, void* stream);

/* Scheduled sampling in DecoderRNN.forward (BUTD_Model.py:120-132; the decoder attribute `ss_prob`, which
 * Engine.py:140-144 means to raise per epoch but sets on the Captioner, where nothing reads it): from time step 2 on,
 * row b of the following icz_butd_xe_forward calls feeds a draw from softmax(logits of step t-1) instead of its caption
 * token when gate[t,b] < ss_prob.  gate_uniforms / draw_uniforms: device arrays [T,B] in [0,1) (T = max(lengths), B of
 * the forward call; parity tests) or NULL for the Philox generator keyed by the call's icz_rng seed.  The draw is the
 * inverse-CDF draw of the sampler contract (smallest v with cumsum(p)[v] > u sum(p), float64 sums); no gradient
 * flows through it and the embedding gradient goes to the tokens actually fed.  ss_prob = 0 (default) switches it off. */
int icz_butd_set_scheduled_sampling(icz_butd_t* h, float ss_prob, const float* gate_uniforms, const float* draw_uniforms);

/* Attention maps of the forward pass the handle holds (the last icz_butd_xe_forward or icz_butd_sample of B rows and T
 * steps, or icz_butd_xe_forward_n of B K rows): alphas_out [B, T, R].  A teacher-forced evaluation-mode forward over a decoded sentence yields the alphas the
 * reference's sample / beam_search_sample return beside the ids (BUTD_Model.py:178-189, :309-317), which
 * eval_test_image hands to show_additional_rlt (Engine.py:325,339). */
int icz_butd_saved_alphas(icz_butd_t* h, float* alphas_out, void* stream);

/* XE backward driven by an upstream gradient w.r.t. the packed logits [sum(lengths), V] (autograd path:
 * criterion(predictions[0], targets[0]).backward(), Engine.py:182-186). */
int icz_butd_xe_backward_dlogits(icz_butd_t* h, const float* dpacked, const icz_butd_params* grads, void* stream);

/* DecoderRNN.beam_search_sample (BUTD_Model.py:236-318) for n_img images at once (the reference runs one image
 * per call, Utils.py:72-73).  feats [n_img,R,D]; seqs_out [n_img, max_steps+1] float32 incl. the leading <sta>
 * and, if finished, the trailing <end>; lens_out [n_img] int32 = valid length of each row. */
int icz_butd_beam_search(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                         float* seqs_out, int32_t* lens_out, void* stream);

/* Options of the icz_*_beam_search_opts entries (the same search, every step as above):
 *   n_best       1..beam: hypotheses returned per image.  Each image ends with exactly `beam` of them (the retired ones and those
 *                live at the step limit), ranked finished before live, then by normalised score (descending), then by order of
 *                retirement (step, then merge rank; live ones in beam order).
 *   block_ngram  0 (off), 2, 3 or 4: a beam with prefix y_0..y_s may not take v if (y_{s-n+2}, ..., y_s, v) already occurs in the
 *                prefix.  A banned token scores -inf after the log-softmax (whose normaliser still runs over the whole vocabulary),
 *                so every score stays the model's log-probability of its tokens.  The first step has no bans.
 *   lp_kind      0 none, 1 avg (score / len^alpha), 2 wu (score / ((5 + len) / 6)^alpha), len = generated tokens with <end>
 *                (lens - 1), fp32.  It changes only the final ranking, never which beams expand, retire or survive.
 *   lp_alpha     >= 0, finite.
 * {1, 0, 0, 0} is icz_*_beam_search bit for bit. */
typedef struct {
    int32_t n_best;
    int32_t block_ngram;
    int32_t lp_kind;   /* 0 none, 1 avg, 2 wu */
    float lp_alpha;
} icz_beam_opts;

/* Beam search with options: seqs_out [n_img, n_best, max_steps+1] float32 (zero-padded), lens_out [n_img, n_best] int32,
 * scores_out [n_img, n_best] float32 raw summed log-probabilities.  Argument errors (null handle / argument / options, n_best
 * outside 1..beam, block_ngram not in {0, 2, 3, 4}, lp_kind unknown, lp_alpha negative or not finite) return ICZ_ERR_INVALID
 * before any device work. */
int icz_butd_beam_search_opts(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                              const icz_beam_opts* opts, float* seqs_out, int32_t* lens_out, float* scores_out, void* stream);

/* Diverse beam search (Vijayakumar et al., "Diverse Beam Search", AAAI 2018) for the icz_*_beam_search_diverse entries:
 *   groups     1..beam, dividing beam: the beam splits into `groups` groups of kg = beam / groups beams, each run as the search
 *              above (shrinking kg, its own <end> retirements) over the same decoder step.
 *   diversity  lambda >= 0, finite.  At every step the groups select in order; group g ranks its candidates by
 *              score - fp32(lambda * c), c = how often groups 0 .. g-1 picked that token at this step (<end> included).
 *              The penalty acts on this step's selection only: it never enters the running score, and every group starts at
 *              step 1 (self-critical.pytorch's variant accumulates it and staggers the groups; neither is done here).
 * The image's list holds the beam hypotheses of all groups (retirements in order of step, group, merge rank, then the beams
 * live at the limit in group, slot order), ranked as icz_beam_opts says, with raw log-probability scores.
 * {1, 0} is icz_*_beam_search_opts bit for bit; lambda = 0 runs `groups` independent copies of the kg-beam search. */
typedef struct {
    int32_t groups;
    float diversity;
} icz_beam_diversity;

/* icz_butd_beam_search_opts with grouped beams and a diversity penalty; the outputs are those of _opts.  Argument errors return
 * ICZ_ERR_INVALID before any device work, checked in this order: the options (as _opts), a null `div`, groups outside 1..beam
 * or not dividing it, diversity negative or not finite, null arguments, null handle. */
int icz_butd_beam_search_diverse(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                                 const icz_beam_opts* opts, const icz_beam_diversity* div, float* seqs_out, int32_t* lens_out,
                                 float* scores_out, void* stream);

/* Constrained beam search (Anderson, Fernando, Johnson, Gould, "Guided Open Vocabulary Image Captioning with Constrained Beam Search",
 * EMNLP 2017) for the icz_*_beam_search_constrained entries: every returned caption is steered to contain given words.
 *   Constraints.  Image img has c constraints, 0 <= c <= max_constraints = C <= 3; a constraint is a set of 1..max_alts = A <= 4
 *     alternative word ids (singular / plural, synonyms) and is satisfied once the hypothesis contains any of them.  words_dev (a
 *     DEVICE array) and words_host (its HOST copy, read for the checks; the dev + host contract of icz_*_set_regions) are both
 *     [n_img, C, A] int32 with -1 for an empty slot, constraints and alternatives filled from the left.  A word id lies in [3, V)
 *     (not <pad>, <sta>, <end>) and appears at most once among the words of its image.  Multi-word phrases are not supported.
 *   States.  A hypothesis's state is the bit mask of its satisfied constraints: S = 2^C states, each owning `beam` row slots; an
 *     image has K = S * beam decoder rows, state-major (row img * K + s * beam + j).  beam in 1..8, K <= 32, n_img * K within
 *     the row capacity.  Every state runs the search of icz_*_beam_search_opts: its own capacity cap[s] (beam minus its <end>
 *     retirements) and its own live beams.  Before step 1 only state 0 is live, with the hypothesis [<sta>] at score 0 (one
 *     row is scored at step 1); an image with c < C constraints never sets bits >= c, so those states stay empty.
 *   A step.  Every live row (s, j) is scored over all tokens v as run + log_softmax(logits)[v] (on the device
 *     rs + ((x - mx) - ls)); under block_ngram a banned token scores -inf as icz_beam_opts says.  Candidate (s, j, v) has target
 *     state s | bit(v), bit(v) = 0 for a word in none of the image's constraints.  Then, for every target t in ascending order:
 *     t takes the best cap[t] finite candidates whose target is t, ties to the lower flat index (s * beam + j) * V + v; a pick of
 *     <end> retires into the image's list (with t, the step, the raw score and the tokens) and lowers cap[t] by one; every other
 *     pick becomes a live beam of t, compacted into t's slots in pick order.
 *   The search ends at max_steps or when no state of any image has a live beam.
 *   Result.  The image's hypotheses are its retirements in order (step, target state, merge rank) followed by the beams live at
 *     the limit in (state, slot) order, ranked by (1) the popcount of the state, descending, (2) finished before live, (3) the
 *     length-normalised score of icz_beam_opts, descending, (4) that order.  The first n_best (1..beam) are returned with raw summed
 *     log-probabilities (seqs_out / lens_out / scores_out as _opts) and their states in sat_out [n_img, n_best] int32; a rank past the
 *     image's hypotheses has length 0, score -inf and state 0.
 *   When no image has a constraint (C = 0 or every slot -1) the call is icz_*_beam_search_opts bit for bit (its kernels; sat_out 0).
 *   Diverse groups cannot be combined with constraints: the entries take no icz_beam_diversity.
 * Argument errors return ICZ_ERR_INVALID before any device work (a refused call queues nothing), checked in this order: the options
 * (as _opts); the constraints (null struct, C outside 0..3, A outside 1..4, a null word array with C > 0, beam outside 1..8,
 * 2^C * beam above 32, n_img < 1, a slot filled behind an empty one, an id below -1, <pad> / <sta> / <end>, a repeated id); null
 * arguments; a null handle; then, with the handle, max_steps, n_img * K above the row capacity, an id >= V, an unrefreshed handle. */
typedef struct {
    int32_t max_constraints;      /* C */
    int32_t max_alts;             /* A */
    const int32_t* words_dev;     /* [n_img, C, A] device */
    const int32_t* words_host;    /* [n_img, C, A] host */
} icz_beam_constraints;
int icz_butd_beam_search_constrained(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                                     const icz_beam_opts* opts, const icz_beam_constraints* cons, float* seqs_out, int32_t* lens_out,
                                     float* scores_out, int32_t* sat_out, void* stream);

/* One decoder step from an explicit state (BUTD_Model.py:172-182) -- exposed for the per-kernel parity tests.
 * it [B] int64; state tensors [B,H] are updated in place; ctx_out [B,D], alpha_out [B,R], logits_out [B,V]. */
int icz_butd_step(icz_butd_t* h, const float* feats, int32_t B, const int64_t* it, float* h1, float* c1,
                  float* h2, float* c2, float* ctx_out, float* alpha_out, float* logits_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * NIC decoder (Models/NIC_Model.py:39-212, DecoderRNN): plain embedding -> one LSTMCell -> predict; the image
 * embedding `features` [B,E] (output of the CNN encoder, outside the hot path) enters through one LSTM step from the
 * zero state (:52-56).  Same conventions as the BUTD entry points; of icz_rng only `uniforms` and `out_mask` are used.
 * dfeatures_out [B,E] (may be NULL) receives d loss / d features for an upstream encoder.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct icz_nic icz_nic_t;
typedef struct { int32_t E, H, V, max_rows, max_len; } icz_nic_dims;
typedef struct {
    float* embed_weight;                  /* embed.weight   [V, E]                         */
    float *w_ih, *w_hh, *b_ih, *b_hh;     /* lstm.*         [4H, E] [4H, H] [4H] [4H]      */
    float *predict_v, *predict_g, *predict_b;   /* predict.weight_v [V,H], weight_g [V,1], bias [V] */
} icz_nic_params;
int icz_nic_create(const icz_nic_dims* dims, icz_nic_t** out);
int icz_nic_destroy(icz_nic_t* h);
int icz_nic_bind_params(icz_nic_t* h, const icz_nic_params* params);
int icz_nic_refresh_weights(icz_nic_t* h, void* stream);
/* DecoderRNN.sample, NIC_Model.py:100-119 */
int icz_nic_greedy(icz_nic_t* h, const float* features, int32_t B, int32_t max_len, int64_t* ids_out, void* stream);
/* DecoderRNN.sample_rl, NIC_Model.py:121-151, and RewardCriterion + backward (Utils.py:295-317) */
int icz_nic_sample(icz_nic_t* h, const float* features, int32_t B, int32_t max_len, const icz_rng* rng, int64_t* seq_out,
                   float* logprobs_out, void* stream);
int icz_nic_sample_backward(icz_nic_t* h, const float* reward, const icz_nic_params* grads, float* dfeatures_out, float* loss_out,
                            float* mask_sum_out, float mask_sum_global, void* stream);
/* Beyond the reference (extends icz_nic_sample as icz_butd_sample_n extends icz_butd_sample): the multi-sample rollout -- K = 2..8
 * sampled captions per image for B images, decoder row = img * K + k, B K <= max_rows.  features [B, E] are expanded to the B K rows on
 * the device and the rollout runs on those rows: tokens, log-probs and, after icz_nic_sample_backward with a reward [B K, max_len], every
 * parameter gradient are bitwise those of icz_nic_sample on the features repeated K times (explicit icz_rng arrays are laid out for
 * B K rows).  seq_out [B K, max_len] int64, logprobs_out [B K, max_len].  dfeatures_out of the backward call is per image, [B, E]: the
 * K rows' gradients added in k order. */
int icz_nic_sample_n(icz_nic_t* h, const float* features, int32_t B, int32_t K, int32_t max_len, const icz_rng* rng, int64_t* seq_out,
                     float* logprobs_out, void* stream);
/* DecoderRNN.forward, NIC_Model.py:58-98, and LabelSmoothingLoss + backward (Utils.py:268-286) */
int icz_nic_xe_forward(icz_nic_t* h, const float* features, const int64_t* captions, int32_t B, int32_t L, const int32_t* lengths_host,
                       const icz_rng* rng, int32_t train, float* packed_logits_out, void* stream);
int icz_nic_xe_backward(icz_nic_t* h, float smoothing, const icz_nic_params* grads, float* dfeatures_out, float* loss_out,
                        float n_tokens_global, void* stream);
int icz_nic_set_norm_global(icz_nic_t* h, const float* norm_dev, void* stream);
/* Option "early_out" (default 1; also icz_butd_set_option / icz_aoa_set_option): the kernels of the rollout / BPTT steps behind
 * sample_rl's break (NIC_Model.py:150: every row has finished) return at entry; 0 = run them as rounds 1 - 4 did (A/B switch: the
 * results are the same). */
int icz_nic_set_option(icz_nic_t* h, const char* name, int32_t value);
/* Scheduled sampling for the following icz_nic_xe_forward calls (NIC_Model.py:77-89): see icz_butd_set_scheduled_sampling. */
int icz_nic_set_scheduled_sampling(icz_nic_t* h, float ss_prob, const float* gate_uniforms, const float* draw_uniforms);
/* DecoderRNN.beam_search_sample, NIC_Model.py:153-212 (batched over images) */
int icz_nic_beam_search(icz_nic_t* h, const float* features, int32_t n_img, int32_t beam, int32_t max_steps, float* seqs_out,
                        int32_t* lens_out, void* stream);
/* ... with options (icz_beam_opts, see icz_butd_beam_search_opts) */
int icz_nic_beam_search_opts(icz_nic_t* h, const float* features, int32_t n_img, int32_t beam, int32_t max_steps,
                             const icz_beam_opts* opts, float* seqs_out, int32_t* lens_out, float* scores_out, void* stream);
/* ... with grouped beams and a diversity penalty (icz_beam_diversity, see icz_butd_beam_search_diverse) */
int icz_nic_beam_search_diverse(icz_nic_t* h, const float* features, int32_t n_img, int32_t beam, int32_t max_steps,
                                const icz_beam_opts* opts, const icz_beam_diversity* div, float* seqs_out, int32_t* lens_out,
                                float* scores_out, void* stream);
/* ... with constraints: captions that must contain given words (icz_beam_constraints states the search; see
 * icz_butd_beam_search_constrained) */
int icz_nic_beam_search_constrained(icz_nic_t* h, const float* features, int32_t n_img, int32_t beam, int32_t max_steps,
                                    const icz_beam_opts* opts, const icz_beam_constraints* cons, float* seqs_out, int32_t* lens_out,
                                    float* scores_out, int32_t* sat_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * AoADetection captioner (Models/AoA_Model.py:657-753): img_feats_porjection (Linear 2048->Hd + ReLU + Dropout) ->
 * AoA_Refine_Core (6 x {LayerNorm -> 8-head self-attention over the R regions -> GLU gate -> residual}, final LayerNorm;
 * :122-162) once per image, then AoA_Decoder (:197-502) per step: embed -> LSTMCell([emb, mean + drop(ctx)]) -> LayerNorm
 * -> 8-head attention over the refined regions + GLU -> predict.  Fixed region sets (36 boxes or the 7x7 grid,
 * bu_masks = None) and the 'adaptive' ones (10..100 boxes per image with prefix bu_masks, AoA_Engine.py:37-44) through
 * icz_aoa_set_regions.
 * Only decoder.* parameters receive gradients: they are the only ones in the reference's optimizer (:669-674).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct icz_aoa icz_aoa_t;
typedef struct { int32_t R, D, Hd, E, V, NH, max_rows, max_len; } icz_aoa_dims;
typedef struct {   /* one AoABlock + its LayerNorm: linear_Q/K/V [Hd,Hd]+[Hd], aoa_module.0 [2Hd,2Hd]+[2Hd], norm gain/bias [Hd] */
    float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *aoa_w, *aoa_b, *ln_g, *ln_b;
} icz_aoa_block;
typedef struct {
    float *proj_w, *proj_b;                        /* img_feats_porjection.0.{weight [Hd,D], bias [Hd]}              */
    icz_aoa_block layer[6];                        /* aoa_refine.aoa_layers.<l>.{aoa_block.*, sublayer.norm.*}        */
    float *ref_ln_g, *ref_ln_b;                    /* aoa_refine.norm.{gain, bias}                                    */
    float *lstm_w_ih, *lstm_w_hh, *lstm_b_ih, *lstm_b_hh;   /* decoder.lstm.*  [4Hd, E+Hd] [4Hd, Hd] [4Hd] [4Hd]      */
    icz_aoa_block dec;                             /* decoder.aoa_block.* and decoder.h_norm.{gain,bias} (ln_g, ln_b) */
    float* embed_weight;                           /* decoder.embed.0.weight [V, E]                                   */
    float *predict_v, *predict_g, *predict_b;      /* decoder.predict.*                                               */
} icz_aoa_params;
/* Randomness of the training-mode paths (explicit arrays for parity tests, Philox from `seed` for NULL pointers).
 * Keep-masks (1 = keep) with the reference's drop probabilities: proj 0.5 [B,R,Hd]; per refiner layer: ref_att 0.1
 * [6,B,NH,R,R], ref_aoa 0.3 [6,B,R,2Hd], ref_sc 0.1 [6,B,R,Hd]; per step: emb 0.5 [T,B,E], ctx 0.5 [T,B,Hd], att 0.1
 * [T,B,NH,R], out 0.5 [T,B,Hd]; uniforms [T,B]. */
typedef struct {
    uint64_t seed;
    const float* uniforms;
    const uint8_t *proj_mask, *ref_att_mask, *ref_aoa_mask, *ref_sc_mask, *emb_mask, *ctx_mask, *att_mask, *out_mask;
} icz_aoa_rng;
int icz_aoa_create(const icz_aoa_dims* dims, icz_aoa_t** out);
int icz_aoa_destroy(icz_aoa_t* h);
int icz_aoa_bind_params(icz_aoa_t* h, const icz_aoa_params* params);
int icz_aoa_refresh_weights(icz_aoa_t* h, void* stream);
/* Region layout of the batches that follow (sticky; a new handle has regions = dims.R and no counts): `feats` of every
 * later call is [B, regions, D] with regions <= dims.R (the handle's capacity).  counts = the number of valid leading
 * regions of each image, i.e. bu_masks.sum(1) of the reference's prefix masks (AoA_Engine.py:37-40), in device memory
 * (read by the kernels of the following calls -- keep it alive until they have run) and in host memory (validated here:
 * 1 <= counts[i] <= regions); both NULL = every region valid (bu_masks = None).  Masked keys get attention weight 0
 * (masked_fill(-1e9) before the softmax, AoA_Model.py:63-64), the projection runs on the valid rows only (pack_wrapper,
 * :650-653 -- here the whole refiner does: the padded rows the reference carries along never reach a result) and
 * mean_features averages the valid rows (:253). */
int icz_aoa_set_regions(icz_aoa_t* h, int32_t regions, const int32_t* counts_dev, const int32_t* counts_host, int32_t n_img);
/* Option "graphs" = 1 (round 5): icz_aoa_scst_rollouts and icz_aoa_sample_backward are captured into hipGraphs on first use and
 * replayed afterwards, as icz_butd_set_option("graphs") does for the BUTD decoder; keyed by every pointer and size of the call, so
 * enable it only when buffers are reused.  Batches with per-image region counts (icz_aoa_set_regions), explicit randomness arrays
 * and a backward pass under a gradient-ready callback stay eager.
 * Option "refine_pair" (default 1, round 5): icz_aoa_scst_rollouts runs the evaluation-mode refiner pass of the greedy baseline and the
 * training-mode pass of the sampled rollout (AoA_Model.py:698-714 under Engine.py:256-262) as ONE pass over twice the rows -- same
 * bits in both halves as the two passes when the GEMMs take the same split-K decomposition (they do at the BASELINE batch of 64;
 * otherwise within fp32 rounding); 0 = two passes.  Fixed region counts only (a batch under icz_aoa_set_regions runs two passes).
 * Option "mha_mfma" (default 1, round 5): the refiner's self-attention (AoA_Model.py:41-69) on the fp32 matrix pipe for up to 64
 * regions; 0 = the register-blocked kernel of rounds 1 - 4 (which larger region sets use anyway). 
 * Option "train_refiner" (default 0; beyond the reference, which optimises the decoder only, AoA_Model.py:669-674): 1 = the backward passes
 * (icz_aoa_xe_backward, icz_aoa_sample_backward) also fill the gradient slots of img_feats_porjection.* and aoa_refine.* of `grads`: d refined
 * from the decoder block's linear_K / linear_V and the region mean, back through the final norm, the six refiner layers (each recomputed from
 * its stored input: a training-mode refiner pass keeps 7 tensors of region rows x Hd) and the projection; there is no gradient to the features.
 * With 1 every one of those 64 slots must be non-null (ICZ_ERR_INVALID before any launch otherwise) and the forward pass must have been a
 * training-mode one made while the option was on (an evaluation-mode pass stores nothing).  With 0 those slots are ignored, as before, and
 * nothing else changes.  The self-attention backward keeps three head tiles and two R x R tiles of an (image, head) in LDS: batches whose region
 * count needs more than 156 KB (more than 64 regions at heads of 128 columns) are REFUSED with an error, there is no slower path.  Changing the
 * option releases the training buffers and the captured graphs.  Deterministic: no atomics, fixed summation order. */
int icz_aoa_set_option(icz_aoa_t* h, const char* name, int32_t value);
/* eval-mode refined features [B,regions,Hd] (AoADetection_Captioner.sampler's first two lines, :712-713) -- for tests.  With
 * region counts the refiner runs on the packed valid rows; rows past an image's count come back as zeros. */
int icz_aoa_refine(icz_aoa_t* h, const float* feats, int32_t B, float* refined_out, void* stream);
/* AoADetection_Captioner.sampler / beam_search_sampler / sampler_rl / forward (:698-753, :676-696) */
int icz_aoa_greedy(icz_aoa_t* h, const float* feats, int32_t B, int32_t max_len, int64_t* ids_out, void* stream);
int icz_aoa_beam_search(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps, float* seqs_out,
                        int32_t* lens_out, void* stream);
int icz_aoa_beam_search_opts(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                             const icz_beam_opts* opts, float* seqs_out, int32_t* lens_out, float* scores_out, void* stream);
/* ... with grouped beams and a diversity penalty (icz_beam_diversity, see icz_butd_beam_search_diverse) */
int icz_aoa_beam_search_diverse(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                                const icz_beam_opts* opts, const icz_beam_diversity* div, float* seqs_out, int32_t* lens_out,
                                float* scores_out, void* stream);
/* ... with constraints: captions that must contain given words (icz_beam_constraints states the search; see
 * icz_butd_beam_search_constrained) */
int icz_aoa_beam_search_constrained(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                                    const icz_beam_opts* opts, const icz_beam_constraints* cons, float* seqs_out, int32_t* lens_out,
                                    float* scores_out, int32_t* sat_out, void* stream);
int icz_aoa_sample(icz_aoa_t* h, const float* feats, int32_t B, int32_t max_len, const icz_aoa_rng* rng, int64_t* seq_out,
                   float* logprobs_out, void* stream);
/* Beyond the reference (extends icz_aoa_sample as icz_butd_sample_n extends icz_butd_sample): the multi-sample rollout -- K = 2..8
 * sampled captions per image for B images, decoder row = img * K + k, B K <= max_rows.  The training-mode refiner pass, the region mean
 * and the hoisted linear_K / linear_V run ONCE over the B images (the region counts of icz_aoa_set_regions apply); the T decoder steps
 * run over the B K rows, which find their image through a device index.  Decoder dropout (embedding, ctx, attention, output) and the
 * draws are indexed by the row in the B K space: explicit masks are [T, B K, ...], uniforms [T, B K]; the refiner's masks are per image.
 * Row img * K + k draws what row img * K + k of icz_aoa_sample on the features repeated K times (refiner masks repeated too) draws, up to
 * the rounding of the refiner's GEMMs at another M.  seq_out [B K, max_len] int64, logprobs_out [B K, max_len].
 * icz_aoa_sample_backward then takes a reward [B K, max_len]: d linear_K / d linear_V are summed per image over its K rows and the steps
 * in a fixed order, their weight gradients run over the B images' region rows, and with option "train_refiner" the refiner's backward
 * pass runs over the B images.  Option "graphs" captures the call (K is part of the key, also of the backward pass's). */
int icz_aoa_sample_n(icz_aoa_t* h, const float* feats, int32_t B, int32_t K, int32_t max_len, const icz_aoa_rng* rng, int64_t* seq_out,
                     float* logprobs_out, void* stream);
/* The two decodes of one SCST step (Engine.py:256-261: greedy in eval mode, sampler_rl in train mode) as concurrent chains. */
int icz_aoa_scst_rollouts(icz_aoa_t* h, const float* feats, int32_t B, int32_t max_len, const icz_aoa_rng* rng, int64_t* ids_out,
                          int64_t* seq_out, float* logprobs_out, void* stream);
int icz_aoa_sample_backward(icz_aoa_t* h, const float* reward, const icz_aoa_params* grads, float* loss_out, float* mask_sum_out,
                            float mask_sum_global, void* stream);
int icz_aoa_xe_forward(icz_aoa_t* h, const float* feats, const int64_t* captions, int32_t B, int32_t L, const int32_t* lengths_host,
                       const icz_aoa_rng* rng, int32_t train, float* packed_logits_out, void* stream);
int icz_aoa_xe_backward(icz_aoa_t* h, float smoothing, const icz_aoa_params* grads, float* loss_out, float n_tokens_global,
                        void* stream);
int icz_aoa_set_norm_global(icz_aoa_t* h, const float* norm_dev, void* stream);
/* Data-parallel overlap hook of the AoA decoder's backward passes (icz_aoa_sample_backward, icz_aoa_xe_backward), as
 * icz_butd_set_grad_callback: cb(user, stage) is called on the calling thread while the backward pass is being enqueued, each time
 * a group of the decoder's gradients (the only parameters in the reference's optimizer, AoA_Model.py:669-674) is complete in
 * stream order:
 *   stage 0: decoder.predict.{weight_v, weight_g, bias} -- before the reverse-time loop, so its all-reduce runs beside all of BPTT;
 *   stage 1: decoder.embed.0.weight, decoder.lstm.{weight_ih, weight_hh, bias_ih, bias_hh};
 * the attention block's and h_norm's gradients are complete when the call returns.  NULL removes the hook. */
int icz_aoa_set_grad_callback(icz_aoa_t* h, icz_grad_ready_cb cb, void* user);
/* As icz_butd_saved_alphas: the decoder block's attention weights averaged over the heads (AoA_Model.py:118), [B, T, regions]. */
int icz_aoa_saved_alphas(icz_aoa_t* h, float* alphas_out, void* stream);
/* Scheduled sampling for the following icz_aoa_xe_forward calls (AoA_Model.py:258-270): see icz_butd_set_scheduled_sampling. */
int icz_aoa_set_scheduled_sampling(icz_aoa_t* h, float ss_prob, const float* gate_uniforms, const float* draw_uniforms);

/* ------------------------------------------------------------------------------------------------------------
 * Model ensembles (beyond the reference; self-critical.pytorch's AttEnsemble): M = 1..4 member decoders -- any mix of BUTD, AoA
 * and NIC handles (kinds 0, 1, 2) of one vocabulary size V -- decode together.  Each member gets its own features (BUTD / AoA
 * [B, R_m, D], NIC [B, E]); image b of every member's features is image b of the batch.  Optional weights w_m (finite, >= 0,
 * sum > 0; normalised to sum 1; NULL = uniform).  Every step, every row's combined log-probability is
 *     lp[v] = log( sum_m w_m softmax(logits_m)[v] )
 * (probabilities are averaged, not log-probabilities), computed as lse_m per member, then shifted by the largest term over m.
 *   greedy: argmax_v lp (ties to the lowest index, as torch.max) for max_len steps, no early stop; ids [B, max_len] int64.
 *   beam search: the shared search of icz_*_beam_search_diverse runs on lp (its row-top-k takes log_softmax of the row again,
 *   which leaves a normalised row's selections unchanged); every option holds, the outputs are those of _diverse.
 * The ensemble does not own its members: they stay alive, bound and refreshed while it decodes; an AoA member's region counts are
 * those of its last icz_aoa_set_regions.  A decode runs each member's step on one stream, then the combine kernel; beam search
 * re-gathers every member's state.  Training through an ensemble is out of scope; its sampling decode is declared below, behind
 * icz_sample_opts.
 * Argument errors return ICZ_ERR_INVALID before any device work: create -- M outside 1..4, a null array, an unknown kind, a null
 * or repeated member, a bad weight, members of different V; decode -- the options (as _diverse, checked first), a null handle, null
 * features, an unrefreshed member, B (greedy) or n_img x beam (beam) above any member's row capacity.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct icz_ensemble icz_ensemble_t;
int icz_ensemble_create(const int32_t* kinds, void* const* members, const float* weights, int32_t M, icz_ensemble_t** out);
int icz_ensemble_destroy(icz_ensemble_t* h);
/* feats: HOST array of M device pointers */
int icz_ensemble_greedy(icz_ensemble_t* h, const float* const* feats, int32_t B, int32_t max_len, int64_t* ids_out, void* stream);
int icz_ensemble_beam_search_diverse(icz_ensemble_t* h, const float* const* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                                     const icz_beam_opts* opts, const icz_beam_diversity* div, float* seqs_out, int32_t* lens_out,
                                     float* scores_out, void* stream);
/* The constrained search of icz_beam_constraints (see icz_butd_beam_search_constrained) on the combined log-probabilities: the same
 * specification, outputs and order of argument errors, with the ensemble's features (a HOST array of M device pointers) and, behind
 * the null handle, the member checks of the other decode entries on n_img * 2^C * beam rows.  An ensemble of one member runs the
 * member's own search (its weight normalises to 1): the result is icz_<family>_beam_search_constrained's bit for bit, and its handle
 * errors are the family's. */
int icz_ensemble_beam_search_constrained(icz_ensemble_t* h, const float* const* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                                         const icz_beam_opts* opts, const icz_beam_constraints* cons, float* seqs_out, int32_t* lens_out,
                                         float* scores_out, int32_t* sat_out, void* stream);
/* The combine kernel on its own (tests): member m's logits are finished rows [rows][ld_m] (nsplit 1) or nsplit split-K slabs
 * [nsplit][rows][ld_m] summed in slab order + bias_m.  lp_out [rows][ldo] receives lp; or, argmax_out != NULL, the greedy variant
 * writes each row's argmax there instead.  Host arrays of device pointers; bias may be NULL when every nsplit is 1. */
int icz_ensemble_logprob(int32_t M, const float* const* logits, const float* const* bias, const int32_t* nsplit, const int32_t* ld,
                         const float* weights, int32_t rows, int32_t V, float* lp_out, int32_t ldo, int64_t* argmax_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Sampling decode (beyond the reference; self-critical.pytorch's sample_method / temperature / top-k / top-p): n = 1..8 captions
 * per image drawn in EVALUATION mode (dropout off, nothing kept for a backward pass), decoder row = img * n + j.  The per-image
 * work runs once per image.  At every step, for every unfinished row with finished logits x [V]:
 *   1. y = x / temperature (temperature > 0, finite), evaluated in float64.
 *   2. top-k (top_k = 0: off; else 1..V): the top_k largest y survive; ties at the cut go to the LOWEST token index, so exactly
 *      top_k tokens survive.
 *   3. nucleus (top_p = 1: off; else 0 < top_p < 1): q = softmax(y over the survivors); tokens ordered by q descending, ties to
 *      the lowest index; a token survives while the mass of the tokens before it is < top_p (the largest always survives).
 *   4. the draw is the sampler contract of icz_butd_sample over the survivors' masses exp(y - max y) (a filtered token carries
 *      mass 0): the smallest token index v, in vocabulary order, with cumsum(mass)[v] > u * sum(mass), sums in float64.
 *   5. logp_out[row, t] = log_softmax(x)[token] -- the model's own log-probability (temperature 1, unfiltered), the quantity
 *      the beam scores are; score_out[row] = their fp32 sum in step order.
 *   6. a drawn <end> (2) is recorded with its log-probability and finishes the row: behind it ids are 0 and log-probs 0.  Once
 *      every row has finished, the kernels of the remaining steps return at entry (the early-out of the rollouts).
 * The order of steps 2 and 3 is the order of x: x -> x / temperature is monotone.  The nucleus cut is found on masses held as
 * 2^-40 fixed-point integers (integer sums are the same in any order); the draw's float64 sums run in one fixed order: one seed
 * gives the same bits run to run.
 * Uniforms: `uniforms` [max_len, n_img n] in [0, 1) (tests), or NULL = Philox keyed by (seed, step, row) under a stream tag of
 * its own (no other stream changes).  ids_out [n_img n, max_len] int64, logp_out [n_img n, max_len], score_out [n_img n].
 * An AoA handle decodes on the region counts of its last icz_aoa_set_regions.
 * Argument errors return ICZ_ERR_INVALID before any device work, in this order: null options, n outside 1..8, temperature <= 0 or
 * not finite, top_k < 0 or > V, top_p outside (0, 1], n_img n above the row capacity, null arguments, null handle.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    float temperature;   /* > 0, finite; 1 = the model's distribution */
    int32_t top_k;       /* 0 = off, else 1..V */
    float top_p;         /* (0, 1]; 1 = off */
} icz_sample_opts;
/* the argument rules above on the host alone (no handle, no device): V and max_rows are the handle's */
int icz_sample_decode_check(const icz_sample_opts* opts, int32_t n_img, int32_t n, int32_t V, int32_t max_rows);
int icz_butd_sample_decode(icz_butd_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, const icz_sample_opts* opts,
                           uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out, float* score_out, void* stream);
int icz_aoa_sample_decode(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, const icz_sample_opts* opts,
                          uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out, float* score_out, void* stream);
int icz_nic_sample_decode(icz_nic_t* h, const float* features, int32_t n_img, int32_t n, int32_t max_len, const icz_sample_opts* opts,
                          uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out, float* score_out, void* stream);
/* The filter-and-draw kernel on its own (tests): logits are finished rows [rows][ld] (nsplit 1) or nsplit split-K slabs
 * [nsplit][rows][ld] summed in slab order + bias.  uniforms [rows]; tok_out [rows] int64, logp_out [rows]; keep_out [rows][V]
 * (may be NULL) receives 1 for every token that survived the filters. */
int icz_sample_filter_draw(const float* logits, const float* bias, int32_t nsplit, int32_t ld, int32_t rows, int32_t V,
                           const icz_sample_opts* opts, const float* uniforms, int64_t* tok_out, float* logp_out, uint8_t* keep_out,
                           void* stream);

/* The sampling decode of a model ensemble: the rules above applied, per decoder row and step, to the combined row
 *     x[v] = lp[v] = log( sum_m w_m softmax(logits_m)[v] )
 * of icz_ensemble_logprob -- temperature divides lp, top-k and the nucleus are cut on it, logp_out is lp[token] - lse(lp) (lp is
 * normalised up to rounding).  Row img * n + j is sample j of image img; every member runs its per-image work once per image and its
 * step over all n_img n rows on the shared tokens; then one launch combines the members' logits (read as finished rows or split-K
 * slabs, the combined row held in LDS only), filters, draws and writes every member's next input embedding.  The Philox uniforms
 * are keyed by (seed, step, row) as in icz_*_sample_decode: a one-member ensemble and its member see the same uniforms.  feats: HOST
 * array of M device pointers; every other argument as in icz_butd_sample_decode (uniforms [max_len, n_img n] or NULL).
 * Argument errors return ICZ_ERR_INVALID before any device work, in this order: the options (as above, without the capacity), null
 * arguments, null handle, n_img n above the smallest member's row capacity, null features of a member or a member not refreshed. */
int icz_ensemble_sample_decode(icz_ensemble_t* h, const float* const* feats, int32_t n_img, int32_t n, int32_t max_len,
                               const icz_sample_opts* opts, uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out,
                               float* score_out, void* stream);
/* The ensemble instance of the filter-and-draw kernel on its own (tests), the counterpart of icz_sample_filter_draw and
 * icz_ensemble_logprob: M = 1..4 members' logits as in icz_ensemble_logprob (host arrays of device pointers; bias may be NULL when
 * every nsplit is 1), weights as in icz_ensemble_create; uniforms [rows]; tok_out [rows] int64; logp_out [rows] = lp[token] -
 * lse(lp); keep_out [rows][V] (may be NULL) receives 1 for every token that survived the filters.  Errors: the options first, then M,
 * null / bad arguments, the weights, each member's view. */
int icz_ensemble_sample_filter_draw(int32_t M, const float* const* logits, const float* const* bias, const int32_t* nsplit,
                                    const int32_t* ld, const float* weights, int32_t rows, int32_t V, const icz_sample_opts* opts,
                                    const float* uniforms, int64_t* tok_out, float* logp_out, uint8_t* keep_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Scoring given captions (beyond the reference; self-critical.pytorch's eval_split reports the perplexity this gives): the
 * log-probability a model, or an ensemble, assigns to captions it is GIVEN -- teacher forcing in EVALUATION mode (dropout off,
 * nothing kept for a backward pass).  Decoder row r = img * n + j scores caption j of image img; n = 1..8 captions per image,
 * n_img n within the handle's row capacity.  The per-image work runs once per image (NIC's image step once per image, expanded
 * to its n rows).  ids [n_img n, max_len] int64 in the format icz_*_sample_decode / icz_*_greedy WRITE: no leading <sta>, <end> (2)
 * included, 0 behind it.  For row r with caption c = ids[r, :]:
 *   1. len(r), the number of scored tokens: the index of the first 2 plus one if a 2 occurs before any 0; else the index of the
 *      first 0; else max_len.  Whatever lies behind len(r) is ignored; an empty caption (c[0] = 0) is legal.  A token id outside
 *      [0, V) ends the row as a 0 does and is never used as an index.
 *   2. step t < len(r): the decoder is fed <sta> (1) at t = 0 and c[t-1] afterwards, and
 *          logp_out[r, t] = log_softmax(x_t)[c[t]]
 *      with x_t the row's finished logits (split-K slabs summed in slab order + bias) -- step 5 of the sampling contract above and
 *      the quantity the beam scores are.  For t >= len(r): logp_out[r, t] = 0.
 *   3. score_out[r] = the fp32 sum of logp_out[r, :len(r)] in step order (icz_*_sample_decode's score_out); 0 for an empty caption.
 *   4. an ensemble: logp = log( sum_m w_m softmax(logits_m)[c[t]] ), the definition of icz_ensemble_logprob, evaluated as
 *      log sum_m exp(log w_m + x_m[c[t]] - lse_m) shifted by the largest term: one pass over each member's logits for lse_m and the
 *      one logit; the combined row of V entries is never formed.
 *   5. a row past its length keeps running on <pad> (finite, never read); once every row is past its length the kernels of the
 *      remaining steps return at entry (the early-out of the sampling decode: the same per-step count of unfinished rows).
 * One launch per step behind the decoder step (score_tokens_kernel): the online max / sum-exp over V (fp32 terms, float64 sums),
 * the target's logit, logp and the running score, the finished flag and the count, and every member's next input embedding.  No row
 * is held in LDS: there is no cap on V.  Reduction orders are fixed and there are no float atomics: two runs give the same bits.
 * An AoA handle scores on the region counts of its last icz_aoa_set_regions.
 * Argument errors return ICZ_ERR_INVALID before any device work, in this order: n outside 1..8, max_len outside 1..256, n_img <= 0
 * or n_img n above the (smallest member's) row capacity, null arguments, null handle, an unrefreshed member or null member features.
 * ---------------------------------------------------------------------------------------------------------- */
/* the host-only argument rules above (no handle, no device): max_rows is the handle's row capacity */
int icz_score_captions_check(int32_t n_img, int32_t n, int32_t max_len, int32_t max_rows);
/* Score ids under one decoder: logp_out [n_img n, max_len], score_out [n_img n]. */
int icz_butd_score_captions(icz_butd_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, const int64_t* ids,
                            float* logp_out, float* score_out, void* stream);
int icz_aoa_score_captions(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, const int64_t* ids,
                           float* logp_out, float* score_out, void* stream);
int icz_nic_score_captions(icz_nic_t* h, const float* features, int32_t n_img, int32_t n, int32_t max_len, const int64_t* ids,
                           float* logp_out, float* score_out, void* stream);
/* Score ids under an ensemble (rule 4): every member steps on the shared fed tokens, then one launch scores the row from all
 * members' logits and writes every member's next input embedding.  feats: HOST array of M device pointers. */
int icz_ensemble_score_captions(icz_ensemble_t* h, const float* const* feats, int32_t n_img, int32_t n, int32_t max_len,
                                const int64_t* ids, float* logp_out, float* score_out, void* stream);
/* score_tokens_kernel on its own (tests), the counterpart of icz_sample_filter_draw: logits are finished rows [rows][ld] (nsplit 1)
 * or nsplit split-K slabs [nsplit][rows][ld] summed in slab order + bias; targets [rows] int64; logp_out [rows] =
 * log_softmax(row)[target] (0 for a target outside [0, V), which is never used as an index). */
int icz_score_tokens(const float* logits, const float* bias, int32_t nsplit, int32_t ld, int32_t rows, int32_t V,
                     const int64_t* targets, float* logp_out, void* stream);
/* The ensemble instance on its own (tests), the counterpart of icz_ensemble_sample_filter_draw: M = 1..4 members' logits and
 * weights as in icz_ensemble_logprob (host arrays of device pointers; bias may be NULL when every nsplit is 1); logp_out [rows] =
 * log( sum_m w_m softmax(logits_m)[target] ).  Errors: M, null / bad arguments, the weights, each member's view. */
int icz_ensemble_score_tokens(int32_t M, const float* const* logits, const float* const* bias, const int32_t* nsplit,
                              const int32_t* ld, const float* weights, int32_t rows, int32_t V, const int64_t* targets,
                              float* logp_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Sampling without replacement: stochastic beam search (beyond the reference; Kool, van Hoof and Welling, "Stochastic Beams and
 * Where to Find Them", ICML 2019).  n = 1..8 DISTINCT captions per image that are exactly a sample without replacement from the
 * model's (tempered) sequence distribution, for the cost of one beam search of width n, with the perturbed values the unbiased
 * without-replacement estimators need (Kool et al., ICLR 2020).  EVALUATION mode; csrc/stochastic_beam.hip, csrc/sbs_kernels.h.
 * Per image there are n slots; decoder row img * n + slot holds a hypothesis: its tokens, phi (the fp32 running sum of its token
 * log-probs in step order, as the beam search's running score), G (its perturbed value, float64) and a frozen flag, set once it
 * has emitted <end> (2).  The occupied slots are kept sorted by G descending after every step: slot 0 is the best.
 *   1. Root: phi = 0, G_root = gumbel(u_root[img]) with gumbel(u) = -log(-log(u)); only slot 0 is occupied.  Step 1 runs one decoder
 *      row per image where every member allows it (the beam search's compact step).
 *   2. Row scoring, for a live (occupied, not frozen) row at step s = 1, 2, ... with finished logits x (split-K slabs summed in
 *      slab order + bias):  lp[v] = x[v] / T - lse(x / T);  phi_c[v] = phi + lp[v] (fp32);  g[v] = phi_c[v] + gumbel(u[s, img, slot, v])
 *      (fp32).  The row emits its min(n, V) largest g with phi_c and v, ties to the lower v; Z = the row maximum of g.  A token whose
 *      g is -inf is never emitted: a row may emit fewer than n.
 *   3. Conditioning on the parent, in float64 with Tp = the parent's G:  w = Tp - g + log1mexp(g - Z);
 *      G~ = Tp - max(0, w) - log1p(exp(-|w|)) -- the stable form of -log(exp(-Tp) - exp(-Z) + exp(-g)); the row's argmax gets exactly
 *      Tp.  The map is monotone in g, so only the emitted candidates are ever transformed.  A frozen row emits one candidate: itself,
 *      with G, phi and tokens unchanged and next input <pad>; its logits are never read.
 *   4. Merge, per image: of the <= n n candidates the n largest G~ become the new slots 0 .. n-1 in that order, ties to the lower
 *      (parent slot, v) (a frozen parent counts as v = 0).  A candidate whose token is <end> is frozen on entry.  The step also counts
 *      the occupied slots per image and, over all images, the rows that are occupied and not frozen: every third step from step 6
 *      on one 4-byte read-back ends the search once that count is 0 (the result is that of all max_len steps).
 *   5. After max_len steps the outputs per image are in slot order, G descending (icz_sample_distinct_out): ids [n_img n, max_len]
 *      int64 in the format icz_*_sample_decode writes (no <sta>, <end> included, 0 behind it), lens, finished (0 for a hypothesis cut
 *      at max_len), phi fp32 and g float64.  An unoccupied slot (an image with fewer than n sequences: only at toy vocabularies)
 *      writes length 0, finished 0, phi = g = -inf and zeros.  <pad> (0) is a token like any other and may be sampled inside a
 *      caption: in ids it cannot be told from the padding, only lens says where the caption ends.  icz_*_score_captions and the
 *      Engine's caption strings end a caption at its first 0, so such a hypothesis is scored and printed up to there only -- its phi is
 *      the whole sequence's -- and two distinct hypotheses may print as one string.  A trained model gives <pad> no mass to speak of.
 *   6. Noise: uniforms == NULL: Philox4x32-10 with counter {v >> 2, img * 8 + slot, step, 8} (stream tag 8, no other stream changes),
 *      key = seed, word v & 3, and u = ((r >> 9) + 0.5) * 2^-23, exact in fp32 and strictly inside (0, 1); the root uses step 0, slot 0,
 *      v = 0.  `img` in the counter is first_image + the image's index in the call (first_image >= 0, first_image + n_img <= 2^28): a batch
 *      decoded in chunks with first_image = the chunk's offset draws the noise of the whole batch.  The slot stride is the constant 8, not n: since slots are sorted, the first j hypotheses of a run are the run with
 *      n = j on the same seed.  Explicit noise (tests): uniforms [max_len, n_img, n, V] fp32 and root_uniforms [n_img], every value
 *      strictly inside (0, 1); both or neither.
 *   7. Temperature T > 0, finite, is the only option: phi is the log-probability under the tempered distribution, the one sampled
 *      from.  Top-k, nucleus, n-gram blocking and length penalties would change what "without replacement from the model" means.
 * Reduction orders are fixed and no float is accumulated atomically: one seed gives the same bits run to run.  An ensemble samples
 * from x = lp of icz_ensemble_logprob (the combined rows); an ensemble of one member runs that member's own search, bit for bit.
 * Argument errors return ICZ_ERR_INVALID before any device work, in this order: (1) n outside 1..8 or above V, (2) a temperature
 * that is not finite or not positive, (3) max_len outside 1..256, (4) null arguments, exactly one of uniforms / root_uniforms
 * included, (5) a null handle, (6) n_img <= 0 or n_img n above the (smallest member's) row capacity, or first_image out of range, (7) unrefreshed weights (an
 * ensemble: null features of a member, a member not refreshed or short of rows).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t* ids;        /* [n_img n, max_len] */
    int32_t* lens;       /* [n_img n] */
    int32_t* finished;   /* [n_img n] */
    float* phi;          /* [n_img n] */
    double* g;           /* [n_img n] */
} icz_sample_distinct_out;
/* rules 1 - 3 and 6 above on the host alone (no handle, no device): V and max_rows are the handle's */
int icz_sample_distinct_check(int32_t n_img, int32_t n, int32_t max_len, float temperature, int32_t V, int32_t max_rows);
int icz_butd_sample_distinct(icz_butd_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, float temperature, uint64_t seed,
                             int32_t first_image, const float* uniforms, const float* root_uniforms, const icz_sample_distinct_out* out,
                             void* stream);
int icz_aoa_sample_distinct(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, float temperature, uint64_t seed,
                            int32_t first_image, const float* uniforms, const float* root_uniforms, const icz_sample_distinct_out* out,
                            void* stream);
int icz_nic_sample_distinct(icz_nic_t* h, const float* features, int32_t n_img, int32_t n, int32_t max_len, float temperature, uint64_t seed,
                            int32_t first_image, const float* uniforms, const float* root_uniforms, const icz_sample_distinct_out* out,
                            void* stream);
/* feats: HOST array of M device pointers */
int icz_ensemble_sample_distinct(icz_ensemble_t* h, const float* const* feats, int32_t n_img, int32_t n, int32_t max_len, float temperature,
                                 uint64_t seed, int32_t first_image, const float* uniforms, const float* root_uniforms,
                                 const icz_sample_distinct_out* out, void* stream);
/* The kernels alone (tests), launched with the grids of the search.  Rows: img * n + slot.  logits: finished rows [R][ld] (nsplit 1) or
 * nsplit split-K slabs [nsplit][R][ld] + bias, R = n_img n, or n_img when compact (step 1 only).  occ [n_img], frozen [rows] uint8, phi
 * [rows]; uniforms [n_img, n, V] of this step or NULL (Philox: seed, step); cand_g / cand_phi / cand_idx [rows, 8]: the first n entries
 * of every scored row are written (an empty entry: idx -1, g = phi = -inf), nothing else. */
int icz_test_sbs_rowtopk(const float* logits, const float* bias, int32_t nsplit, int32_t ld, int32_t n_img, int32_t n, int32_t V, int32_t step,
                         int32_t compact, float temperature, const int32_t* occ, const uint8_t* frozen, const float* phi,
                         const float* uniforms, uint64_t seed, int32_t first_image, float* cand_g, float* cand_phi, int32_t* cand_idx,
                         void* stream);
/* The state one step reads and writes: the row kernel, then the merge.  occ, frozen, phi, G [rows] float64 and len [rows] are
 * rewritten in place; seqs_in / seqs_out [rows, L] (tokens without <sta>); src_row [rows], it_next [rows] int64; n_live [1] is
 * incremented by the rows occupied and not frozen after the step. */
typedef struct {
    const float* logits; const float* bias; const float* uniforms;
    int32_t* occ; uint8_t* frozen; float* phi; double* G; int32_t* len;
    const int32_t* seqs_in; int32_t* seqs_out; int32_t* src_row; int64_t* it_next; int32_t* n_live;
    float* cand_g; float* cand_phi; int32_t* cand_idx;
} icz_sbs_step_state;
int icz_test_sbs_step(const icz_sbs_step_state* s, int32_t nsplit, int32_t ld, int32_t n_img, int32_t n, int32_t V, int32_t step, int32_t L,
                      int32_t compact, float temperature, uint64_t seed, int32_t first_image, void* stream);
/* the start state (rule 1) of n_img images: root_uniforms [n_img] or NULL (Philox); it [rows] int64, img_of_row / src_row [rows] */
int icz_test_sbs_init(int32_t n_img, int32_t n, const float* root_uniforms, uint64_t seed, int32_t first_image, int32_t* occ, uint8_t* frozen,
                      float* phi, double* G,
                      int32_t* len, int64_t* it, int32_t* img_of_row, int32_t* src_row, void* stream);
/* the outputs (rule 5) of a given state; seqs [rows, L] */
int icz_test_sbs_finalize(int32_t n_img, int32_t n, int32_t L, const int32_t* occ, const uint8_t* frozen, const float* phi, const double* G,
                          const int32_t* len, const int32_t* seqs, const icz_sample_distinct_out* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Word-level knowledge distillation (beyond the reference): the XE training step of one student decoder on the word distribution of
 * an ensemble of M = 1..4 teachers of the same vocabulary (csrc/distill.hip).  For a token row with student logits s, teacher logits
 * z_1..z_M, normalised weights w, target c, label smoothing sigma, mixing weight alpha in [0, 1] and temperature tau in [0.25, 8]:
 *     q[v]  = sum_m w_m softmax(z_m / tau)[v]                  (the probabilities averaged, as the ensemble decodes)
 *     hard  = LabelSmoothingLoss(s, c; sigma)                  (the per-row term of icz_*_xe_backward)
 *     kd    = tau^2 KL(q || softmax(s / tau)) = tau^2 sum_v q[v] (log q[v] - log_softmax(s / tau)[v])     (terms with q[v] = 0 are 0)
 *     loss  = ((1 - alpha) sum_rows hard + alpha sum_rows kd) / N
 *     d s   = ((1 - alpha) (softmax(s) - true) + alpha tau (softmax(s / tau) - q)) / N
 * N is the token normaliser of icz_*_xe_backward: the local token count, n_tokens_global > 0, or (n_tokens_global < 0) the device
 * scalar of icz_*_set_norm_global.  teacher[m] is a device tensor [N_tokens, ld[m]] of packed logits in the order of
 * packed_logits_out -- what the teacher's icz_*_xe_forward(train = 0, packed_logits_out) writes for the same captions and lengths;
 * ld[m] >= V lets the caller pad the rows to a 16-byte multiple (ld = V = 10 102 is not one; unaligned rows take a scalar path).
 * teacher, ld and weights are HOST arrays; weights NULL = uniform, else the rules of icz_ensemble_create; a member of weight 0 is
 * never read.  One launch (distill_loss_dlogits_kernel) replaces the loss kernel of icz_*_xe_backward: one workgroup per (b, t), an
 * online max / sum-exp per row in pass 1, q formed in registers in pass 2 (never written to memory), d s written over the stored
 * logits; every exponent is taken behind its row's maximum; per-row losses are summed in fixed order, no float atomics: two runs give
 * the same bits.  loss_out3 = {loss, sum hard / N, sum kd / N} (device).
 * alpha = 0 runs the launches of icz_*_xe_backward (bit for bit its gradients and loss; no teacher is read).
 * Errors return ICZ_ERR_INVALID before any device work, in this order: 1. null opts; 2. M outside 1..4; 3. alpha; 4. temperature;
 * 5. smoothing outside [0, 1); 6. null teacher or ld, or a null member; 7. ld[m] < V; 8. the weights; 9. null grads or loss;
 * 10. null handle; 11. no XE forward stored; 12. the stored forward ran with scheduled sampling (ss_prob > 0): the teachers were fed
 * other tokens than the student (also at alpha = 0).  (With a null handle V is unknown and rule 7 is not applied.)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t M;
    const float* const* teacher;
    const int32_t* ld;
    const float* weights;          /* NULL = uniform */
    float alpha, temperature, smoothing;
} icz_distill_opts;
/* rules 1 - 8 above on their own (host only: no handle, no device) */
int icz_distill_check(const icz_distill_opts* opts, int32_t V);
/* icz_*_xe_backward with the distillation loss in the place of LabelSmoothingLoss (for AoA with the refiner's backward pass when
 * train_refiner is on; for NIC with dfeatures_out [B, E] or NULL). */
int icz_butd_xe_backward_distill(icz_butd_t* h, const icz_distill_opts* opts, const icz_butd_params* grads, float* loss_out3,
                                 float n_tokens_global, void* stream);
int icz_aoa_xe_backward_distill(icz_aoa_t* h, const icz_distill_opts* opts, const icz_aoa_params* grads, float* loss_out3,
                                float n_tokens_global, void* stream);
int icz_nic_xe_backward_distill(icz_nic_t* h, const icz_distill_opts* opts, const icz_nic_params* grads, float* dfeatures_out,
                                float* loss_out3, float n_tokens_global, void* stream);
/* The kernel alone (tests, tools): student [rows, ld_s], the teachers' rows [rows, ld[m]], targets [rows] int64 (one outside [0, V)
 * matches no column and is never used as an index), N = n_tokens > 0; dlogits_out [rows, ld_out] (columns [V, ld_out) are written
 * as zeros), loss_out3 as above.  alpha = 0 reads no teacher (kd = 0). */
int icz_distill_loss(const float* student, int32_t ld_s, const icz_distill_opts* opts, const int64_t* targets, int32_t rows, int32_t V,
                     float n_tokens, float* dlogits_out, int32_t ld_out, float* loss_out3, void* stream);
/* icz_butd_xe_backward_dlogits for the other two families: the backward pass of the stored XE forward driven by an upstream gradient
 * w.r.t. the packed logits [sum(lengths), V] (NIC: with dfeatures_out [B, E] or NULL). */
int icz_aoa_xe_backward_dlogits(icz_aoa_t* h, const float* dpacked, const icz_aoa_params* grads, void* stream);
int icz_nic_xe_backward_dlogits(icz_nic_t* h, const float* dpacked, const icz_nic_params* grads, float* dfeatures_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SCST objectives (beyond the reference; csrc/scst_objective.hip): what turns the sampled captions of a stored rollout into a gradient,
 * in the place of RewardCriterion in icz_*_sample_backward.
 *
 * Rows are r = img * K + k; a single-sample rollout has K = 1.  mask[r, 0] = 1 and mask[r, t] = seq[r, t - 1] > 0, as in
 * RewardCriterion.  M is sum(mask), or the global mask sum under the rules of icz_*_sample_backward: mask_sum_global > 0 is the global
 * sum given on the host side, < 0 takes the device scalar of icz_*_set_mask_sum_global / _set_norm_global, 0 uses the local sum.
 * p[r, t, :] is the softmax of the STORED training-mode logits of step t -- the distribution the token was drawn from, with dropout
 * applied; its log-sum-exp is stored beside the drawn token.
 *
 * Objective term, one of
 *   ICZ_SCST_REINFORCE (0): obj = -sum(logp * reward * mask) / M with reward [rows, T] float32 -- today's form; coef = d obj / d logp
 *     comes from reinforce_loss_kernel, unchanged.
 *   ICZ_SCST_RISK (1), K = 2..8, scores [rows] float64 (the CIDEr-D of every sample, laid out as icz_ciderd_reward_loo's scores_out),
 *     minimum-risk training: the expected cost under the model's distribution renormalised over the K samples.  With c_r = -scores[r]:
 *       s_r   = sum_t mask[r, t] * logp[r, t]        (the float32 logp values, summed in float64 in ascending t)
 *       Q_r   = exp(a s_r) / sum_{j in image} exp(a s_j)   (float64, shifted by the image's largest a s_j, j ascending)
 *       L_img = sum_k Q_k c_k
 *       obj   = (1 / N) sum_img L_img                (N = n_img_global if > 0, else the call's image count)
 *       coef[r, t] = mask[r, t] * a * Q_r * (c_r - L_img) / N     (stored as float32)
 *     a = risk_alpha must be finite and > 0.
 * Entropy term, for entropy_weight = b >= 0 (finite):
 *       H[r, t] = -sum_v p_v log p_v,   ent = sum(mask * H) / M,   loss = obj - b * ent.
 * The gradient written in place over the stored logits (pad columns [V, ldl) zero) is
 *       dlogits[row, v] = coef[r, t] * (1[v == draw] - p_v) + (b * mask[r, t] / M) * p_v * (log p_v + H[r, t])
 * with log p_v = logits[v] - lse[row].  A row with mask = 0, or draw < 0 (the evaluation-mode rows of a merged chain), becomes all
 * zeros WITHOUT BEING READ: steps behind the rollout's early-out hold stale data.
 *
 * Kernels: scst_risk_kernel (one wave per image, float64, fixed orders) + scst_risk_sum_kernel fill coef, obj and the mask sum;
 * scst_entropy_dlogits_kernel (b > 0; one 256-thread workgroup per stored row, two passes over the row with 16-byte loads, fp32 terms
 * and float64 sums in one fixed order, nothing kept in LDS: no cap on V) stands in for reinforce_dlogits_kernel; scst_finish_kernel
 * sums the per-row entropies in a fixed order.  No float atomics: two runs give the same bits.  Kind 0 with b = 0 runs the launches
 * of icz_*_sample_backward (bit for bit its gradients, loss and mask sum).
 * loss_out3 = {loss, obj, ent} (device floats); ent_out [rows, T] (optional) = mask * H.  With b = 0 no row is read for H: ent and
 * ent_out are reported as 0.
 *
 * icz_scst_objective_check returns ICZ_ERR_INVALID in this order: 1. null struct; 2. kind; 3. K outside 1..8 (risk: 2..8), or rows / T
 * not positive, or rows % K != 0; 4. risk_alpha not finite or <= 0 (both kinds); 5. entropy_weight not finite or < 0; 6. n_img_global
 * not finite or < 0; 7. the pointer the kind needs (reward / scores) null.  icz_*_sample_backward_objective applies rules 1 - 7 (rule 3
 * without the row count), then 8. null grads or loss_out3; 9. null handle; 10. no rollout stored; 11. rule 3 against the stored rows;
 * 12. a risk term whose K is not the stored rollout's (icz_*_sample_n's K, else 1).  Every refusal happens before anything is queued:
 * the stored rollout stays usable.
 * BUTD and AoA replay captured graphs as icz_*_sample_backward does; the key also carries kind, K, the bit patterns of risk_alpha,
 * entropy_weight and n_img_global, and the reward / scores / ent_out pointers.  BUTD with a gradient callback runs the loss head in
 * its first phase.  train_refiner, per-image region counts, the early-out and the global mask sum work as behind icz_*_sample_backward.
 * ---------------------------------------------------------------------------------------------------------- */
enum { ICZ_SCST_REINFORCE = 0, ICZ_SCST_RISK = 1 };
typedef struct {
    int32_t kind, K;
    float risk_alpha, entropy_weight, n_img_global;
    const float* reward;           /* kind 0: [rows, T] (device) */
    const double* scores;          /* kind 1: [rows] (device) */
} icz_scst_objective;
/* rules 1 - 7 above on their own (host only: no handle, no device) */
int icz_scst_objective_check(const icz_scst_objective* obj, int32_t rows, int32_t T);
int icz_butd_sample_backward_objective(icz_butd_t* h, const icz_scst_objective* obj, const icz_butd_params* grads, float* loss_out3,
                                       float* ent_out, float* mask_sum_out, float mask_sum_global, void* stream);
int icz_aoa_sample_backward_objective(icz_aoa_t* h, const icz_scst_objective* obj, const icz_aoa_params* grads, float* loss_out3, float* ent_out,
                                      float* mask_sum_out, float mask_sum_global, void* stream);
/* dfeatures_out [images, E] or NULL, as icz_nic_sample_backward */
int icz_nic_sample_backward_objective(icz_nic_t* h, const icz_scst_objective* obj, const icz_nic_params* grads, float* dfeatures_out,
                                      float* loss_out3, float* ent_out, float* mask_sum_out, float mask_sum_global, void* stream);
/* The kernels alone (tests, tools), in the shape of icz_test_reinforce: logp, seq, coef [B, T] (B = rows of the rollout);
 * mask_sum_global a device scalar or NULL; logits [T Bs', ldl] (Bs' = Bs or B), draw / lse [T Bs'], Bs > 0: Bs rows per step of which
 * [row0, row0 + B) are the rollout's.  loss_out3 [3]; ent_out [B, T] and mask_sum_out optional.  With entropy_weight > 0: ldl % 4 == 0
 * and 16-byte aligned logits.  Kind 0 with entropy_weight 0 is icz_test_reinforce. */
int icz_test_scst_objective(const icz_scst_objective* obj, const float* logp, const int64_t* seq, int32_t B, int32_t T,
                            const float* mask_sum_global, float* coef, float* loss_out3, float* ent_out, float* mask_sum_out, float* logits,
                            int32_t V, int32_t ldl, const int32_t* draw, const float* lse, int32_t Bs, int32_t row0, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SCST on without-replacement samples (beyond the reference; csrc/swor_objective.hip): the policy-gradient estimators of Kool, van
 * Hoof and Welling ("Buy 4 REINFORCE Samples, Get a Baseline for Free!", 2019; "Estimating Gradients for Discrete Random Variables
 * by Sampling without Replacement", ICLR 2020) on the n distinct captions per image of icz_*_sample_distinct at temperature 1, in the
 * place of LabelSmoothingLoss behind a TRAINING-MODE icz_*_xe_forward on those captions (dropout on, state kept for the backward pass).
 *
 * phi [images n] float32, G [images n] float64 and scores [images n] float64 (the CIDEr-D of every slot: icz_ciderd_reward_loo's
 * scores_out) are in icz_*_sample_distinct's row order img * n + slot, the slots of an image sorted by G descending.  Slot n - 1 is
 * only the threshold kappa = G[n - 1]; the m = n - 1 slots in front of it are the samples, n in 3..8.  In float64, sums in ascending
 * slot order:
 *     d_i = phi_i - kappa,   q_i = 1 - exp(-exp(d_i)) = -expm1(-exp(d_i)),
 *     log q_i = d_i - exp(d_i) / 2 where d_i < -18 (the series behind its first term: the next one is below exp(-36) / 24 < 1e-17)
 *     p_i = exp(phi_i),   w_i = p_i / q_i = exp(phi_i - log q_i),   W = sum_j w_j,   Bu = sum_j w_j f_j        (f = scores)
 *     ICZ_SWOR_NORMALISED (0):  c_i = w_i / (W - w_i + p_i) * (f_i - Bu / W)
 *     ICZ_SWOR_UNBIASED (1):    c_i = w_i * (f_i * (1 + w_i - p_i) - Bu)
 *     loss = -(1 / N) sum_img sum_{i < m} c_i logp_i,   logp_i = sum_{t < len_i} log softmax(z_{i,t})[y_{i,t}]
 *     d loss / d z[row, t, v] = -(c_row / N) * (1[v == y] - softmax(z)[v])
 * c is a constant of the backward pass.  N = n_img_global if > 0 (data-parallel: the all-reduced image count), else the call's image
 * count rows / (n - 1).  The weights use the sampler's evaluation-mode phi; logp and the gradient are the stored training-mode
 * forward's.  The threshold slot has c = 0 and takes no part in the forward pass: the stored forward holds rows = images (n - 1) rows,
 * sorted by decreasing length as icz_*_xe_forward wants them, and perm [rows] int32 (device) maps the sorted row b back to
 * img * n + slot.
 *
 * Kernels: swor_weights_kernel (one wave per image, lane = slot, float64) writes coef [images n] = -c / N as float32 and
 * stats_out [images, 3] float64 = {W, Bu / W, 1 / sum_j (w_j / W)^2 (the effective sample size)} (NULL: not wanted);
 * swor_dlogits_kernel (grid (B, T), 256 threads, the addressing of xe_loss_dlogits_kernel; an online max / sum-exp of the row with
 * 16-byte loads, the gradient written in place with zeros in the pad columns and in inactive rows; a row whose coefficient is exactly
 * 0 is written as zeros WITHOUT BEING READ; nothing of the row is kept in LDS: no cap on V) leaves the target's log-prob of every
 * (b, t) in loss_rows (0 for a row that was not read); swor_finish_kernel sums in one fixed order to
 * loss_out [1 + images] = {loss, sum_i (-c_i / N) logp_i of every image}.  No float atomics: two runs give the same bits.  In the
 * softmax rows every exponent is taken behind its row's maximum.
 *
 * Errors return ICZ_ERR_INVALID before anything is queued, in this order: 1. null opts; 2. n outside 3..8; 3. an unknown estimator;
 * 4. n_img_global not finite or < 0; 5. rows < 1 or not a multiple of n - 1; 6. null phi, G, scores or perm; then for
 * icz_*_xe_backward_swor 7. null grads or loss_out; 8. null handle; 9. no XE forward stored; 10. the stored forward ran in evaluation
 * mode; 11. it ran with scheduled sampling (ss_prob > 0): it was fed other tokens than the sampled captions; 12. rows is not the
 * stored forward's row count.  A refused call leaves the stored forward usable.
 * icz_swor_check applies rules 1 - 6 and then, on the host copies it is given (each may be NULL), 7'. perm_host [rows]: every entry
 * inside [0, images n), no threshold slot, none twice; 8'. lengths_host [rows]: >= 1 and sorted in decreasing order.  (On the device a
 * perm entry outside [0, images n) is never used as an index: its row counts as one of coefficient 0.)
 * ---------------------------------------------------------------------------------------------------------- */
enum { ICZ_SWOR_NORMALISED = 0, ICZ_SWOR_UNBIASED = 1 };
typedef struct {
    int32_t n, estimator;
    float n_img_global;
    const float* phi;              /* [images n] (device) */
    const double* G;               /* [images n] (device) */
    const double* scores;          /* [images n] (device) */
    const int32_t* perm;           /* [rows] (device) */
    double* stats_out;             /* [images, 3] (device) or NULL */
} icz_swor_opts;
int icz_swor_check(const icz_swor_opts* opts, int32_t rows, const int32_t* perm_host, const int32_t* lengths_host);
/* icz_*_xe_backward with this loss head (for AoA with the refiner's backward pass when train_refiner is on; for NIC with
 * dfeatures_out [rows, E] or NULL); loss_out [1 + rows / (n - 1)] */
int icz_butd_xe_backward_swor(icz_butd_t* h, const icz_swor_opts* opts, int32_t rows, const icz_butd_params* grads, float* loss_out,
                              void* stream);
int icz_aoa_xe_backward_swor(icz_aoa_t* h, const icz_swor_opts* opts, int32_t rows, const icz_aoa_params* grads, float* loss_out, void* stream);
int icz_nic_xe_backward_swor(icz_nic_t* h, const icz_swor_opts* opts, int32_t rows, const icz_nic_params* grads, float* dfeatures_out,
                             float* loss_out, void* stream);
/* The kernels alone (tests, tools), in the shape of icz_test_xe_loss: logits [T B, ldl] (ldl % 4 == 0, 16-byte aligned; the gradient is
 * written over it), captions [B, L] int64 with L > T (the target of (b, t) is captions[b, t + 1]; one outside [0, V) matches no column
 * and is never used as an index), rows_t [T] a HOST array; coef_out [B / (n - 1) * n], loss_rows [T B], loss_out [1 + B / (n - 1)]. */
int icz_test_swor_objective(const icz_swor_opts* opts, float* logits, int32_t V, int32_t ldl, const int64_t* captions, int32_t L, int32_t B,
                            int32_t T, const int32_t* rows_t, float* coef_out, float* loss_rows, float* loss_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimiser step: clip_gradient (Utils.py:241-250, value clamp) + torch.optim.Adam(betas=(0.9,0.999),
 * eps=1e-8, weight_decay=0) (Utils.py:219-220) fused, one call per parameter tensor.
 * ---------------------------------------------------------------------------------------------------------- */
int icz_adam_clamp_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                        float lr, float clip, int32_t step, void* stream);
/* The same update for `count` (<= 32) tensors in one launch; the pointer arrays are HOST arrays of device pointers. */
int icz_adam_clamp_multi(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                         float* const* exp_avg_sq, const int64_t* numel, float lr, float clip, int32_t step, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * CIDEr-D reward (Utils.py:319-367 get_self_critical_reward -> ciderD.py:30-55 -> ciderD_scorer.py:127-206)
 * The document-frequency table and the cooked references are built once on the host by the Python side
 * (they depend on strings) and uploaded as flat arrays; scoring runs on the device in float64.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct icz_ciderd icz_ciderd_t;

/* df table: open-addressing hash of n-grams of token ids.  keys [cap,4] int32 (unused slots -1-filled, n-gram
 * right-padded with -1), idf [cap] float64 = log(ref_len) - log(max(1, df)); cap is a power of two.
 * default_idf = log(ref_len) (n-gram absent from the table).  penalty [64] float64: exp(-d^2/(2 sigma^2)) for
 * |delta| = 0..63 computed on the host exactly as the reference does.  The three arrays are DEVICE arrays owned
 * by the caller and must outlive the handle. */
int icz_ciderd_create(const int32_t* df_keys, const double* df_idf, int64_t cap, double default_idf,
                      const double* penalty, icz_ciderd_t** out);
int icz_ciderd_destroy(icz_ciderd_t* h);

/* Cooked references of a batch, CSR over images -> refs -> n-gram entries:
 *   img_ref_ptr [B+1]; ref_ent_ptr [n_refs+1]; ent_key [n_ent,4] int32; ent_order [n_ent] int32 (1..4);
 *   ent_w [n_ent] float64 tf-idf weight; ref_norm [n_refs,4] float64; ref_len [n_refs] int32 (bigram count).
 * gen [B,T] int64 = sampled ids (sample_rl semantics), greedy [B,T] int64.  reward_out [B,T] float32 =
 * (CIDEr-D(sample) - CIDEr-D(greedy)) broadcast over T.  scores_out [2B] float64 or NULL. */
int icz_ciderd_reward(icz_ciderd_t* h, const int64_t* gen, const int64_t* greedy, int32_t B, int32_t T,
                      const int32_t* img_ref_ptr, const int32_t* ref_ent_ptr, const int32_t* ent_key,
                      const int32_t* ent_order, const double* ent_w, const double* ref_norm,
                      const int32_t* ref_len, float* reward_out, double* scores_out, void* stream);
/* Host-side cooking of references (ciderD_scorer.py:17-32, 128-153) from token ids into the flat arrays above -- pure host code,
 * HOST pointers throughout.  df_keys_host / df_idf_host: the table of icz_ciderd_create in host memory (it must then also hold
 * the n-grams that contain out-of-vocabulary words, under the private ids the caller gives those words).  tokens: the token
 * ids of n_refs references back to back, reference r = tokens[ref_tok_ptr[r] .. ref_tok_ptr[r+1]).  Outputs sized by the
 * caller (max_ent entries; at most 4 * tokens in all): ref_ent_ptr_out [n_refs+1] counts from 0. */
int icz_ciderd_cook_host(const int32_t* df_keys_host, const double* df_idf_host, int64_t cap, double default_idf,
                         const int32_t* tokens, const int32_t* ref_tok_ptr, int32_t n_refs, int64_t max_ent,
                         int32_t* ent_key_out, int32_t* ent_order_out, double* ent_w_out, int32_t* ref_ent_ptr_out,
                         double* ref_norm_out, int32_t* ref_len_out, int64_t* n_ent_out);
/* Host-side word -> id map of the scorer: the caption vocabulary (Caption_Vocabulary.word2ix, ClassRepository/CaptionVocabClass.py:1-19)
 * plus private ids >= V, in order of first appearance, for words outside it (references and the document-frequency table contain
 * them; ciderD_scorer.py keys n-grams by the word strings themselves).  words: n_words strings back to back, word i =
 * words[word_off[i] .. word_off[i+1]) with id word_id[i].  Thread-safe. */
typedef struct icz_ciderd_vocab icz_ciderd_vocab_t;
int icz_ciderd_vocab_create(const char* words, const int64_t* word_off, const int32_t* word_id, int32_t n_words, int32_t V,
                            icz_ciderd_vocab_t** out);
int icz_ciderd_vocab_destroy(icz_ciderd_vocab_t* v);
int icz_ciderd_vocab_oov_id(icz_ciderd_vocab_t* v, const char* word, int32_t len, int32_t* id_out);
/* icz_ciderd_cook_host with `precook`'s tokenisation (ciderD_scorer.py:17-32: s.split()) in front of it: text = n_refs ASCII
 * references separated by '\n', words by runs of blanks.  Outputs as icz_ciderd_cook_host (at most 4 * words entries). */
int icz_ciderd_cook_text(icz_ciderd_vocab_t* vocab, const int32_t* df_keys_host, const double* df_idf_host, int64_t cap, double default_idf,
                         const char* text, int64_t text_len, int32_t n_refs, int64_t max_ent,
                         int32_t* ent_key_out, int32_t* ent_order_out, double* ent_w_out, int32_t* ref_ent_ptr_out,
                         double* ref_norm_out, int32_t* ref_len_out, int64_t* n_ent_out);
/* The same against a device-resident STORE of cooked references (every image of the dataset cooked once, instead of the
 * reference's re-cooking of the batch's references on every call, ciderD.py:41-52): the seven arrays are the store's, laid
 * out as above with one CSR row per stored image, and img_slot [B] int32 (device) names the store row of image b of the
 * batch -- the only per-batch upload. */
int icz_ciderd_reward_indexed(icz_ciderd_t* h, const int64_t* gen, const int64_t* greedy, int32_t B, int32_t T,
                              const int32_t* img_slot, const int32_t* img_ref_ptr, const int32_t* ref_ent_ptr,
                              const int32_t* ent_key, const int32_t* ent_order, const double* ent_w, const double* ref_norm,
                              const int32_t* ref_len, float* reward_out, double* scores_out, void* stream);
/* Beyond the reference (Utils.py:319-367 baselines a sampled caption with the greedy one): the reward of the multi-sample SCST
 * variant with a leave-one-out mean baseline.  gen [B K, T] holds K sampled captions per image (row = img * K + k, K = 2..8),
 * img_slot [B] the store row of each IMAGE, the store arrays as in icz_ciderd_reward_indexed.  scores_out [B K] float64 receives
 * the CIDEr-D scores s_i; reward_out [B K, T] every column of row i = (float)(s_i - (sum_{j != i, ascending j} s_j) / (K - 1)),
 * computed in float64, the sum over the other K - 1 captions of the same image. */
int icz_ciderd_reward_loo(icz_ciderd_t* h, const int64_t* gen, int32_t B, int32_t K, int32_t T, const int32_t* img_slot,
                          const int32_t* img_ref_ptr, const int32_t* ref_ent_ptr, const int32_t* ent_key, const int32_t* ent_order,
                          const double* ent_w, const double* ref_norm, const int32_t* ref_len, float* reward_out, double* scores_out,
                          void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Caption sets (beyond the reference): K candidate captions per image, as n-best lists, diverse beams, ensembles and the sampling
 * decode produce them, scored against EACH OTHER -- consensus (minimum-Bayes-risk) reranking -- and counted for the diversity
 * metrics of a set report (Div-n, mBLEU, mean pairwise CIDEr-D).  Candidates arrive as int32 DEVICE arrays in CSR form, as for
 * icz_bleu_stats: candidate c = img * K + k is tok[ptr[c] .. ptr[c+1]), token ids >= 0, every token a word (no <sta>, <end> or
 * <pad> unless the caller wants them counted), at most 60 tokens (the caller checks), empty candidates are legal.  Argument
 * errors return ICZ_ERR_INVALID before any device work, in the order K, n_img, null arrays, null handle.  No atomics and fixed
 * summation orders: two runs give the same bits.
 * ---------------------------------------------------------------------------------------------------------- */
/* icz_ciderd_cook_host on the device, against the handle's df table: one workgroup per candidate; entries in the scorer's
 * dict-insertion order (order k = 1..4, first occurrence ascending), weight = (double)tf * idf, norms = sqrt of the squares summed
 * in that order, length = number of bigrams -- bit for bit what icz_ciderd_cook_host writes for the same tokens.  The entries are
 * PACKED: candidate c owns ent_ptr_out[c] .. ent_ptr_out[c+1] with ent_ptr_out[0] = 0 (a counting pass and a prefix sum over the
 * candidates run in front of the writing pass); the three entry arrays must hold the worst case of 240 entries per candidate
 * (ent_key_out [n_cand*240, 4], ent_order_out / ent_w_out [n_cand*240]), ent_ptr_out [n_cand+1], norm_out [n_cand, 4], len_out [n_cand]. */
int icz_ciderd_cook_device(icz_ciderd_t* h, const int32_t* tok, const int32_t* ptr, int32_t n_cand, int32_t* ent_key_out,
                           int32_t* ent_order_out, double* ent_w_out, int32_t* ent_ptr_out, double* norm_out, int32_t* len_out, void* stream);
/* CIDEr-D of every candidate with its siblings as references, K = 2..8: the n_img K candidates are cooked once on the device, then
 * the matching loop of the reward kernel runs hypothesis a against the cooked candidates of its image.
 *   pair_out [n_img, K, K] float64: [i][a][b] = CIDEr-D of a with b as its only reference (sim() of ciderD_scorer.py:155-183, mean over
 *     n, * 10), diagonal included; not symmetric (the clipping min(vh, vr) * vr is not).
 *   consensus_out [n_img, K] float64 or NULL: CIDEr-D of a with the OTHER K - 1 candidates as its reference set in the scorer's order
 *     (per-order sums over b ascending, b != a; mean over n; / (K - 1); * 10).
 *   best_out [n_img] int32 or NULL: the a with the largest consensus, ties to the lowest a.
 * workspace: icz_ciderd_pairwise_workspace_bytes(n_img, K) bytes of device memory, 8-byte aligned (0 = bad arguments). */
size_t icz_ciderd_pairwise_workspace_bytes(int32_t n_img, int32_t K);
int icz_ciderd_pairwise(icz_ciderd_t* h, const int32_t* tok, const int32_t* ptr, int32_t n_img, int32_t K, double* pair_out,
                        double* consensus_out, int32_t* best_out, void* workspace, size_t workspace_bytes, void* stream);
/* The CSR candidates against the reference STORE (arrays and img_slot [n_img] as icz_ciderd_reward_loo), K = 1..8:
 * scores_out [n_img K] float64 = CIDEr-D of candidate img * K + k against the references of image img -- the reward kernel with
 * a CSR hypothesis source instead of the int64 rows and their length rules. */
int icz_ciderd_scores_csr(icz_ciderd_t* h, const int32_t* tok, const int32_t* ptr, int32_t n_img, int32_t K, const int32_t* img_slot,
                          const int32_t* img_ref_ptr, const int32_t* ref_ent_ptr, const int32_t* ent_key, const int32_t* ent_order,
                          const double* ent_w, const double* ref_norm, const int32_t* ref_len, double* scores_out, void* stream);
/* counts_out [n_img, 4, 2] int32: for n = 1..4 {distinct n-grams over the image's K candidates, n-gram positions over them}
 * (n-grams do not cross candidates), K = 1..8.  One workgroup per image, the set in LDS. */
int icz_ngram_diversity(const int32_t* tok, const int32_t* ptr, int32_t n_img, int32_t K, int32_t* counts_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * BLEU and ROUGE-L of the evaluation report (COCO_Eval_Utils.py:15-35 -> coco_caption/pycocoevalcap/eval.py:24-69): the
 * integer statistics on the device, the float64 scores on the host in the reference's order (coco_eval.py Bleu / Rouge).
 * All arrays are int32 DEVICE arrays of corpus-local token ids >= 0 in CSR form: hypothesis i = hyp_tok[hyp_ptr[i] ..
 * hyp_ptr[i+1]) with at most 60 tokens (the caller checks), reference r = ref_tok[ref_ptr[r] .. ref_ptr[r+1]) of any length,
 * image i owns references img_ref_ptr[i] .. img_ref_ptr[i+1] (at least one).  stream: hipStream_t or NULL.
 * ---------------------------------------------------------------------------------------------------------- */
/* Replaces precook / cook_refs / cook_test with option "closest" (bleu/bleu_scorer.py:26-86, :190-191):
 * stats_out [n_img, 6] = testlen, closest reference length (ties: the shorter), correct[1..4] (clipped n-gram matches). */
int icz_bleu_stats(const int32_t* hyp_tok, const int32_t* hyp_ptr, const int32_t* ref_tok, const int32_t* ref_ptr,
                   const int32_t* img_ref_ptr, int32_t n_img, int32_t* stats_out, void* stream);
/* Replaces my_lcs (rouge/rouge.py:15-36) as called by Rouge.calc_score (:38-71): lcs_out [n_ref] = length of the longest
 * common subsequence of reference r and its image's hypothesis. */
int icz_rouge_lcs(const int32_t* hyp_tok, const int32_t* hyp_ptr, const int32_t* ref_tok, const int32_t* ref_ptr,
                  const int32_t* img_ref_ptr, int32_t n_img, int32_t* lcs_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Building blocks exported for tests and benchmarks
 * ---------------------------------------------------------------------------------------------------------- */
/* C[M,N] = X[M,K] W[N,K]^T (+ bias[N]) on the fp32 MFMA; layout 0 = NT (y = x W^T), 1 = NN (C = X[M,K] W[K,N]),
 * 2 = TN (C = X[K,M]^T W[K,N]).  nsplit = 0 lets the library choose (then icz_gemm_workspace_floats(M,N) floats
 * of workspace suffice); an explicit nsplit needs nsplit*M*N floats. */
int icz_gemm_f32(int32_t layout, const float* X, int32_t ldx, const float* W, int32_t ldw, const float* bias,
                 float* C, int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t nsplit, float* workspace,
                 size_t workspace_floats, void* stream);
size_t icz_gemm_workspace_floats(int32_t M, int32_t N);
/* The same product over nseg = 1..4 K segments, as the decoder steps issue it: C = sum_s A_s B_s (+ bias), segment s with its own
 * operands, leading dimensions and K[s] (layouts as above; every A_s / B_s may be a column slice of a wider buffer).  Fills the
 * library's GEMM arguments and launches, nothing more.  nsplit = 0: the split of a decoder step (what icz_gemm_route_for assumes),
 * cut to the workspace; an explicit nsplit is taken as given (a split that leaves an empty split is an error).  accumulate != 0:
 * C += product, one split.  live: optional device int32, 0 = the launch returns without writing (a finished rollout's step).
 * More than one split: slabs [nsplit][M][N] go to `workspace`; with C they are then summed in slab order, with the bias (needs
 * ldc == N, M * N % 4 == 0, N % 4 == 0 with a bias); C == NULL leaves the raw slabs (one split: the finished product, dense) in
 * `workspace` for the caller.  *nsplit_used (optional) = the split that ran.  ICZ_ERR, nothing launched, for a null table, nseg
 * out of range and everything the library's own argument check refuses. */
int icz_gemm_f32_seg(int32_t layout, int32_t nseg, const float* const* A, const int32_t* lda, const float* const* B, const int32_t* ldb,
                     const int32_t* K, const float* bias, float* C, int32_t ldc, int32_t M, int32_t N, int32_t nsplit, int32_t accumulate,
                     const int32_t* live, float* workspace, size_t workspace_floats, int32_t* nsplit_used, void* stream);
/* Two independent NT products of that kind as ONE launch of the resident-activation kernel (the two recurrent dgrad products of a
 * BPTT step): 33..64 rows each, whole 64-deep stages, N >= 512, both in the same stage form (512-deep or four-stage k ranges) and
 * more than one k range each, else ICZ_ERR and nothing is launched.  Slabs [nsplit][M][N] go to slabs_a / slabs_b (no bias);
 * *nsplit_a / *nsplit_b = their counts.  live as above. */
int icz_gemm_resident_pair(int32_t nseg_a, const float* const* A_a, const int32_t* lda_a, const float* const* B_a, const int32_t* ldb_a, const int32_t* K_a,
                           int32_t M_a, int32_t N_a, float* slabs_a, size_t slabs_a_floats, int32_t* nsplit_a,
                           int32_t nseg_b, const float* const* A_b, const int32_t* lda_b, const float* const* B_b, const int32_t* ldb_b, const int32_t* K_b,
                           int32_t M_b, int32_t N_b, float* slabs_b, size_t slabs_b_floats, int32_t* nsplit_b, const int32_t* live, void* stream);
/* Which kernel the many-row split-precision products (>= 128 rows: weight gradients, dgrad over all steps, beam / refiner / XE forward
 * GEMMs) run on: -1 = chosen per shape (default; the environment's ICZ_GEMM_BIG sets the same switch), 0 = the 128 x 128 two-barrier
 * kernel everywhere, 1..5 = one large-tile configuration of gemm_big_x3.hip everywhere, -2 = back to the environment's value.
 * Process-wide; meant for tests and A/B measurements, not for use while other threads launch. */
int icz_gemm_set_big_cfg(int32_t cfg);
/* The tile configuration a many-row product of that shape is given (host logic only, no GPU needed): 0 = the 128 x 128 two-barrier
 * kernel, 1 = 256 x 256 / eight waves, 4 = 128 x 128 three workgroups per CU; -1 = bad arguments.  Only meaningful for shapes that
 * reach those kernels at all (>= 128 rows and columns, K in whole 128-deep chunks; TN: >= 256 tiles of 128 x 128). */
int icz_gemm_big_cfg_for(int32_t layout, int32_t M, int32_t N, int32_t K, int32_t nsplit);
/* Weight gradients that share d y as ONE launch: out_j[M, cols_j] (row stride ldo_j) = dY[K, M]^T X_j[K, cols_j], j < ngroups <= 4,
 * cols_j % 256 == 0, M * sum(cols_j) >= 256 tiles of 128 x 128 (else ICZ_ERR: issue them one by one through icz_gemm_f32).
 * rows_live: optional device count of leading rows of K that matter (rounded up to 32).  What Butd::bptt does for the
 * LSTM weight gradients (BUTD_Model.py:137-145 under loss.backward(), Engine.py:186,270). */
int icz_gemm_tn_grouped(const float* dY, int32_t ldy, int32_t M, int32_t K, int32_t ngroups, const float* const* X, const int32_t* ldx,
                        const int32_t* cols, float* const* out, const int32_t* ldo, const int32_t* rows_live, void* stream);
/* The split-K factor Butd::wgrad gives a weight gradient dY[K, M]^T X[K, N] with fewer than 256 tiles of 128 x 128 (host logic only, no
 * GPU needed): > 1 = that many slabs on the large-tile split-precision kernel (gemm_tn_split), 1 = shape not taken (it goes through
 * icz_gemm_f32's TN route), -1 = bad arguments.  Taken: M, N >= 128 and multiples of 4, K >= 512 and a multiple of 16. */
int icz_gemm_tn_split_pick(int32_t M, int32_t N, int32_t K);
/* out[M, N] (dense: ldo == N) = dY[K, M]^T X[K, N] the way Butd::wgrad computes such a product: icz_gemm_tn_split_pick(M, N, K) slabs of
 * M x N floats into `workspace` (splits on 128-deep chunk boundaries of K), then their sum in slab order into `out`.  ICZ_ERR when the
 * shape is not taken or the workspace is too small.  rows_live: optional device count of the leading rows of K that matter (rounded
 * up to 32); the rows behind it are not read. */
int icz_gemm_tn_split(const float* dY, int32_t ldy, int32_t M, const float* X, int32_t ldx, int32_t N, int32_t K, float* out, int32_t ldo,
                      float* workspace, size_t workspace_floats, const int32_t* rows_live, void* stream);
/* The kernel icz_gemm_f32 / the decoders' GEMM calls launch for a product of K[0] + ... + K[nseg - 1] (host logic only, no GPU needed):
 * 0 / 1 / 2 = fp32-MFMA NT kernel with 16 / 32 / 64-row tiles, 3 = resident-activation kernel, four 64-deep stages per workgroup,
 * 4 = its 512-deep form, 5 = its 128-row form, 6 = split-precision 128 x 128 two-barrier kernel, 7 = a large-tile configuration
 * (icz_gemm_big_cfg_for says which), 8 = fp32-MFMA NN kernel, 9 = fp32-MFMA TN kernel on 64 x 64 tiles, 10 = fp32 TN kernel on
 * 128 x 128 tiles (ICZ_GEMM_TN_X3=0); -1 = bad arguments or a split the library refuses.  nsplit 0: the split of a decoder step. */
int icz_gemm_route_for(int32_t layout, int32_t M, int32_t N, int32_t nseg, const int32_t* K, int32_t nsplit);
/* The split icz_gemm_f32_seg takes for nsplit = 0 with a workspace of that many floats (host logic only, no GPU needed): the split of a
 * decoder step, cut to the largest one whose slabs fit; -1 = bad arguments. */
int icz_gemm_split_for(int32_t layout, int32_t M, int32_t N, int32_t nseg, const int32_t* K, size_t workspace_floats);
/* Whether icz_gemm_tn_grouped takes column groups of these widths over K rows (host logic only, no GPU needed): 1 / 0, -1 = bad arguments. */
int icz_gemm_tn_grouped_fits(int32_t M, int32_t K, int32_t ngroups, const int32_t* cols);
/* Test entry for the fork / join rule of the decoders' side streams (SideStream::Branch, decoder_core.h): as one captured graph of its
 * own cache (a call that fails nowhere is replayed by the next such call with the same inline_branch and out2), a branch is forked off `stream`, one tiny kernel writes
 * out2[0] = 1 on `stream` and one writes out2[1] = 2 on the branch's stream (inline_branch != 0: the branch runs in line on `stream`),
 * and the branch is joined.  fail_at = 0..3: the call returns ICZ_ERR_INVALID with "side-branch test: stage <fail_at>" behind the fork
 * point (0), behind the branch's start (1), behind its launch (2), behind its finish (3) -- the branch is still joined, so the error
 * is reported as itself and `stream` is left usable; fail_at = -1 fails nowhere.  out2: two device floats. */
int icz_test_side_branch(int32_t fail_at, int32_t inline_branch, float* out2, void* stream);
/* Test entries for the kernels that finish a backward pass and the weight refresh, each on its own (tests/test_gpu_support_kernels.py):
 * the library's kernel through the library's launch code, arguments filled as the decoders fill them (tables: blocks job after
 * job).  Every entry checks on the host what its kernel needs of the shape and the pointers -- columns in whole groups of 4,
 * 16-byte alignment wherever the kernel moves four floats at a time, table sizes -- and returns ICZ_ERR_INVALID without launching
 * otherwise.  All data pointers are DEVICE pointers; the tables (v[], rows[], ...) are HOST arrays of `count` entries.
 *
 * Embedding gradient: dE[v, :] = sum over i < n_tok with tok[i] == v, in list order, of (sum_{z < ns} demb[z * slab_stride + i * E + :])
 * * (relu ? (emb[i * E + :] > 0 ? scale : 0) : scale); every row of dE [V, E] is written.  rows_live: optional device int32, only the
 * first min(n_tok, *rows_live) list entries count (and are read).  route 0 = the form the decoders' launch picks for n_tok, 1 = the
 * form that holds the whole list in LDS (lists of up to ~4500 tokens), 2 = the windowed form (E <= 1024); a forced form that cannot
 * take the shape is an error.  Both forms add the same numbers in the same order: the same bits. */
int icz_test_embed_grad(const int64_t* tok, int32_t n_tok, const float* demb, int32_t ns, int64_t slab_stride, const float* emb, float scale,
                        int32_t E, float* dE, int32_t V, int32_t relu, const int32_t* rows_live, int32_t route, void* stream);
/* The form route 0 takes (host logic only, no GPU needed): 1 or 2, *lds_bytes_out (optional) = dynamic LDS bytes of the launch (form 2:
 * 0); ICZ_ERR_INVALID for bad arguments and for a list that needs the windowed form at E > 1024. */
int icz_embed_grad_route_for(int32_t n_tok, int32_t E, size_t* lds_bytes_out);
/* w_j[r, :] = v_j[r, :] g_j[r] / ||v_j[r, :]||, norm_j[r] = ||v_j[r, :]|| for `count` matrices [rows[j], cols[j]] (dense).  multi != 0:
 * the table kernel, 1..4 jobs in one launch; multi == 0: the single-matrix kernel, count == 1. */
int icz_test_weight_norm(int32_t multi, int32_t count, const float* const* v, const float* const* g, float* const* w, float* const* norm,
                         const int32_t* rows, const int32_t* cols, void* stream);
/* Its backward: dg_j[r] = dw_j[r, :] . v_j[r, :] / norm_j[r], dv_j[r, :] = (g_j[r] / norm_j[r]) (dw_j[r, :] - (dg_j[r] / norm_j[r]) v_j[r, :]);
 * dw_j has row stride lddw[j] >= cols[j] (a multiple of 4), everything else is dense.  multi / count as above. */
int icz_test_weight_norm_bwd(int32_t multi, int32_t count, const float* const* dw, const int32_t* lddw, const float* const* v, const float* const* g,
                             const float* const* norm, float* const* dv, float* const* dg, const int32_t* rows, const int32_t* cols, void* stream);
/* dst_j[c, r] = src_j[r * ld[j] + c], r < rows[j], c < cols[j] (both multiples of 64; dst row stride rows[j]), 1..4 jobs in one launch. */
int icz_test_transpose(int32_t count, const float* const* src, const int32_t* ld, const int32_t* rows, const int32_t* cols, float* const* dst,
                       void* stream);
/* out_j[n] = sum_{k < K[j]} X_j[k * ldx[j] + n], n < N[j]; K[j] = 0 writes zeros.  multi != 0: 1..8 jobs in one launch, out2 (optional
 * table, entries may be NULL) receives a copy of out_j; multi == 0: the single sum behind every bias gradient, count == 1, no out2. */
int icz_test_colsum(int32_t multi, int32_t count, const float* const* X, const int32_t* K, const int32_t* N, const int32_t* ldx, float* const* out,
                    float* const* out2, void* stream);
/* out[i] = sum_{t < T} X[t * BN + i], i < BN, added in t order (BN a multiple of 4). */
int icz_test_timesum(const float* X, int32_t T, int64_t BN, float* out, void* stream);
/* out[i, n] = sum_{k < G} X[(i * G + k) * N + n], i < n_img, n < N, added in k order (N a multiple of 4). */
int icz_test_rowgroup_sum(const float* X, int32_t n_img, int32_t G, int64_t N, float* out, void* stream);
/* One "X2 = d dec . w_dec, then the TD-LSTM backward" step of the BUTD reverse-time loop on given buffers (tests/test_gpu_bptt_fused_step.py):
 * arguments filled as the loop fills them, and either lstm_bwd_dh1_fused_kernel (route 1; ICZ_ERR_INVALID unless rows <= 64, H % 16 == 0,
 * A % 64 == 0) or the NN product into split-K slabs followed by lstm_bwd_point_kernel (route 0), or whichever the loop takes with the
 * option "fused_dh1" on (route -1), reported in *route_out (optional).  *nsplit_out (optional): the K ranges the library cuts the
 * product into for the shape, which both routes follow.  With dh1 = (carry ? sum of the ns_carry slabs carry[z][rows_carry][H] at rows <
 * rows_carry : 0) + sum of the ns_x1 slabs x1[z][rows][ld_x1] (columns 0..H of each row: pass the pointer at the column offset) + sum
 * over the ranges of d dec[rows, A] . w_dec[A, H]:  dc = (dc_in [rows_carry, H], optional, rows < rows_carry) + dh1 o (1 - tanh^2 c_cur),
 * dgates [rows, 4H] = d(pre-activation i, f, g, o) from the activated gates [rows, 4H], c_prev [rows, H] (optional: zeros) and c_cur,
 * dc_prev [rows, H] = dc f.  live / carry_live: optional device int32 flags; *live == 0 writes zero dgates rows and nothing else,
 * *carry_live == 0 drops carry and dc_in.  x2_slabs / x2_floats: the two-launch route's slab buffer (route 1 does not touch it).
 * rows 1..64, H and A multiples of 4, ld_x1 >= H, ddec / w_dec / x2_slabs 16-byte aligned. */
int icz_test_bptt_dh1_step(int32_t route, int32_t rows, int32_t H, int32_t A, const float* ddec, const float* w_dec, const float* carry,
                           int32_t ns_carry, int32_t rows_carry, const float* x1, int32_t ns_x1, int32_t ld_x1, const float* dc_in,
                           const float* gates, const float* c_prev, const float* c_cur, float* dgates, float* dc_prev, const int32_t* live,
                           const int32_t* carry_live, float* x2_slabs, size_t x2_floats, int32_t* nsplit_out, int32_t* route_out, void* stream);
/* Test entries for the kernels of one beam-search step and of the final selection, each on given logits and a given search state
 * (tests/test_gpu_beam_step.py): the library's kernels through the launch code and the grids of every icz_*_beam_search entry.  All data
 * pointers are DEVICE pointers.  Every entry checks its arguments on the host and returns ICZ_ERR_INVALID without launching on: k outside
 * 1..8, groups not dividing k, step (steps_done) outside 1..256 or L <= step, ngram not in {0, 2, 3, 4}, compact other than 0 or (1 at
 * step 1), V < 1 or ldl < V, a forced route that cannot take the shape, null pointers.  (n_act holds device data: at most k per image, at
 * most k / groups per group.)
 *
 * The kernel that picks a row's candidates: route 1 = beam_rowtopk_reg_kernel<3> (V <= 3072), 2 = beam_rowtopk_reg_kernel<10>
 * (V <= 10240), both with 16-byte loads: ldl % 4 == 0, ldl >= V rounded up to 4, a 16-byte aligned base; 3 = the sweep kernel
 * beam_rowtopk_kernel (any V, ldl and base; compiled with the ban test from step ngram on).  Route 0 = what a search takes, the first
 * of 1, 2, 3 that fits -- icz_beam_rowtopk_route_for says which (host logic only, no GPU needed; base_aligned: whether the logits start
 * on 16 bytes); ICZ_ERR_INVALID for V < 1 or ldl < V. */
int icz_beam_rowtopk_route_for(int32_t V, int32_t ldl, int32_t base_aligned);
/* Row top-k of step `step`: for every scored row (row = img * k + r; plain: r < n_act[img], at step 1 row 0 only; grouped: n_act
 * [n_img, groups], see icz_beam_diversity) its best n candidates by (run[row] + log_softmax(logits[row, :V]) descending, token
 * ascending), n = n_act[img] (grouped: min(k, n_act[img, 0] + ... + n_act[img, g]); step 1: k), into cand_val / cand_idx [n_img * k, 8];
 * a slot without an admissible token holds index 0x7fffffff; every other slot is left untouched.  logits [rows, ldl] (compact = 1, step 1
 * only: one row per image); run is not read at step 1; ngram > 0: tokens banned by the prefixes seqs_in [n_img * k, L] score -inf. */
int icz_test_beam_rowtopk(int32_t route, const float* logits, int32_t n_img, int32_t k, int32_t V, int32_t ldl, int32_t step, const int32_t* n_act,
                          const float* run, int32_t compact, const int32_t* seqs_in, int32_t L, int32_t ngram, int32_t groups, float* cand_val,
                          int32_t* cand_idx, void* stream);
/* The state one step of a search reads and writes (BeamBuf, csrc/decoder_core.h): n_act [n_img] (grouped [n_img, groups]), run [n_img * k],
 * seqs_in / seqs_out [n_img * k, L] (distinct), src_row [n_img * k], it_next [n_img * k], best_* / has_complete per image (best_seq
 * [n_img, L]), n_live one word the step adds its live images to, the n-best list hyp_seq [n_img * k, L], hyp_score / hyp_len [n_img * k],
 * hyp_cnt [n_img] (all four null: no list; a grouped step needs it), and the candidate scratch cand_val / cand_idx [n_img * k, 8]. */
typedef struct {
    const float* logits;
    int32_t* n_act;
    float* run;
    const int32_t* seqs_in;
    int32_t* seqs_out;
    int32_t* src_row;
    int64_t* it_next;
    float* best_score;
    int32_t* best_len;
    int32_t* best_seq;
    int32_t* has_complete;
    int32_t* n_live;
    int32_t* hyp_seq;
    float* hyp_score;
    int32_t* hyp_len;
    int32_t* hyp_cnt;
    float* cand_val;
    int32_t* cand_idx;
} icz_beam_step_state;
/* One whole step: the row top-k (route as above), then beam_merge_kernel (groups == 1, lambda == 0) or beam_merge_groups_kernel (groups
 * > 1, lambda = the diversity penalty, >= 0 and finite). */
int icz_test_beam_step(int32_t route, const icz_beam_step_state* s, int32_t n_img, int32_t k, int32_t V, int32_t ldl, int32_t step, int32_t L,
                       int32_t compact, int32_t ngram, int32_t groups, float lambda, void* stream);
/* The final selection on a given state: form 0 = beam_finalize_kernel (n_best 1; scores may be null), 1 = beam_finalize_nbest_kernel<false>,
 * 2 = beam_finalize_nbest_kernel<true> (n_act [n_img, groups]); forms 1 and 2 check n_best, lp_kind and lp_alpha as icz_beam_opts.  seqs
 * [n_img * k, L] = the live beams after steps_done steps; out [n_img, n_best, L] float32, lens / scores [n_img, n_best].  Pointers a form
 * does not read may be null. */
int icz_test_beam_finalize(int32_t form, int32_t n_img, int32_t k, int32_t L, int32_t steps_done, int32_t n_best, int32_t lp_kind, float lp_alpha,
                           int32_t groups, const int32_t* n_act, const float* run, const int32_t* seqs, const int32_t* has_complete,
                           const float* best_score, const int32_t* best_len, const int32_t* best_seq, const int32_t* hyp_cnt, const float* hyp_score,
                           const int32_t* hyp_len, const int32_t* hyp_seq, float* out, int32_t* lens, float* scores, void* stream);
/* Test entries of the constrained step's kernels (tests/test_gpu_beam_constrained_step.py), on given logits and a given state as the
 * entries above: rows state-major (row img * K + s * beam + j, K = 2^C * beam <= 32), n_act / cap [n_img, 2^C] (cap = a state's
 * remaining capacity, n_act <= cap <= beam its live beams), words [n_img, C, A] device word ids (-1 empty; may be null for C = 0).
 * Host checks as above with beam in 1..8, C in 0..3, A in 1..4 (the device data is the caller's: word ids below V).
 * Row top-k, constrained instances of the three routes: for every live row (j < n_act[img, s]) its best cap[img, s] candidates over the
 * tokens that are no constraint word of the image into cand_val / cand_idx [n_img * K, 8] (an empty slot: index 0x7fffffff), and the
 * score rs + ((x - mx) - ls) of constraint word c, alternative a into force_val [n_img * K, 12] slot c * 4 + a (-inf: n-gram-banned
 * or an empty slot); rows that are not live are left untouched. */
int icz_test_beam_rowtopk_constrained(int32_t route, const float* logits, int32_t n_img, int32_t beam, int32_t C, int32_t A, const int32_t* words,
                                      int32_t V, int32_t ldl, int32_t step, const int32_t* n_act, const int32_t* cap, const float* run,
                                      int32_t compact, const int32_t* seqs_in, int32_t L, int32_t ngram, float* cand_val, int32_t* cand_idx,
                                      float* force_val, void* stream);
/* The state one constrained step reads and writes: icz_beam_step_state without the single best hypothesis, plus words, cap, hyp_state
 * [n_img * K] (the state of every listed retirement; the list is always kept, hyp_cnt [n_img] <= K) and force_val [n_img * K, 12]. */
typedef struct {
    const float* logits;
    const int32_t* words;
    int32_t* n_act;
    int32_t* cap;
    float* run;
    const int32_t* seqs_in;
    int32_t* seqs_out;
    int32_t* src_row;
    int64_t* it_next;
    int32_t* n_live;
    int32_t* hyp_seq;
    float* hyp_score;
    int32_t* hyp_len;
    int32_t* hyp_state;
    int32_t* hyp_cnt;
    float* cand_val;
    int32_t* cand_idx;
    float* force_val;
} icz_beam_constrained_state;
/* One whole constrained step: the constrained row top-k (route as above), then beam_merge_states_kernel (icz_beam_constraints: "A step"). */
int icz_test_beam_constrained_step(int32_t route, const icz_beam_constrained_state* s, int32_t n_img, int32_t beam, int32_t C, int32_t A, int32_t V,
                                   int32_t ldl, int32_t step, int32_t L, int32_t compact, int32_t ngram, void* stream);
/* The final ranking of a constrained search on a given state (beam_finalize_states_kernel; icz_beam_constraints: "Result"); n_best, lp_kind
 * and lp_alpha checked as icz_beam_opts.  out [n_img, n_best, L] float32, lens / scores / sat [n_img, n_best]. */
int icz_test_beam_finalize_states(int32_t n_img, int32_t beam, int32_t C, int32_t L, int32_t steps_done, int32_t n_best, int32_t lp_kind,
                                  float lp_alpha, const int32_t* n_act, const float* run, const int32_t* seqs, const int32_t* hyp_cnt,
                                  const float* hyp_score, const int32_t* hyp_len, const int32_t* hyp_state, const int32_t* hyp_seq, float* out,
                                  int32_t* lens, float* scores, int32_t* sat, void* stream);
/* Test entries for the kernels that turn a row of logits into a token, a log-probability or a gradient, each on given logits
 * (tests/test_gpu_token_choice.py): the library's kernels through the launch helpers of the decoders, arguments filled as the decoders
 * fill them.  All data pointers are DEVICE pointers (rows_t of icz_test_xe_loss is a HOST array).  Every entry checks its arguments on
 * the host and returns ICZ_ERR_INVALID without launching on: V < 1 or ldl < V (V < 2 for the XE loss), rows < 1, ns outside 1..16 or
 * slabs that overlap, E < 4 or E % 4, a table / emb that is not 16-byte aligned, t outside 0..T-1, T above 128 for the XE loss, a row that
 * does not fit in LDS (icz_sample_select_max_vocab), null pointers.
 *
 * The logits: ns == 1 finished rows [rows, ldl]; ns > 1 the ns split-K slabs of the vocabulary projection, slab z at logits + z *
 * slab_stride, and the finished logit is slab0 + slab1 + ... + bias[v] in fp32, in that order.  Any ldl >= V, slab_stride and alignment
 * of logits / bias / logits_store is taken: 16-byte loads need ldl % 4 == 0, slab_stride % 4 == 0 and 16-byte aligned bases, every other
 * layout goes through the scalar loads and gives the same bits.
 *
 * Greedy choice: ids = argmax_v, the lowest index among equal maxima, 0 for a row without any logit above -inf (NaN rows too);
 * it_next[row] = id, ids_out[row, t] = id (optional, [rows, T]), emb[row, :] = relu ? max(table[id, :], 0) : table[id, :].
 * route 1 = argmax_part_kernel + embed_argmax_kernel (ns == 1, bias == NULL, no counters; part_val / part_idx [rows, 8] scratch),
 * route 2 = greedy_select_kernel (any ns, bias optional; unfinished [rows] / n_unfinished [T] optional, both or none: the SCST baseline's
 * <end> bookkeeping -- token 2 clears unfinished[row], n_unfinished[t] counts the rows still unfinished, and at t > 0 with
 * n_unfinished[t - 1] == 0 the kernel writes ids_out[row, t] = 0 and nothing else), route 0 = what the decoders' launch_greedy_select
 * takes: route 2 for ns > 1, else route 1. */
int icz_test_greedy_select(int32_t route, const float* logits, int32_t rows, int32_t V, int32_t ldl, int32_t ns, int64_t slab_stride,
                           const float* bias, const float* table, int32_t E, int32_t relu, int32_t t, int32_t T, int64_t* ids_out,
                           int64_t* it_next, float* emb, uint8_t* unfinished, int32_t* n_unfinished, float* part_val, int32_t* part_idx,
                           void* stream);
/* The longest row sample_select_kernel and ss_select_kernel take: the row lies in dynamic LDS, whose limit both launch helpers raise once;
 * a longer row is refused on the host by the rollouts of all three decoders, by scheduled sampling and by the two entries below (host
 * logic only, no GPU needed). */
int icz_sample_select_max_vocab(void);
/* The fields of the multinomial step (sample_select_kernel) that a caller owns.  Per sampled row r (rows - row0 of them): uniforms [.] or
 * NULL (Philox: seed, a device uint64, stream RNG_UNIFORM, step t), unfinished [.] in/out, seq_out / logp_out [., T], n_unfinished [T].
 * Per launched row: it_next, draw_out, lse_out [rows], emb_next [rows, E] (optional: emb_table [V, E]; emb_mode 0 no dropout, 1 emb_mask
 * = keep flags [rows - row0, E] of step t + 1, 2 Philox RNG_EMB at step t + 1; kept elements are doubled), logits_store [rows, ldl]
 * (ns > 1).  live_rows: optional int32, receives (t + 1) * rows.  row0 > 0: the merged kernel, rows [0, row0) are greedy rows (ids_out
 * [row0, T], g_unfinished [row0], n_any [T]). */
typedef struct {
    const float* logits; int32_t V, ldl, ns; int64_t slab_stride; const float* bias; float* logits_store;
    const float* uniforms; const uint64_t* seed; int32_t t, T;
    uint8_t* unfinished; int32_t* n_unfinished; int64_t* seq_out; float* logp_out; int64_t* it_next; int32_t* draw_out; float* lse_out;
    const float* emb_table; float* emb_next; int32_t E, emb_mode; const uint8_t* emb_mask;
    int32_t* live_rows;
    int32_t row0; int64_t* ids_out; uint8_t* g_unfinished; int32_t* n_any;
} icz_sample_select_args;
/* One multinomial step: logp = log_softmax(logits), draw = the smallest v with cumsum(exp(logp))[v] > u * sum (float64 sums, clamped to
 * V - 1), logp_out = logp[draw], lse_out = log-sum-exp, unfinished &= (draw != 2), seq_out = it_next = draw * unfinished; at t > 0 with
 * the gate counter of step t - 1 at zero the zeros of a finished rollout are written instead. */
int icz_test_sample_select(const icz_sample_select_args* a, int32_t rows, void* stream);
/* Scheduled sampling (ss_select_kernel): for the `rows` active rows of XE step t, tok[row] = a draw from softmax(logits_prev[row, :V]) where
 * gate[t * B + row] < ss_prob, else left as it is.  gate / draw: explicit [T, B] arrays (row t is read), or NULL: Philox streams RNG_SS_GATE /
 * RNG_SS_DRAW of *seed at step t. */
int icz_test_ss_select(const float* logits_prev, int32_t rows, int32_t B, int32_t V, int32_t ldl, int32_t t, float ss_prob, const float* gate,
                       const float* draw, const uint64_t* seed, int64_t* tok, void* stream);
/* LabelSmoothingLoss and its gradient over all steps (xe_loss_dlogits_kernel + sum_scale_kernel): logits [T B, ldl] in (row t * B + b), the
 * gradient (softmax - true) / N out, in place; rows b >= rows_t[t] and the pad columns [V, ldl) become zero.  captions [B, L], target =
 * captions[b, t + 1]; N = *n_dev if n_dev is given and positive, else n_tokens.  loss_rows [T B] per-row losses (zeroed first),
 * loss_out (optional) = their sum / N. */
int icz_test_xe_loss(float* logits, int32_t V, int32_t ldl, const int64_t* captions, int32_t L, int32_t B, int32_t T, const int32_t* rows_t,
                     float smoothing, float n_tokens, const float* n_dev, float* loss_rows, float* loss_out, void* stream);
/* The same loss over image-major rows (xe_group_loss_dlogits_kernel + sum_scale_kernel; what icz_butd_xe_backward runs behind
 * icz_butd_xe_forward_n): lengths [rows] is a DEVICE array of per-row step counts, each 0..T (read back and checked), and (row, t) is
 * active while t < lengths[row], in any order of the rows.  An inactive (row, t) is written as zeros without being read and leaves 0 in
 * loss_rows; an active one gives the bits icz_test_xe_loss gives for it.  ldl % 4 == 0 and logits 16-byte aligned.  N = *n_dev if given
 * and positive, else n_tokens if positive, else (n_tokens == 0) the sum of the lengths. */
int icz_test_xe_group_loss(float* logits, int32_t V, int32_t ldl, const int64_t* captions, int32_t L, int32_t rows, int32_t T,
                           const int32_t* lengths, float smoothing, float n_tokens, const float* n_dev, float* loss_rows, float* loss_out,
                           void* stream);
/* RewardCriterion and its gradient (reinforce_loss_kernel + reinforce_dlogits_kernel): logp, seq, reward, coef [B, T]; mask[b, 0] = 1,
 * mask[b, t] = seq[b, t - 1] > 0; denominator = *mask_sum_global if given and positive, else sum(mask); loss_out / mask_sum_out optional.
 * logits [T Bs', ldl] (Bs' = Bs or B), draw / lse [T Bs']: dlogits[row, v] = coef[b, t] (1[v == draw] - exp(logits - lse)) in place, zero
 * where draw < 0 or coef == 0 and in the pad columns.  Bs > 0: Bs rows per step of which [row0, row0 + B) are the rollout's. */
int icz_test_reinforce(const float* logp, const int64_t* seq, const float* reward, int32_t B, int32_t T, const float* mask_sum_global, float* coef,
                       float* loss_out, float* mask_sum_out, float* logits, int32_t V, int32_t ldl, const int32_t* draw, const float* lse, int32_t Bs,
                       int32_t row0, void* stream);
/* Test entries for the kernels of the AoA family, each on given operands (tests/test_gpu_aoa_kernels.py): the library's kernels through
 * the launch helpers of the AoA handle (route, query chunk, LDS bytes and the dynamic-LDS opt-in above 48 KB are the handle's).  All data
 * pointers are DEVICE pointers.  Every entry checks on the host what its kernel needs -- 1..128 regions, heads of a multiple of 4 columns,
 * 16-byte alignment wherever the kernel loads 16 bytes, the LDS budget of 156 KB, the dropout and region arguments below -- and returns
 * ICZ_ERR_INVALID without launching otherwise.
 *
 * Dropout: mode 0 off, 1 keep flags (uint8, nonzero = keep; element i of the draw reads mask[i - idx0]), 2 Philox (*seed a device uint64;
 * stream, step as the AoA handle numbers them: word (i - idx0) & 3 of counter ((i - idx0) >> 2, step, stream) >= floor(p 2^32) keeps).
 * Kept values are multiplied by 1 / (1 - p).  Elements in front of idx0 pass unchanged: the evaluation-mode half of a paired refiner
 * pass.  A null icz_test_dropp is mode 0.
 *
 * Region counts: `counts` [n_img] device int32, each 1..R (read back and checked), or NULL = R regions everywhere.  With counts the
 * region rows are PACKED -- image i owns rows off[i] .. off[i] + counts[i] of qkv / o / Kd / Vd -- while the dropout index of a draw
 * keeps the padded strides (R); the entry builds off / rowmap as the handle does and waits for the stream before it returns. */
typedef struct {
    int32_t mode;
    const uint8_t* mask;
    const uint64_t* seed;
    uint32_t stream, step;
    float p;
    uint64_t idx0;
} icz_test_dropp;
/* layer_norm_kernel: y = gain (x - mean) / (std + 1e-6) + bias per row of n >= 2 columns, std unbiased (AoA_Model.py:14-25); stats
 * (optional) [rows, 2] = (mean, 1 / (std + 1e-6)); live (optional) device int32: 0 = the launch writes nothing.  geometry 0: four rows per
 * workgroup (the refiner's launch), 1: one wave per workgroup (the decoder's).  n <= 2048 with n % 4 == 0 keeps the row in registers
 * (16-byte aligned x, gain, bias, y); any other n re-reads the row with scalar loads. */
int icz_test_aoa_layer_norm(int32_t geometry, const float* x, const float* gain, const float* bias, float* y, int32_t rows, int32_t n, float* stats,
                            const int32_t* live, void* stream);
/* Which kernel the refiner self-attention of R regions takes, and how (host logic only, no GPU needed): returns 2 = mha_self_mfma_kernel
 * (mha_mfma != 0, R <= 64, heads of a multiple of 64 columns), 1 = mha_self_kernel; *qc_out = query rows per pass of mha_self_kernel (R when
 * everything fits the LDS budget, else the largest multiple of 4 that does), *lds_out = dynamic LDS bytes of the launch.  ICZ_ERR_INVALID
 * for a shape the handle refuses. */
int icz_aoa_self_attn_route_for(int32_t R, int32_t Hd, int32_t NH, int32_t mha_mfma, int32_t* qc_out, size_t* lds_out);
/* Refiner self-attention of n_img images: qkv [region rows, 3 Hd] = [Q | K | V], head h in columns [h d, (h + 1) d) of each block;
 * S = Q_h K_h^T / sqrt(d) over the image's valid keys, P = softmax_rows(S), Pd = drop(P) with draw index ((img NH + h) R + q) R + k,
 * o [region rows, Hd] = Pd V_h.  route 0: the handle's choice, 1: mha_self_kernel, 2: mha_self_mfma_kernel (refused unless R <= 64 and
 * d % 64 == 0).  qc 0: the handle's chunk; else a forced chunk of query rows for mha_self_kernel (R, or a multiple of 4 below R whose LDS
 * fits the budget).  route_out / qc_out (optional, host): what was launched. */
int icz_test_aoa_self_attn(int32_t route, const float* qkv, float* o, int32_t n_img, int32_t R, int32_t Hd, int32_t NH, const int32_t* counts,
                           int32_t qc, const icz_test_dropp* dropp, int32_t* route_out, int32_t* qc_out, void* stream);
/* aoa_dec_attn_kernel, one query per decoder row: row b attends image img_of_row[b] (NULL: image b; read back and checked against n_img);
 * s_r = Qp_h . Kd_h[r] / sqrt(d), P = softmax over the image's valid regions, Pd = drop(P) with draw index (b NH + h) R + r,
 * xatt [rows, Hd] = sum_r Pd_r Vd_h[r].  P_out / Pd_out (optional) [rows, NH, R]: exact zeros behind the image's count.  qns == 1: Qp
 * [rows, Hd] is the finished query projection; qns > 1 (up to 16): Qp holds qns slabs, q_stride >= rows Hd floats apart, and the kernel
 * leaves slab0 + slab1 + ... + q_bias (fp32, in that order) in Qp_store [rows, Hd].  live as above. */
int icz_test_aoa_dec_attn(const float* Qp, int32_t qns, int64_t q_stride, const float* q_bias, float* Qp_store, const float* Kd, const float* Vd,
                          const int32_t* img_of_row, float* xatt, float* P_out, float* Pd_out, int32_t rows, int32_t n_img, int32_t R, int32_t Hd,
                          int32_t NH, const int32_t* counts, const icz_test_dropp* dropp, const int32_t* live, void* stream);
/* The two LayerNorm backward kernels, one workgroup per row of n columns (a multiple of 4, at most 4096: refused otherwise); every tensor
 * 16-byte aligned.  With xh = x - mean, inv = 1 / (std + 1e-6), dy = dq gain:
 *   dx = dy inv - inv^2 sum(dy xh) xh / (std (n - 1)) - inv sum(dy) / n
 * form 0, aoa_ln_bwd_kernel (the decoder's h_norm): dq = the ns_a (1..16) slabs dq_a [ns_a][rows][n] + columns [n, 2 n) of the ns_b slabs
 *   dq_b [ns_b][rows][2 n], each summed in slab order; stats [rows, 2] = (mean, inv) of the forward pass; dq_tot [rows, n] = dq and dx out;
 *   live (optional): 0 = nothing is written.  res and prod must be NULL.
 * form 1, aoa_ln_bwd_dense_kernel (the refiner's norms; mean and std recomputed from x): dq = slabs dq_a (NULL with ns_a = 0: none) + the dense
 *   dq_b [rows][n] (may be NULL; ns_b must be 0); dq_tot (optional) = dq, prod [rows, n] = dq xh inv, dx = res (optional) + the formula.
 *   stats and live must be NULL. */
int icz_test_aoa_ln_bwd(int32_t form, const float* dq_a, int32_t ns_a, const float* dq_b, int32_t ns_b, int32_t rows, const float* x, const float* stats,
                        const float* gain, const float* res, float* dq_tot, float* prod, float* dx, int32_t n, const int32_t* live, void* stream);
/* mha_self_bwd_kernel, the backward of icz_test_aoa_self_attn on the same qkv, counts and dropout draw: P is recomputed, Pd = drop(P);
 *   dV = Pd^T dO;  dP = drop'(dO V^T);  dS = P (dP - sum_k P dP) / sqrt(d);  dQ = dS K;  dK = dS^T Q
 * dO [region rows, Hd], dqkv [region rows, 3 Hd] = [dQ | dK | dV].  Three head tiles [R][d + 1] and two [R][R + 1] floats of LDS: above
 * 156 KB the call is refused with the handle's message. */
int icz_test_aoa_self_attn_bwd(const float* qkv, const float* dO, float* dqkv, int32_t n_img, int32_t R, int32_t Hd, int32_t NH, const int32_t* counts,
                               const icz_test_dropp* dropp, void* stream);
/* aoa_dec_attn_bwd_kernel, the backward of icz_test_aoa_dec_attn for one step: dx = columns [0, Hd) of the ns (1..16) slabs dxq
 * [ns][rows][2 Hd] summed in slab order (dx_out [rows, Hd]); with P, Pd [rows, NH, R] of the forward pass and Qp [rows, Hd]:
 *   dPd_r = dx_h . Vd_h[r];  dP_r = Pd_r != 0 ? keep_scale dPd_r : 0;  dS_r = P_r (dP_r - sum_k P_k dP_k) / sqrt(d);  dQp_h = sum_r dS_r Kd_h[r]
 * dS_out [rows, NH, R] (already scaled by 1 / sqrt(d); zero behind the image's count), dQp [rows, Hd].  keep_scale: 1 without dropout,
 * else 1 / (1 - p).  counts, img_of_row (checked against n_img) and live as for icz_test_aoa_dec_attn. */
int icz_test_aoa_dec_attn_bwd(const float* dxq, int32_t ns, int32_t rows, const float* P, const float* Pd, const float* Qp, const float* Kd,
                              const float* Vd, float* dQp, float* dS_out, float* dx_out, int32_t n_img, int32_t R, int32_t Hd, int32_t NH,
                              const int32_t* counts, float keep_scale, const int32_t* live, const int32_t* img_of_row, void* stream);
/* aoa_dkv_kernel, the gradients of the hoisted decoder keys and values summed over the decoder rows and steps of every image:
 *   dKd[img, r, head cols] = sum_k sum_t dS[t, img G + k, head, r] Qp[t, img G + k, head cols],   dVd likewise from Pd and dx
 * dS_all, Pd_all [T, B, NH, R], Qp_all, dx_all [T, B, Hd], dKd, dVd [region rows, Hd] (packed with counts; rows behind a count are not
 * written).  B must be n_img * G -- the handle's decoder rows are the images' rows, row img * G + k, and nothing else -- any other B is
 * refused.  The (k, t) pairs are added k-major, t-minor in one fp32 accumulation that passes through dKd / dVd between chunks of tc
 * pairs, so every tc gives the same bits.  tc 0: the handle's rule (all G T pairs when they fit 48 KB of LDS, else as many as do); else a
 * forced chunk of 1..G T pairs within 48 KB.  tc_out (optional, host): the chunk that was launched. */
int icz_test_aoa_dkv(const float* dS_all, const float* Pd_all, const float* Qp_all, const float* dx_all, float* dKd, float* dVd, int32_t n_img,
                     int32_t B, int32_t T, int32_t tc, int32_t R, int32_t Hd, int32_t NH, const int32_t* counts, int32_t G, int32_t* tc_out,
                     void* stream);
/* Test entries for the kernels of an LSTM decoder step shared by BUTD, AoA and NIC (csrc/lstm_kernels.h), each on given operands
 * (tests/test_gpu_lstm_kernels.py): the library's kernel with the grid the decoders launch it with.  All data pointers are DEVICE
 * pointers (rows_t of icz_test_embed_steps is a HOST array).  Every entry checks its arguments on the host and returns ICZ_ERR_INVALID
 * without launching otherwise; device index arrays (token ids, pre_row) are read back and checked too, for which the entry waits for
 * the stream.
 *
 * Dropout (p = 0.5, kept values are doubled), the library's DropCfg: mode 0 off, 1 keep flags (uint8, nonzero = keep), 2 Philox (*seed a
 * device uint64; stream and step as the decoders number them, csrc/rng.h).  The forward kernels take row r >= row0 as row r - row0 of
 * the draw and leave rows < row0 undropped (the evaluation-mode rows of a merged chain); the backward and the all-steps embedding run over
 * the sampled rows alone and refuse row0 != 0.  The embedding kernels read four keep flags at once: their mask must be 4-byte aligned.  A
 * null icz_test_drop is mode 0. */
typedef struct {
    int32_t mode;
    const uint8_t* mask;
    const uint64_t* seed;
    uint32_t stream, step;
    int32_t row0;
} icz_test_drop;
/* embed_kernel: emb[row, :] = drop((relu ? max(table[it[row], :], 0) : table[it[row], :])), keep index (row - row0) E + e; table [V, E], it
 * [rows] (each 0..V-1), emb [rows, E].  E a multiple of 4 (at least 4), table and emb 16-byte aligned, rows >= 1.  live (optional) device
 * int32: 0 = the launch writes nothing. */
int icz_test_embed(const float* table, int32_t V, int32_t E, const int64_t* it, int32_t rows, float* emb, int32_t relu, const icz_test_drop* drop,
                   const int32_t* live, void* stream);
/* embed_steps_kernel, every step of a teacher-forced pass in one launch: emb[t B + b, :] = drop_t(max(table[tok[t B + b], :], 0)) for
 * b < rows_t[t], every other row left untouched; drop_t = Philox step t (the struct's step is not read) or the slice t of a mask [T, B, E],
 * keep index b E + e.  T in 1..128, rows_t [T] in 0..B and never increasing with t; all T B tokens are checked, the unused ones too. */
int icz_test_embed_steps(const float* table, int32_t V, int32_t E, const int64_t* tok, int32_t T, int32_t B, const int32_t* rows_t, float* emb,
                         const icz_test_drop* drop, void* stream);
/* The LSTMCell pointwise part behind the gate GEMMs (gate order i, f, g, o):
 *   p[row, :] = slab[0][row, :] + ... + slab[ns - 1][row, :] + pre[pre_row[row], :] + b_ih + b_hh   (fp32, in that order)
 *   c' = sig(p_f) c_prev + sig(p_i) tanh(p_g);  h' = sig(p_o) tanh(c')
 * slab [ns][rows][4H] dense with ns in 1..32; pre (optional) [n_pre, 4H] with pre_row (optional) [rows] int32, each 0..n_pre-1 (null:
 * row r reads pre row r, n_pre >= rows); gates_out (optional) [rows, 4H] the activated gates; hdrop_out (optional) [rows, H] = drop(h'),
 * keep index (row - row0) H + j; live as above. */
typedef struct {
    const float* slab; int32_t ns;
    const float* pre; int32_t n_pre; const int32_t* pre_row;
    const float* b_ih; const float* b_hh;
    const float* c_prev; float* h_out; float* c_out;
    float* gates_out; float* hdrop_out;
    int32_t rows, H;
    const int32_t* live;
} icz_test_lstm_point_args;
/* route 0 = what launch_lstm_point takes (the gate-per-wave kernel wherever H % 4 == 0), 1 = lstm_point_kernel (any H), 2 =
 * lstm_point_gw_kernel, refused unless H % 4 == 0 with 16-byte aligned slab, pre and biases (route 0 needs the same where it takes
 * that kernel).  Both kernels add the same numbers in the same order: the same bits.  *route_out (optional, host): the kernel taken. */
int icz_test_lstm_point(int32_t route, const icz_test_lstm_point_args* a, const icz_test_drop* drop, int32_t* route_out, void* stream);
/* lstm_bwd_point_kernel with every field of its arguments:
 *   dh = set a (if *carry_live != 0) + set b + set c + drop(dhdrop), each set summed in slab order first; set x = ns_x slabs of rows_x
 *        rows of lda_x floats (lda_x >= H; columns 0..H of each row: pass the pointer at the column offset), rows >= rows_x add nothing
 *   dc = (dc_in [.., H] at rows < dc_in_rows, if *carry_live != 0) + dh o (1 - tanh^2 c_cur)
 *   dgates [rows, 4H] = d(pre-activation i, f, g, o) from the activated gates [rows, 4H], c_prev [rows, H] (null: zeros) and c_cur;
 *   dc_prev [rows, H] = dc f.
 * Absent sets, dhdrop, dc_in: null pointers.  drop(dhdrop): doubled where kept, else 0, keep index row H + j.  live / carry_live:
 * optional device int32; *live == 0 writes zero dgates rows and nothing else.  Refused: lda_x < H, rows_x outside 1..rows, a set with
 * a pointer but ns_x outside 1..32, dc_in_rows outside 1..rows, null gates / c_cur / dgates / dc_prev. */
typedef struct {
    const float* dh_a; int32_t ns_a, lda_a, rows_a;
    const float* dh_b; int32_t ns_b, lda_b, rows_b;
    const float* dh_c; int32_t ns_c, lda_c, rows_c;
    const float* dhdrop;
    const float* dc_in; int32_t dc_in_rows;
    const float* gates; const float* c_prev; const float* c_cur;
    float* dgates; float* dc_prev;
    int32_t rows, H;
    const int32_t* live; const int32_t* carry_live;
} icz_test_lstm_bwd_args;
int icz_test_lstm_bwd_point(const icz_test_lstm_bwd_args* a, const icz_test_drop* drop, void* stream);
/* Test entries for the kernels of the BUTD soft attention (csrc/butd_kernels.h), each on given operands
 * (tests/test_gpu_butd_att_kernels.py): the library's kernel through the launch helper the decoders use (csrc/butd_impl.h) -- the same
 * template instance, grid rule and dynamic LDS size.  All data pointers are DEVICE pointers.  Every entry checks its arguments on the
 * host and returns ICZ_ERR_INVALID without launching otherwise; the device index arrays (counts [n_img], each 1..R; img_of_row [rows],
 * each 0..n_img-1) are read back and checked too, for which the entry waits for the stream.
 *
 * Common to all: n_img images of R regions (1..128; R stays the row stride of every tensor); the <true> instances of the kernels are
 * taken where counts are given or R > 64, as the handle takes them; widths (A, D) are positive multiples of 4 and the tensors read or
 * written 16 bytes at a time are 16-byte aligned; img_of_row null = row r attends over image r (rows <= n_img); live: optional device
 * int32, 0 = a dead step.  Dropout: icz_test_drop above (the keep index of element (row, r, a) is ((row - row0) R + r) A + a; keep
 * flags 4-byte aligned).
 *
 * mean_feats_kernel, or mean_feats_counts_kernel where counts are given: mean[b, :] = sum_{r < c_b} feats[b, r, :] / c_b in row order. */
int icz_test_att_mean(const float* feats, int32_t n_img, int32_t R, int32_t D, const int32_t* counts, float* mean, void* stream);
/* The score kernels, every field of AttScoreArgs:
 *   dec_ctx[row, :] = slab 0 + slab 1 + ... + slab nsplit-1 + b_dec (fp32, in that order; slabs rows A floats apart, nsplit in 1..32),
 *   also written to dec_ctx_out (optional) [rows, A];
 *   scores[row, r] = sum_a w_aff[a] drop(relu(enc_ctx[img, r, a] + dec_ctx[row, a])) + b_aff[0] for r < c_img, 0 behind it. */
typedef struct {
    const float* enc_ctx; int32_t n_img;     /* [n_img, R, A] */
    const int32_t* img_of_row;
    const float* dec_slab; int32_t nsplit;
    const float* b_dec; const float* w_aff; const float* b_aff;
    float* dec_ctx_out; float* scores;
    int32_t rows, R, A;
    const int32_t* live; const int32_t* counts;
} icz_test_att_scores_args;
/* route 0 = att_scores_kernel (G 0 or 1), 1 = att_scores_group_kernel (neither dropout nor live), 2 = att_scores_group_train_kernel.
 * The grouped routes take rows = G rows of each of rows / G <= n_img images, G in 1..8 with G A floats within 60 KB of LDS, an
 * img_of_row that says row / G or none, and row0 = 0.  parts: gridDim.y, 0 = ATT_PARTS. */
int icz_test_att_scores(int32_t route, const icz_test_att_scores_args* a, const icz_test_drop* drop, int32_t G, int32_t parts, void* stream);
/* att_ctx_kernel (G = 0) or att_ctx_group_kernel (G in 1..8, rows = G rows per image, no img_of_row but row / G, no alpha_out2):
 * alpha[row, :] = softmax over the image's regions of scores[row, :] (0 behind the count), written to alpha_out [rows, R] and (optional)
 * alpha_out2 with row stride alpha2_stride >= R; ctx[row, :] = sum_r alpha[row, r] feats[img, r, :]. */
int icz_test_att_ctx(const float* feats, int32_t n_img, const int32_t* img_of_row, const float* scores, float* alpha_out, float* alpha_out2,
                     int32_t alpha2_stride, float* ctx, int32_t rows, int32_t R, int32_t D, int32_t G, const int32_t* live, const int32_t* counts,
                     void* stream);
/* saved_alphas_kernel: src [T, B, NH, R] -> out [B, T, R], the fp32 mean over the NH heads added in head order. */
int icz_test_att_saved_alphas(const float* src, int32_t T, int32_t B, int32_t NH, int32_t R, float* out, void* stream);
/* att_bwd_dalpha_kernel: dctx = the sum of ns slabs (1..32) of rows rows of ldc floats (ldc >= D, a multiple of 4; columns 0..D);
 * dalpha_part[row][p][r] = dctx[row, 512 p .. 512 p + 512] . feats[img, r, the same columns] for r < c_img, [rows][ceil(D / 512)][R];
 * behind the count nothing is written. */
int icz_test_att_bwd_dalpha(const float* dctx, int32_t ns, int32_t ldc, int32_t rows, const float* feats, int32_t n_img, int32_t R, int32_t D,
                            float* dalpha_part, const int32_t* live, const int32_t* img_of_row, const int32_t* counts, void* stream);
/* att_bwd_ddec_kernel, every field of AttBwdDdecArgs: dalpha[row, r] = the nparts parts of dalpha [rows][nparts][R] added in order,
 * ds = alpha o (dalpha - alpha . dalpha) -> ds_out [rows, R] (0 behind the count); ddec[row, a] = sum_r on ds_r w_aff[a] (x 2 under
 * dropout) with on = (enc_ctx[img, r, a] + dec_ctx[row, a] > 0 in fp32) and kept.  A dead step writes zero ddec and ds rows.  row0 = 0. */
typedef struct {
    const float* enc_ctx; int32_t n_img;
    const float* dec_ctx; const float* w_aff; const float* alpha; const float* dalpha;
    float* ddec; float* ds_out;
    int32_t rows, R, A, nparts;
    const int32_t* live; const int32_t* img_of_row; const int32_t* counts;
} icz_test_att_ddec_args;
int icz_test_att_bwd_ddec(const icz_test_att_ddec_args* a, const icz_test_drop* drop, void* stream);
/* att_bwd_denc_kernel (G = 0) or att_bwd_denc_group_kernel (G >= 1: B = G rows of each of B / G <= n_img images, no img_of_row), every
 * field of AttBwdDencArgs: dec_all [T][Bs][A] and ds_all [T][Bs][R] (Bs 0 = B, else >= B rows per step of which the first B are taken:
 * pass the pointers at the row offset); on_t = (enc_ctx[img, r, a] + dec_all[t, row, a] > 0 in fp32) and kept, the keep flag of step t
 * from mask + t mask_step (mode 1; mask_step a multiple of 4, at least B R A) or Philox step t of `stream` (mode 2), index (row R + r) A + a;
 *   denc[row, r, a] = sum_t on_t ds_t[row, r] w_aff[a] (x 2 under dropout), rows behind the count zeros; grouped: the G rows of an
 *   image added in k order into denc[img];
 *   dwaff_part[row, p, a] = sum over the regions r = p mod parts and t of on_t (enc_ctx + dec_all) ds_t (x 2), [B or B / G][parts][A].
 * parts: gridDim.y, 0 = the library's rule (ATT_PARTS; grouped: as many parts of 16 regions as cover R, at least ATT_PARTS); a grouped
 * launch whose parts do not cover R is refused.  *parts_out (optional, host): the parts launched.  T R floats fit 60 KB of LDS. */
typedef struct {
    const float* enc_ctx; int32_t n_img;
    const float* dec_all; const float* ds_all; const float* w_aff;
    float* denc; float* dwaff_part;
    int32_t B, R, A, T;
    int32_t mode; const uint8_t* mask; int64_t mask_step; const uint64_t* seed; uint32_t stream;
    int32_t Bs;
    const int32_t* img_of_row; const int32_t* counts;
} icz_test_att_denc_args;
int icz_test_att_bwd_denc(const icz_test_att_denc_args* a, int32_t G, int32_t parts, int32_t* parts_out, void* stream);
/* Live timing of the dominant kernel (the forward GEMMs of a decoder step at 33..64 rows: gemm_resident_x3_kernel, or
 * gemm_nt_kernel<4, ...> with ICZ_GEMM_RESIDENT_X3=0; see icz_prof_select) with HIP events on its launch stream, for bench.py's
 * roofline line.  Between begin and end every launch is bracketed by an event
 * pair; end synchronises on them and reports the average duration [us] and the ALGORITHMIC bytes / flops per launch
 * (A read once + W read once + C written once; 2MNK). */
int icz_prof_begin(void);
/* Which launches icz_prof_begin brackets: 0 (default) = every forward GEMM of a decoder step at 33..64 rows, whatever kernel
 * takes it; 1 = only the launches of the resident-activation split-precision kernel (gemm_resident_x3_kernel: the LSTM-gate
 * and vocabulary-projection GEMMs, the dominant kernel of the SCST step since round 2). */
int icz_prof_select(int32_t which);
/* Average time [us] of an event pair around an EMPTY kernel on `stream` (n pairs): what the pair itself and the dispatch
 * of the bracketed kernel add to every duration icz_prof_end reports. */
int icz_prof_pair_overhead(void* stream, int32_t n, double* avg_us);
int icz_prof_end(double* avg_us, double* bytes_per_launch, double* flops_per_launch, long long* launches);
/* The same for the small kernels of a BUTD decoder step (bench.py's roofline entries of the attention trio and the select kernels):
 * between icz_kprof_begin and icz_kprof_end every EAGER launch (never inside a captured graph) of a group is bracketed by an event
 * pair on its stream.  Groups: 0 = SoftAttention.forward (BUTD_Model.py:49-62: dec_att product + scores + softmax / weighted sum,
 * three launches), 1 = greedy token choice + next embedding (:183), 2 = multinomial draw + log-prob + next embedding (:221-233),
 * 3 = one LSTMCell's pointwise part (:82-83).  icz_kprof_end synchronises and reports the average pair time [us] and the count. */
int icz_kprof_begin(void);
int icz_kprof_end(int32_t group, double* avg_us, long long* pairs);
/* What THIS box streams from HBM (bench.py's roofline.peak_measured, beside the 8 TB/s specification): a read-only kernel over
 * `buf` (`bytes` a multiple of 65536, at least 64 MiB; take it well above the 256 MB Infinity Cache), 64 KB chunks dealt to workgroups, sixteen
 * 16-byte loads in flight per lane, `reps` launches timed with one HIP event pair on `stream`; *gbs = bytes * reps / time. */
int icz_prof_stream_rate(const void* buf, size_t bytes, int32_t reps, void* stream, double* gbs);

#ifdef __cplusplus
}
#endif
#endif /* ICZ_H_ */
