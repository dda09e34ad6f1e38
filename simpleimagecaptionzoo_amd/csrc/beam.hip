// Batched beam search (DecoderRNN.beam_search_sample, Models/BUTD_Model.py:236-318) for many images at once, one driver for the
// BUTD, AoA and NIC decoders and their ensembles (DecodeMember, decoder_core.h).
// The reference decodes one image per call with a Python list comprehension over tensor elements every step
// (k host syncs per step, :282-283).  Here every image owns k consecutive decoder rows; after the shared decoder
// step a per-image workgroup does log-softmax + running score + top-k over (active beams x V), retires beams that
// emitted <end> (k shrinks exactly as in the reference; no length normalisation unless icz_beam_opts asks for it), and emits the row permutation
// that re-gathers the LSTM state.  No host synchronisation inside a step.
#include <cmath>

#include "beam_kernels.h"
#include "decoder_core.h"

namespace icz {

int BeamBuf::check(const char* who, int n_img, int k, int max_steps, int max_rows) {
    ICZ_REQUIRE(k >= 1 && k <= BEAM_MAX_K, "%s beam: beam size %d out of range 1..%d", who, k, BEAM_MAX_K);
    ICZ_REQUIRE(n_img > 0 && (long)n_img * k <= max_rows, "%s beam: %d images x %d beams exceed row capacity %d", who, n_img, k, max_rows);
    ICZ_REQUIRE(max_steps >= 1 && max_steps <= 256, "%s beam: max_steps out of range", who);
    return ICZ_OK;
}

const icz_beam_opts BeamBuf::defaults = {1, 0, 0, 0.f};

int BeamBuf::check_opts(const char* who, int k, const icz_beam_opts* o) {
    ICZ_REQUIRE(o, "%s: null options", who);
    ICZ_REQUIRE(o->n_best >= 1 && o->n_best <= k, "%s: n_best %d outside 1..beam (%d)", who, o->n_best, k);
    ICZ_REQUIRE(o->block_ngram == 0 || (o->block_ngram >= 2 && o->block_ngram <= 4), "%s: block_ngram %d not 0, 2, 3 or 4", who,
                o->block_ngram);
    ICZ_REQUIRE(o->lp_kind >= 0 && o->lp_kind <= 2, "%s: lp_kind %d unknown (0 none, 1 avg, 2 wu)", who, o->lp_kind);
    ICZ_REQUIRE(std::isfinite(o->lp_alpha) && o->lp_alpha >= 0.f, "%s: lp_alpha %g negative or not finite", who, (double)o->lp_alpha);
    return ICZ_OK;
}

const icz_beam_diversity BeamBuf::no_diversity = {1, 0.f};

int BeamBuf::check_diversity(const char* who, int k, const icz_beam_diversity* d) {
    ICZ_REQUIRE(d, "%s: null diversity", who);
    ICZ_REQUIRE(d->groups >= 1 && d->groups <= k && k % d->groups == 0, "%s: groups %d outside 1..beam (%d) or not dividing it", who,
                d->groups, k);
    ICZ_REQUIRE(std::isfinite(d->diversity) && d->diversity >= 0.f, "%s: diversity %g negative or not finite", who, (double)d->diversity);
    return ICZ_OK;
}

int BeamBuf::check_constraints(const char* who, int n_img, int beam, const icz_beam_constraints* c, bool* any) {
    ICZ_REQUIRE(c, "%s: null constraints", who);
    const int C = c->max_constraints, A = c->max_alts;
    ICZ_REQUIRE(C >= 0 && C <= BEAM_CONS_MAX_C, "%s: max_constraints %d outside 0..%d", who, C, BEAM_CONS_MAX_C);
    ICZ_REQUIRE(A >= 1 && A <= BEAM_CONS_MAX_A, "%s: max_alts %d outside 1..%d", who, A, BEAM_CONS_MAX_A);
    ICZ_REQUIRE(C == 0 || (c->words_dev && c->words_host), "%s: null constraint words (device and host copies are both needed)", who);
    ICZ_REQUIRE(beam >= 1 && beam <= BEAM_MAX_K, "%s: beam size %d out of range 1..%d", who, beam, BEAM_MAX_K);
    ICZ_REQUIRE((beam << C) <= BEAM_CONS_MAX_ROWS, "%s: 2^%d states x %d beams exceed %d rows per image", who, C, beam, BEAM_CONS_MAX_ROWS);
    ICZ_REQUIRE(n_img > 0, "%s: n_img %d", who, n_img);
    *any = false;
    for (int img = 0; img < n_img && C > 0; ++img) {
        const int32_t* w = c->words_host + (size_t)img * C * A;
        bool ended = false;                        // constraints filled from the left
        for (int q = 0; q < C; ++q) {
            const bool empty = w[q * A] < 0;
            ICZ_REQUIRE(!(ended && !empty), "%s: image %d: constraint %d behind an empty one (fill from the left)", who, img, q);
            ended = ended || empty;
            bool gap = false;                      // alternatives filled from the left
            for (int a = 0; a < A; ++a) {
                const int v = w[q * A + a];
                ICZ_REQUIRE(v >= -1, "%s: image %d: word id %d", who, img, v);
                ICZ_REQUIRE(!(gap && v >= 0), "%s: image %d, constraint %d: word behind an empty slot (fill from the left)", who, img, q);
                gap = gap || v < 0;
                if (v < 0) continue;
                ICZ_REQUIRE(v > 2, "%s: image %d: word id %d is <pad>, <sta> or <end>", who, img, v);
                for (int p = 0; p < q * A + a; ++p) ICZ_REQUIRE(w[p] != v, "%s: image %d: word id %d appears twice", who, img, v);
                *any = true;
            }
        }
    }
    return ICZ_OK;
}

int BeamBuf::check_constraint_vocab(const char* who, int n_img, int V, const icz_beam_constraints* c) {
    const size_t n = (size_t)n_img * c->max_constraints * c->max_alts;
    for (size_t i = 0; i < n; ++i)
        ICZ_REQUIRE(c->words_host[i] < V, "%s: constraint word id %d outside the vocabulary (%d)", who, c->words_host[i], V);
    ICZ_REQUIRE(((long)V << c->max_constraints) * BEAM_MAX_K < 0x7fffffff, "%s: vocabulary %d too large for %d constraints", who, V, c->max_constraints);
    return ICZ_OK;
}

// sized for the handle's row capacity and at least 51 columns; a longer search re-allocates (the old buffers stay in the
// handle's persistent list), the pinned read-back word is allocated once
int BeamBuf::ensure(DeviceBuffers& m, int max_rows, int L) {
    if (cap_rows >= max_rows && cap_L >= L) return ICZ_OK;
    const size_t R_ = max_rows, L_ = L > 51 ? L : 51;
    ICZ_TRY(m.alloc((void**)&n_act, sizeof(int) * R_));
    ICZ_TRY(m.alloc((void**)&run, sizeof(float) * R_));
    ICZ_TRY(m.alloc((void**)&seqs[0], sizeof(int32_t) * R_ * L_));
    ICZ_TRY(m.alloc((void**)&seqs[1], sizeof(int32_t) * R_ * L_));
    ICZ_TRY(m.alloc((void**)&src_row, sizeof(int32_t) * R_));
    ICZ_TRY(m.alloc((void**)&img_of_row, sizeof(int32_t) * R_));
    ICZ_TRY(m.alloc((void**)&best_score, sizeof(float) * R_));
    ICZ_TRY(m.alloc((void**)&best_len, sizeof(int) * R_));
    ICZ_TRY(m.alloc((void**)&has_complete, sizeof(int) * R_));
    ICZ_TRY(m.alloc((void**)&best_seq, sizeof(int32_t) * R_ * L_));
    ICZ_TRY(m.alloc((void**)&n_live, sizeof(int) * 260));
    ICZ_TRY(m.alloc((void**)&cand_val, sizeof(float) * R_ * BEAM_MAX_K));
    ICZ_TRY(m.alloc((void**)&cand_idx, sizeof(int) * R_ * BEAM_MAX_K));
    ICZ_TRY(m.alloc((void**)&hyp_seq, sizeof(int32_t) * R_ * L_));
    ICZ_TRY(m.alloc((void**)&hyp_score, sizeof(float) * R_));
    ICZ_TRY(m.alloc((void**)&hyp_len, sizeof(int) * R_));
    ICZ_TRY(m.alloc((void**)&hyp_cnt, sizeof(int) * R_));
    ICZ_TRY(m.alloc((void**)&it, sizeof(int64_t) * R_));
    ICZ_TRY(m.alloc((void**)&cap, sizeof(int) * R_));
    ICZ_TRY(m.alloc((void**)&force_val, sizeof(float) * R_ * BEAM_CONS_SLOTS));
    ICZ_TRY(m.alloc((void**)&hyp_state, sizeof(int32_t) * R_));
    if (!n_live_host) ICZ_CHECK_HIP(hipHostMalloc((void**)&n_live_host, sizeof(int) * 4, 0));
    ICZ_TRY(m.synced());
    cap_rows = (int)R_;
    cap_L = (int)L_;
    return ICZ_OK;
}

int BeamBuf::begin(int n_img, int k, int L, hipStream_t st, int states) {
    const int rows = n_img * k;
    ICZ_CHECK_HIP(hipMemsetAsync(n_live, 0, sizeof(int) * 260, st));
    ICZ_CHECK_HIP(hipMemsetAsync(run, 0, sizeof(float) * rows, st));
    hipLaunchKernelGGL(beam_init_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, n_img, k, L, n_act, seqs[0], img_of_row, it, has_complete, best_score,
                       hyp_cnt);
    if (states > 1)
        hipLaunchKernelGGL(beam_init_states_kernel, dim3(cdiv(n_img * states, 256)), dim3(256), 0, st, n_img * states, states, k / states, n_act, cap);
    return ICZ_OK;
}

int BeamBuf::search(DecodeMember* const* m, int M, const BeamCombine* ens, int n_img, int k, int max_steps, float* seqs_out, int32_t* lens_out,
                    const icz_beam_opts& o, const icz_beam_diversity& d, float* scores_out, hipStream_t st, const icz_beam_constraints* cons,
                    int32_t* sat_out) {
    const int rows = n_img * k, L = max_steps + 1, G = d.groups, V = m[0]->vocab();
    const bool listed = o.n_best > 1 || o.lp_kind != 0 || G > 1 || cons;
    const BeamCons cn = cons ? BeamCons{cons->words_dev, cons->max_constraints, cons->max_alts, k >> cons->max_constraints, cap, force_val, hyp_state}
                             : BeamCons{};
    bool compact_first = true;
    for (int i = 0; i < M; ++i) compact_first = compact_first && m[i]->compact_step();
    if (G > 1) hipLaunchKernelGGL(beam_init_groups_kernel, dim3(cdiv(n_img * G, 256)), dim3(256), 0, st, n_img * G, k / G, n_act);
    LogitsView lv[ENS_MAX_M];
    int sb = 0, steps_done = 0;
    for (int s = 1; s <= max_steps; ++s) {
        // Step 1 (compact): the decoder runs ONE row per image (row img of the buffers); the top-k kernel reads image img's logits from
        // row img and the state gather fans row img out to the image's k rows.
        const bool compact = compact_first && s == 1 && k > 1;
        const int r = compact ? n_img : rows;
        // a single handle's consumer reads finished rows; the ensemble's combine kernel sums split-K slabs itself
        for (int i = 0; i < M; ++i) ICZ_TRY(m[i]->step(r, it, compact ? nullptr : img_of_row, compact ? 1 : k, 0, ens != nullptr, &lv[i], st));
        if (ens) ens->run(lv, r);
        BeamArgs a = {ens ? ens->lp : lv[0].p, V, ens ? ens->ld : lv[0].ld, k, s, L, n_act, run, seqs[sb], seqs[sb ^ 1], src_row, it, best_score,
                      best_len, best_seq, has_complete, n_live + s, listed ? hyp_seq : nullptr, hyp_score, hyp_len, listed ? hyp_cnt : nullptr};
        if (cons)
            launch_beam_rowtopk_cons(st, rows, a.logits, a.V, a.ldl, a.k, a.step, (const int*)n_act, (const float*)run, cand_val, cand_idx,
                                     compact ? 1 : 0, seqs[sb], L, o.block_ngram, BEAM_ROUTE_AUTO, cn);
        else
            launch_beam_rowtopk(st, rows, a.logits, a.V, a.ldl, a.k, a.step, (const int*)n_act, (const float*)run, cand_val, cand_idx,
                                compact ? 1 : 0, seqs[sb], L, o.block_ngram, G, BEAM_ROUTE_AUTO);
        if (cons)
            hipLaunchKernelGGL(beam_merge_states_kernel, dim3(n_img), dim3(64), 0, st, a, cn, (const float*)cand_val, (const int*)cand_idx);
        else if (G > 1)
            hipLaunchKernelGGL(beam_merge_groups_kernel, dim3(n_img), dim3(64), 0, st, a, G, d.diversity, (const float*)cand_val,
                               (const int*)cand_idx);
        else
            hipLaunchKernelGGL(beam_merge_kernel, dim3(n_img), dim3(64), 0, st, a, (const float*)cand_val, (const int*)cand_idx);
        for (int i = 0; i < M; ++i) m[i]->gather(src_row, rows, compact ? k : 1, st);
        sb ^= 1;
        steps_done = s;
        if (s >= 6 && (s % 3) == 0 && s < max_steps) {
            ICZ_CHECK_HIP(hipMemcpyAsync(n_live_host, n_live + s, sizeof(int), hipMemcpyDeviceToHost, st));
            ICZ_CHECK_HIP(hipStreamSynchronize(st));
            if (n_live_host[0] == 0) break;
        }
    }
    if (cons)
        hipLaunchKernelGGL(beam_finalize_states_kernel, dim3(n_img), dim3(64), 0, st, k, cn.beam, 1 << cn.C, L, steps_done, o.n_best, o.lp_kind,
                           o.lp_alpha, (const int*)n_act, (const float*)run, (const int32_t*)seqs[sb], (const int*)hyp_cnt, (const float*)hyp_score,
                           (const int*)hyp_len, (const int32_t*)hyp_state, (const int32_t*)hyp_seq, seqs_out, lens_out, scores_out, sat_out);
    else if (G > 1)
        hipLaunchKernelGGL(beam_finalize_nbest_kernel<true>, dim3(n_img), dim3(64), 0, st, k, L, steps_done, o.n_best, o.lp_kind, o.lp_alpha,
                           (const int*)n_act, (const float*)run, (const int32_t*)seqs[sb], (const int*)hyp_cnt, (const float*)hyp_score,
                           (const int*)hyp_len, (const int32_t*)hyp_seq, seqs_out, lens_out, scores_out, G);
    else if (listed)
        hipLaunchKernelGGL(beam_finalize_nbest_kernel<false>, dim3(n_img), dim3(64), 0, st, k, L, steps_done, o.n_best, o.lp_kind, o.lp_alpha,
                           (const int*)n_act, (const float*)run, (const int32_t*)seqs[sb], (const int*)hyp_cnt, (const float*)hyp_score,
                           (const int*)hyp_len, (const int32_t*)hyp_seq, seqs_out, lens_out, scores_out, 1);
    else
        hipLaunchKernelGGL(beam_finalize_kernel, dim3(n_img), dim3(64), 0, st, k, L, steps_done, n_act, run, seqs[sb], has_complete,
                           best_len, best_seq, seqs_out, lens_out, (const float*)best_score, scores_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int check_members(const char* who, DecodeMember* const* m, int M, const float* const* feats, int rows) {
    ICZ_REQUIRE(feats, "%s: null features", who);
    for (int i = 0; i < M; ++i) {
        ICZ_REQUIRE(feats[i], "%s: null features of member %d", who, i);
        ICZ_REQUIRE(m[i]->refreshed(), "%s: member %d is not refreshed (call its icz_*_refresh_weights after binding/updating parameters)", who, i);
        ICZ_REQUIRE(rows <= m[i]->row_capacity(), "%s: %d rows exceed member %d's row capacity %d", who, rows, i, m[i]->row_capacity());
    }
    return ICZ_OK;
}

// Every check runs before the first allocation or launch: a refused call queues nothing.  begin() precedes the prologues: NIC's (and so
// an ensemble's) reads img_of_row, which begin() writes; begin() writes only the beam buffers and a prologue only its handle's
// per-image tensors and state, so for BUTD and AoA the order of the two is free.
int beam_search(const char* who, DecodeMember* const* m, int M, const BeamCombine* ens, const float* const* feats, int n_img, int k,
                int max_steps, const icz_beam_opts& o, const icz_beam_diversity& d, float* seqs_out, int32_t* lens_out, float* scores_out,
                hipStream_t st, const icz_beam_constraints* cons, int32_t* sat_out) {
    if (!ens) ICZ_REQUIRE(feats[0] && seqs_out && lens_out, "%s beam: null argument", who);
    const int S = cons ? 1 << cons->max_constraints : 1, beam = k;
    ICZ_TRY(BeamBuf::check(who, n_img, beam, max_steps, (ens ? 1 << 30 : m[0]->row_capacity()) / S));
    if (cons) ICZ_TRY(BeamBuf::check_constraint_vocab(who, n_img, m[0]->vocab(), cons));
    k = S * beam;                                  // decoder rows per image
    if (ens) ICZ_TRY(check_members(ens->who, m, M, feats, n_img * k));
    else ICZ_REQUIRE(m[0]->refreshed(), "%s: call icz_%s_refresh_weights after binding/updating parameters", who, who);
    BeamBuf& bm = ens ? *ens->bm : m[0]->bm;
    const int L = max_steps + 1;
    ICZ_TRY(bm.ensure(ens ? *ens->mem : m[0]->buffers(), ens ? ens->cap : m[0]->row_capacity(), L));
    ICZ_TRY(bm.begin(n_img, k, L, st, S));
    for (int i = 0; i < M; ++i) ICZ_TRY(m[i]->prologue(feats[i], n_img, k, bm.img_of_row, st));
    if (sat_out && !cons) ICZ_CHECK_HIP(hipMemsetAsync(sat_out, 0, sizeof(int32_t) * n_img * o.n_best, st));      // no constraints: every state is 0
    return bm.search(m, M, ens, n_img, k, max_steps, seqs_out, lens_out, o, d, scores_out, st, cons, sat_out);
}

int beam_constrained_args(const char* entry, int n_img, int beam, const icz_beam_opts* opts, const icz_beam_constraints* cons, bool ptrs_ok,
                          const icz_beam_constraints** cons_out) {
    ICZ_TRY(BeamBuf::check_opts(entry, beam, opts));
    bool any = false;
    ICZ_TRY(BeamBuf::check_constraints(entry, n_img, beam, cons, &any));
    ICZ_REQUIRE(ptrs_ok, "%s: null argument", entry);
    *cons_out = any ? cons : nullptr;
    return ICZ_OK;
}

// A family's icz_*_beam_search_constrained on its member m (null for a null handle)
static int beam_constrained_entry(const char* entry, const char* who, DecodeMember* m, const float* feats, int n_img, int beam, int max_steps,
                                  const icz_beam_opts* opts, const icz_beam_constraints* cons, float* seqs_out, int32_t* lens_out,
                                  float* scores_out, int32_t* sat_out, void* stream) {
    const icz_beam_constraints* use = nullptr;
    ICZ_TRY(beam_constrained_args(entry, n_img, beam, opts, cons, feats && seqs_out && lens_out && scores_out && sat_out, &use));
    ICZ_REQUIRE(m, "%s: null handle", entry);
    return beam_search(who, &m, 1, nullptr, &feats, n_img, beam, max_steps, *opts, BeamBuf::no_diversity, seqs_out, lens_out, scores_out,
                       (hipStream_t)stream, use, sat_out);
}

// The three beam entries of a family on its member m (null for a null handle): plain (the default options, scores_out may be
// null), _opts and _diverse.  `entry` names the C entry in the argument errors, `who` the family in the search's own.
enum BeamEntry { BEAM_PLAIN, BEAM_OPTS, BEAM_DIVERSE };
static int beam_entry(BeamEntry kind, const char* entry, const char* who, DecodeMember* m, const float* feats, int n_img, int beam, int max_steps,
                      const icz_beam_opts* opts, const icz_beam_diversity* div, float* seqs_out, int32_t* lens_out, float* scores_out,
                      void* stream) {
    if (kind == BEAM_PLAIN) {
        ICZ_REQUIRE(m, "null handle");
    } else {
        ICZ_TRY(BeamBuf::check_opts(entry, beam, opts));      // the arguments first: no handle needed to report them
        if (kind == BEAM_DIVERSE) ICZ_TRY(BeamBuf::check_diversity(entry, beam, div));
        ICZ_REQUIRE(feats && seqs_out && lens_out && scores_out, "%s: null argument", entry);
        ICZ_REQUIRE(m, "%s: null handle", entry);
    }
    return beam_search(who, &m, 1, nullptr, &feats, n_img, beam, max_steps, *opts, *div, seqs_out, lens_out, scores_out, (hipStream_t)stream);
}

}  // namespace icz

// ================================================================================================
using namespace icz;
extern "C" {

int icz_butd_beam_search(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps, float* seqs_out, int32_t* lens_out,
                         void* stream) {
    return beam_entry(BEAM_PLAIN, "icz_butd_beam_search", "butd", butd_member(h), feats, n_img, beam, max_steps, &BeamBuf::defaults, &BeamBuf::no_diversity,
                      seqs_out, lens_out, nullptr, stream);
}
int icz_butd_beam_search_opts(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps, const icz_beam_opts* opts,
                              float* seqs_out, int32_t* lens_out, float* scores_out, void* stream) {
    return beam_entry(BEAM_OPTS, "icz_butd_beam_search_opts", "butd", butd_member(h), feats, n_img, beam, max_steps, opts, &BeamBuf::no_diversity, seqs_out,
                      lens_out, scores_out, stream);
}
int icz_butd_beam_search_diverse(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps, const icz_beam_opts* opts,
                                 const icz_beam_diversity* div, float* seqs_out, int32_t* lens_out, float* scores_out, void* stream) {
    return beam_entry(BEAM_DIVERSE, "icz_butd_beam_search_diverse", "butd", butd_member(h), feats, n_img, beam, max_steps, opts, div, seqs_out, lens_out,
                      scores_out, stream);
}
int icz_aoa_beam_search(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps, float* seqs_out, int32_t* lens_out,
                        void* stream) {
    return beam_entry(BEAM_PLAIN, "icz_aoa_beam_search", "aoa", aoa_member(h), feats, n_img, beam, max_steps, &BeamBuf::defaults, &BeamBuf::no_diversity,
                      seqs_out, lens_out, nullptr, stream);
}
int icz_aoa_beam_search_opts(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps, const icz_beam_opts* opts,
                             float* seqs_out, int32_t* lens_out, float* scores_out, void* stream) {
    return beam_entry(BEAM_OPTS, "icz_aoa_beam_search_opts", "aoa", aoa_member(h), feats, n_img, beam, max_steps, opts, &BeamBuf::no_diversity, seqs_out,
                      lens_out, scores_out, stream);
}
int icz_aoa_beam_search_diverse(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps, const icz_beam_opts* opts,
                                const icz_beam_diversity* div, float* seqs_out, int32_t* lens_out, float* scores_out, void* stream) {
    return beam_entry(BEAM_DIVERSE, "icz_aoa_beam_search_diverse", "aoa", aoa_member(h), feats, n_img, beam, max_steps, opts, div, seqs_out, lens_out,
                      scores_out, stream);
}
int icz_nic_beam_search(icz_nic_t* h, const float* features, int32_t n_img, int32_t beam, int32_t max_steps, float* seqs_out, int32_t* lens_out,
                        void* stream) {
    return beam_entry(BEAM_PLAIN, "icz_nic_beam_search", "nic", nic_member(h), features, n_img, beam, max_steps, &BeamBuf::defaults, &BeamBuf::no_diversity,
                      seqs_out, lens_out, nullptr, stream);
}
int icz_nic_beam_search_opts(icz_nic_t* h, const float* features, int32_t n_img, int32_t beam, int32_t max_steps, const icz_beam_opts* opts,
                             float* seqs_out, int32_t* lens_out, float* scores_out, void* stream) {
    return beam_entry(BEAM_OPTS, "icz_nic_beam_search_opts", "nic", nic_member(h), features, n_img, beam, max_steps, opts, &BeamBuf::no_diversity, seqs_out,
                      lens_out, scores_out, stream);
}
int icz_nic_beam_search_diverse(icz_nic_t* h, const float* features, int32_t n_img, int32_t beam, int32_t max_steps, const icz_beam_opts* opts,
                                const icz_beam_diversity* div, float* seqs_out, int32_t* lens_out, float* scores_out, void* stream) {
    return beam_entry(BEAM_DIVERSE, "icz_nic_beam_search_diverse", "nic", nic_member(h), features, n_img, beam, max_steps, opts, div, seqs_out, lens_out,
                      scores_out, stream);
}

int icz_butd_beam_search_constrained(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps, const icz_beam_opts* opts,
                                     const icz_beam_constraints* cons, float* seqs_out, int32_t* lens_out, float* scores_out, int32_t* sat_out,
                                     void* stream) {
    return beam_constrained_entry("icz_butd_beam_search_constrained", "butd", butd_member(h), feats, n_img, beam, max_steps, opts, cons, seqs_out,
                                  lens_out, scores_out, sat_out, stream);
}
int icz_aoa_beam_search_constrained(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps, const icz_beam_opts* opts,
                                    const icz_beam_constraints* cons, float* seqs_out, int32_t* lens_out, float* scores_out, int32_t* sat_out,
                                    void* stream) {
    return beam_constrained_entry("icz_aoa_beam_search_constrained", "aoa", aoa_member(h), feats, n_img, beam, max_steps, opts, cons, seqs_out,
                                  lens_out, scores_out, sat_out, stream);
}
int icz_nic_beam_search_constrained(icz_nic_t* h, const float* features, int32_t n_img, int32_t beam, int32_t max_steps, const icz_beam_opts* opts,
                                    const icz_beam_constraints* cons, float* seqs_out, int32_t* lens_out, float* scores_out, int32_t* sat_out,
                                    void* stream) {
    return beam_constrained_entry("icz_nic_beam_search_constrained", "nic", nic_member(h), features, n_img, beam, max_steps, opts, cons, seqs_out,
                                  lens_out, scores_out, sat_out, stream);
}

// ------------------------------------------------------------------------------------------------
// Test entries of the beam step's kernels (include/icz.h): the arguments are checked on the host, then the kernels are launched through
// launch_beam_rowtopk and with the grids of BeamBuf::search, nothing more.
static int beam_test_shape(const char* who, int route, const float* logits, int n_img, int k, int V, int ldl, int step, int L, int compact,
                           int ngram, int groups) {
    ICZ_REQUIRE(k >= 1 && k <= BEAM_MAX_K, "%s: beam size k=%d outside 1..%d", who, k, BEAM_MAX_K);
    ICZ_REQUIRE(groups >= 1 && groups <= k && k % groups == 0, "%s: groups=%d outside 1..k (%d) or not dividing it", who, groups, k);
    ICZ_REQUIRE(n_img >= 1 && (long)n_img * k <= (1 << 20), "%s: n_img=%d", who, n_img);
    ICZ_REQUIRE(step >= 1 && step <= 256 && L > step, "%s: step=%d outside 1..256 or not below L=%d", who, step, L);
    ICZ_REQUIRE(ngram == 0 || (ngram >= 2 && ngram <= 4), "%s: ngram=%d not 0, 2, 3 or 4", who, ngram);
    ICZ_REQUIRE(compact == 0 || (compact == 1 && step == 1), "%s: compact=%d at step %d (0, or 1 at step 1)", who, compact, step);
    ICZ_REQUIRE(V >= 1 && ldl >= V && (long)V * k < 0x7fffffff, "%s: V=%d, ldl=%d", who, V, ldl);
    ICZ_REQUIRE(route >= BEAM_ROUTE_AUTO && route <= BEAM_ROUTE_SWEEP, "%s: route=%d", who, route);
    ICZ_REQUIRE(beam_rowtopk_route_fits(route, V, ldl, ((uintptr_t)logits & 15) == 0),
                "%s: route %d cannot take V=%d, ldl=%d, base %s (register kernels: 16-byte rows of at least V rounded up to 4, V <= %d)", who,
                route, V, ldl, ((uintptr_t)logits & 15) == 0 ? "aligned" : "not 16-byte aligned", route == BEAM_ROUTE_REG3 ? 3072 : 10240);
    return ICZ_OK;
}

int icz_beam_rowtopk_route_for(int32_t V, int32_t ldl, int32_t base_aligned) {
    ICZ_REQUIRE(V >= 1 && ldl >= V, "icz_beam_rowtopk_route_for: V=%d, ldl=%d", V, ldl);
    return beam_rowtopk_route(V, ldl, base_aligned != 0);
}

int icz_test_beam_rowtopk(int32_t route, const float* logits, int32_t n_img, int32_t k, int32_t V, int32_t ldl, int32_t step, const int32_t* n_act,
                          const float* run, int32_t compact, const int32_t* seqs_in, int32_t L, int32_t ngram, int32_t groups, float* cand_val,
                          int32_t* cand_idx, void* stream) {
    const char* who = "icz_test_beam_rowtopk";
    ICZ_REQUIRE(logits && n_act && run && cand_val && cand_idx && (seqs_in || !ngram), "%s: null argument", who);
    ICZ_TRY(beam_test_shape(who, route, logits, n_img, k, V, ldl, step, L, compact, ngram, groups));
    launch_beam_rowtopk((hipStream_t)stream, n_img * k, logits, V, ldl, k, step, n_act, run, cand_val, cand_idx, compact, seqs_in, L, ngram, groups,
                        route);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_beam_step(int32_t route, const icz_beam_step_state* s, int32_t n_img, int32_t k, int32_t V, int32_t ldl, int32_t step, int32_t L,
                       int32_t compact, int32_t ngram, int32_t groups, float lambda, void* stream) {
    const char* who = "icz_test_beam_step";
    ICZ_REQUIRE(s, "%s: null state", who);
    ICZ_REQUIRE(s->logits && s->n_act && s->run && s->seqs_in && s->seqs_out && s->src_row && s->it_next && s->best_score && s->best_len &&
                    s->best_seq && s->has_complete && s->n_live && s->cand_val && s->cand_idx,
                "%s: null argument", who);
    const bool listed = s->hyp_seq && s->hyp_score && s->hyp_len && s->hyp_cnt;
    ICZ_REQUIRE(listed || (!s->hyp_seq && !s->hyp_score && !s->hyp_len && !s->hyp_cnt), "%s: the n-best list is four pointers or none", who);
    ICZ_REQUIRE(s->seqs_in != s->seqs_out, "%s: seqs_in and seqs_out are the same buffer", who);
    ICZ_TRY(beam_test_shape(who, route, s->logits, n_img, k, V, ldl, step, L, compact, ngram, groups));
    ICZ_REQUIRE(groups == 1 || listed, "%s: a grouped step needs the n-best list", who);
    ICZ_REQUIRE(std::isfinite(lambda) && lambda >= 0.f && (groups > 1 || lambda == 0.f), "%s: lambda=%g negative, not finite, or without groups", who,
                (double)lambda);
    hipStream_t st = (hipStream_t)stream;
    BeamArgs a = {s->logits, V, ldl, k, step, L, s->n_act, s->run, s->seqs_in, s->seqs_out, s->src_row, s->it_next, s->best_score, s->best_len,
                  s->best_seq, s->has_complete, s->n_live, s->hyp_seq, s->hyp_score, s->hyp_len, s->hyp_cnt};
    launch_beam_rowtopk(st, n_img * k, a.logits, V, ldl, k, step, (const int*)s->n_act, (const float*)s->run, s->cand_val, s->cand_idx, compact,
                        s->seqs_in, L, ngram, groups, route);
    if (groups > 1)
        hipLaunchKernelGGL(beam_merge_groups_kernel, dim3(n_img), dim3(64), 0, st, a, groups, lambda, (const float*)s->cand_val,
                           (const int*)s->cand_idx);
    else
        hipLaunchKernelGGL(beam_merge_kernel, dim3(n_img), dim3(64), 0, st, a, (const float*)s->cand_val, (const int*)s->cand_idx);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_beam_finalize(int32_t form, int32_t n_img, int32_t k, int32_t L, int32_t steps_done, int32_t n_best, int32_t lp_kind, float lp_alpha,
                           int32_t groups, const int32_t* n_act, const float* run, const int32_t* seqs, const int32_t* has_complete,
                           const float* best_score, const int32_t* best_len, const int32_t* best_seq, const int32_t* hyp_cnt, const float* hyp_score,
                           const int32_t* hyp_len, const int32_t* hyp_seq, float* out, int32_t* lens, float* scores, void* stream) {
    const char* who = "icz_test_beam_finalize";
    ICZ_REQUIRE(form >= 0 && form <= 2, "%s: form=%d (0 best, 1 n-best, 2 grouped n-best)", who, form);
    ICZ_REQUIRE(k >= 1 && k <= BEAM_MAX_K, "%s: beam size k=%d outside 1..%d", who, k, BEAM_MAX_K);
    ICZ_REQUIRE(groups >= 1 && groups <= k && k % groups == 0 && (form == 2 || groups == 1), "%s: groups=%d outside 1..k (%d), not dividing it, or on form %d",
                who, groups, k, form);
    ICZ_REQUIRE(n_img >= 1 && (long)n_img * k <= (1 << 20), "%s: n_img=%d", who, n_img);
    ICZ_REQUIRE(steps_done >= 1 && steps_done <= 256 && L > steps_done, "%s: steps_done=%d outside 1..256 or not below L=%d", who, steps_done, L);
    ICZ_REQUIRE(n_act && run && seqs && out && lens, "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    if (form == 0) {
        ICZ_REQUIRE(has_complete && best_len && best_seq && (best_score || !scores), "%s: null argument", who);
        ICZ_REQUIRE(n_best == 1, "%s: n_best=%d on form 0", who, n_best);
        hipLaunchKernelGGL(beam_finalize_kernel, dim3(n_img), dim3(64), 0, st, k, L, steps_done, n_act, run, seqs, has_complete, best_len, best_seq,
                           out, lens, best_score, scores);
    } else {
        const icz_beam_opts o = {n_best, 0, lp_kind, lp_alpha};
        ICZ_TRY(BeamBuf::check_opts(who, k, &o));
        ICZ_REQUIRE(hyp_cnt && hyp_score && hyp_len && hyp_seq && scores, "%s: null argument", who);
        if (form == 2)
            hipLaunchKernelGGL(beam_finalize_nbest_kernel<true>, dim3(n_img), dim3(64), 0, st, k, L, steps_done, n_best, lp_kind, lp_alpha, n_act, run,
                               seqs, hyp_cnt, hyp_score, hyp_len, hyp_seq, out, lens, scores, groups);
        else
            hipLaunchKernelGGL(beam_finalize_nbest_kernel<false>, dim3(n_img), dim3(64), 0, st, k, L, steps_done, n_best, lp_kind, lp_alpha, n_act, run,
                               seqs, hyp_cnt, hyp_score, hyp_len, hyp_seq, out, lens, scores, 1);
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// ---- the constrained step's kernels: the shape rules of beam_test_shape on k = 2^C * beam rows per image
static int beam_test_states_shape(const char* who, int route, const float* logits, int n_img, int beam, int C, int A, int V, int ldl, int step,
                                  int L, int compact, int ngram) {
    ICZ_REQUIRE(beam >= 1 && beam <= BEAM_MAX_K, "%s: beam=%d outside 1..%d", who, beam, BEAM_MAX_K);
    ICZ_REQUIRE(C >= 0 && C <= BEAM_CONS_MAX_C && (beam << C) <= BEAM_CONS_MAX_ROWS, "%s: C=%d outside 0..%d or 2^C * beam above %d", who, C,
                BEAM_CONS_MAX_C, BEAM_CONS_MAX_ROWS);
    ICZ_REQUIRE(A >= 1 && A <= BEAM_CONS_MAX_A, "%s: A=%d outside 1..%d", who, A, BEAM_CONS_MAX_A);
    ICZ_REQUIRE(n_img >= 1 && (long)n_img * (beam << C) <= (1 << 20), "%s: n_img=%d", who, n_img);
    ICZ_REQUIRE(step >= 1 && step <= 256 && L > step, "%s: step=%d outside 1..256 or not below L=%d", who, step, L);
    ICZ_REQUIRE(ngram == 0 || (ngram >= 2 && ngram <= 4), "%s: ngram=%d not 0, 2, 3 or 4", who, ngram);
    ICZ_REQUIRE(compact == 0 || (compact == 1 && step == 1), "%s: compact=%d at step %d (0, or 1 at step 1)", who, compact, step);
    ICZ_REQUIRE(V >= 1 && ldl >= V && ((long)V << C) * beam < 0x7fffffff, "%s: V=%d, ldl=%d", who, V, ldl);
    ICZ_REQUIRE(route >= BEAM_ROUTE_AUTO && route <= BEAM_ROUTE_SWEEP, "%s: route=%d", who, route);
    ICZ_REQUIRE(beam_rowtopk_route_fits(route, V, ldl, ((uintptr_t)logits & 15) == 0), "%s: route %d cannot take V=%d, ldl=%d, base %s", who, route,
                V, ldl, ((uintptr_t)logits & 15) == 0 ? "aligned" : "not 16-byte aligned");
    return ICZ_OK;
}

int icz_test_beam_rowtopk_constrained(int32_t route, const float* logits, int32_t n_img, int32_t beam, int32_t C, int32_t A, const int32_t* words,
                                      int32_t V, int32_t ldl, int32_t step, const int32_t* n_act, const int32_t* cap, const float* run,
                                      int32_t compact, const int32_t* seqs_in, int32_t L, int32_t ngram, float* cand_val, int32_t* cand_idx,
                                      float* force_val, void* stream) {
    const char* who = "icz_test_beam_rowtopk_constrained";
    ICZ_REQUIRE(logits && n_act && cap && run && cand_val && cand_idx && force_val && (words || C == 0) && (seqs_in || !ngram), "%s: null argument",
                who);
    ICZ_TRY(beam_test_states_shape(who, route, logits, n_img, beam, C, A, V, ldl, step, L, compact, ngram));
    const BeamCons cn = {words, C, A, beam, const_cast<int*>(cap), force_val, nullptr};
    launch_beam_rowtopk_cons((hipStream_t)stream, n_img * (beam << C), logits, V, ldl, beam << C, step, n_act, run, cand_val, cand_idx, compact,
                             seqs_in, L, ngram, route, cn);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_beam_constrained_step(int32_t route, const icz_beam_constrained_state* s, int32_t n_img, int32_t beam, int32_t C, int32_t A, int32_t V,
                                   int32_t ldl, int32_t step, int32_t L, int32_t compact, int32_t ngram, void* stream) {
    const char* who = "icz_test_beam_constrained_step";
    ICZ_REQUIRE(s, "%s: null state", who);
    ICZ_REQUIRE(s->logits && s->n_act && s->cap && s->run && s->seqs_in && s->seqs_out && s->src_row && s->it_next && s->n_live && s->hyp_seq &&
                    s->hyp_score && s->hyp_len && s->hyp_state && s->hyp_cnt && s->cand_val && s->cand_idx && s->force_val && (s->words || C == 0),
                "%s: null argument", who);
    ICZ_REQUIRE(s->seqs_in != s->seqs_out, "%s: seqs_in and seqs_out are the same buffer", who);
    ICZ_TRY(beam_test_states_shape(who, route, s->logits, n_img, beam, C, A, V, ldl, step, L, compact, ngram));
    hipStream_t st = (hipStream_t)stream;
    const int k = beam << C;
    BeamArgs a = {s->logits, V, ldl, k, step, L, s->n_act, s->run, s->seqs_in, s->seqs_out, s->src_row, s->it_next, nullptr, nullptr,
                  nullptr, nullptr, s->n_live, s->hyp_seq, s->hyp_score, s->hyp_len, s->hyp_cnt};
    const BeamCons cn = {s->words, C, A, beam, s->cap, s->force_val, s->hyp_state};
    launch_beam_rowtopk_cons(st, n_img * k, a.logits, V, ldl, k, step, (const int*)s->n_act, (const float*)s->run, s->cand_val, s->cand_idx, compact,
                             s->seqs_in, L, ngram, route, cn);
    hipLaunchKernelGGL(beam_merge_states_kernel, dim3(n_img), dim3(64), 0, st, a, cn, (const float*)s->cand_val, (const int*)s->cand_idx);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_beam_finalize_states(int32_t n_img, int32_t beam, int32_t C, int32_t L, int32_t steps_done, int32_t n_best, int32_t lp_kind,
                                  float lp_alpha, const int32_t* n_act, const float* run, const int32_t* seqs, const int32_t* hyp_cnt,
                                  const float* hyp_score, const int32_t* hyp_len, const int32_t* hyp_state, const int32_t* hyp_seq, float* out,
                                  int32_t* lens, float* scores, int32_t* sat, void* stream) {
    const char* who = "icz_test_beam_finalize_states";
    ICZ_REQUIRE(beam >= 1 && beam <= BEAM_MAX_K, "%s: beam=%d outside 1..%d", who, beam, BEAM_MAX_K);
    ICZ_REQUIRE(C >= 0 && C <= BEAM_CONS_MAX_C && (beam << C) <= BEAM_CONS_MAX_ROWS, "%s: C=%d outside 0..%d or 2^C * beam above %d", who, C,
                BEAM_CONS_MAX_C, BEAM_CONS_MAX_ROWS);
    ICZ_REQUIRE(n_img >= 1 && (long)n_img * (beam << C) <= (1 << 20), "%s: n_img=%d", who, n_img);
    ICZ_REQUIRE(steps_done >= 1 && steps_done <= 256 && L > steps_done, "%s: steps_done=%d outside 1..256 or not below L=%d", who, steps_done, L);
    const icz_beam_opts o = {n_best, 0, lp_kind, lp_alpha};
    ICZ_TRY(BeamBuf::check_opts(who, beam, &o));
    ICZ_REQUIRE(n_act && run && seqs && hyp_cnt && hyp_score && hyp_len && hyp_state && hyp_seq && out && lens && scores && sat, "%s: null argument",
                who);
    hipLaunchKernelGGL(beam_finalize_states_kernel, dim3(n_img), dim3(64), 0, (hipStream_t)stream, beam << C, beam, 1 << C, L, steps_done, n_best,
                       lp_kind, lp_alpha, n_act, run, seqs, hyp_cnt, hyp_score, hyp_len, hyp_state, hyp_seq, out, lens, scores, sat);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
