// Batched beam search (DecoderRNN.beam_search_sample, Models/BUTD_Model.py:236-318) for many images at once.
// The reference decodes one image per call with a Python list comprehension over tensor elements every step
// (k host syncs per step, :282-283).  Here every image owns k consecutive decoder rows; after the shared decoder
// step a per-image workgroup does log-softmax + running score + top-k over (active beams x V), retires beams that
// emitted <end> (k shrinks exactly as in the reference; no length normalisation unless icz_beam_opts asks for it), and emits the row permutation
// that re-gathers the LSTM state.  No host synchronisation inside a step.
#include "butd_impl.h"

namespace icz {

int Butd::beam_search(const float* feats, int n_img, int k, int max_steps, float* seqs_out, int32_t* lens_out, hipStream_t st,
                      const icz_beam_opts& o, float* scores_out, const icz_beam_diversity& d) {
    ICZ_REQUIRE(feats && seqs_out && lens_out, "butd beam: null argument");
    ICZ_TRY(BeamBuf::check("butd", n_img, k, max_steps, dims.max_rows));
    const int rows = n_img * k, L = max_steps + 1;
    ICZ_TRY(bm.ensure(mem, dims.max_rows, L));
    ICZ_TRY(prologue(feats, n_img, k, nullptr, st));
    ICZ_TRY(bm.begin(n_img, k, L, it, st));
    // Step 1 (compact): the decoder runs ONE row per image (row img of the buffers); the top-k kernel reads image img's logits from
    // row img and the state gather fans row img out to the image's k rows.
    auto step = [&](int, bool compact) {
        return compact ? this->step(n_img, it, nullptr, 1, 0, false, nullptr, st) : this->step(rows, it, bm.img_of_row, k, 0, false, nullptr, st);
    };
    auto gather = [&](bool compact) { this->gather(bm.src_row, rows, compact ? k : 1, st); };
    return bm.search(n_img, k, max_steps, true, logits, dims.V, pad_vocab(dims.V), it, seqs_out, lens_out, o, d, scores_out, st, step, gather);
}

// ---- decoder seams (DecodeMember) ------------------------------------------------------------------------------------------------
// the per-image prologue, then k zeroed state rows per image
int Butd::prologue(const float* feats, int n_img, int k, const int32_t*, hipStream_t st) {
    ICZ_TRY(prologue(feats, n_img, st));
    seam_feats = feats;
    return zero_state(n_img * k, 0, st);
}

int Butd::step(int rows, const int64_t* it_, const int32_t* img_of_row, int rows_per_img, int cur, bool slabs, LogitsView* out,
               hipStream_t st) {
    StepIO s = {};
    s.rows = rows; s.feats = seam_feats; s.img_of_row = img_of_row; s.it = it_;
    s.rows_per_img = rows_per_img;
    s.emb_ready = seam_emb_ready; s.live = seam_live;
    s.h1_in = h1[cur]; s.c1_in = c1[cur]; s.h2_in = h2[cur]; s.c2_in = c2[cur];
    s.h1_out = h1[cur ^ 1]; s.c1_out = c1[cur ^ 1]; s.h2_out = h2[cur ^ 1]; s.c2_out = c2[cur ^ 1];
    int pns = 1;
    if (slabs) s.pred_nsplit = &pns;
    ICZ_TRY(step(s, st));
    const int Vp = pad_vocab(dims.V);
    if (out) *out = pns > 1 ? LogitsView{ws, P.predict_b, (size_t)rows * Vp, Vp, pns} : LogitsView{logits, nullptr, 0, Vp, 1};
    return ICZ_OK;
}

void Butd::gather(const int32_t* src_row, int rows, int fan, hipStream_t st) {
    hipLaunchKernelGGL(beam_gather_kernel, dim3(cdiv(dims.H, 1024), rows), dim3(256), 0, st, src_row, dims.H, h1[1], c1[1], h2[1], c2[1],
                       h1[0], c1[0], h2[0], c2[0], fan);
}

DecodeMember* butd_member(void* handle) { return static_cast<DecodeMember*>(reinterpret_cast<Butd*>(handle)); }

}  // namespace icz

using namespace icz;
extern "C" int icz_butd_beam_search(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                                    float* seqs_out, int32_t* lens_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Butd*>(h)->beam_search(feats, n_img, beam, max_steps, seqs_out, lens_out, (hipStream_t)stream);
}
extern "C" int icz_butd_beam_search_opts(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps, const icz_beam_opts* opts,
                                         float* seqs_out, int32_t* lens_out, float* scores_out, void* stream) {
    ICZ_TRY(BeamBuf::check_opts("icz_butd_beam_search_opts", beam, opts));      // the arguments first: no handle needed to report them
    ICZ_REQUIRE(feats && seqs_out && lens_out && scores_out, "icz_butd_beam_search_opts: null argument");
    ICZ_REQUIRE(h, "icz_butd_beam_search_opts: null handle");
    return reinterpret_cast<Butd*>(h)->beam_search(feats, n_img, beam, max_steps, seqs_out, lens_out, (hipStream_t)stream, *opts, scores_out);
}
extern "C" int icz_butd_beam_search_diverse(icz_butd_t* h, const float* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                                            const icz_beam_opts* opts, const icz_beam_diversity* div, float* seqs_out, int32_t* lens_out, float* scores_out, void* stream) {
    ICZ_TRY(BeamBuf::check_opts("icz_butd_beam_search_diverse", beam, opts));      // the arguments first: no handle needed to report them
    ICZ_TRY(BeamBuf::check_diversity("icz_butd_beam_search_diverse", beam, div));
    ICZ_REQUIRE(feats && seqs_out && lens_out && scores_out, "icz_butd_beam_search_diverse: null argument");
    ICZ_REQUIRE(h, "icz_butd_beam_search_diverse: null handle");
    return reinterpret_cast<Butd*>(h)->beam_search(feats, n_img, beam, max_steps, seqs_out, lens_out, (hipStream_t)stream, *opts, scores_out, *div);
}
