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
    const int rows = n_img * k, L = max_steps + 1, H = dims.H;
    ICZ_TRY(bm.ensure(mem, dims.max_rows, L));
    ICZ_TRY(prologue(feats, n_img, st));
    ICZ_TRY(zero_state(rows, 0, st));
    ICZ_TRY(bm.begin(n_img, k, L, it, st));
    // Step 1 (compact): the decoder runs ONE row per image (row img of the buffers); the top-k kernel reads image img's logits from
    // row img and the state gather fans row img out to the image's k rows.
    auto step = [&](int, bool compact) {
        StepIO s = {};
        s.rows = compact ? n_img : rows; s.feats = feats; s.img_of_row = compact ? nullptr : bm.img_of_row; s.it = it;
        s.rows_per_img = compact ? 1 : k;
        s.h1_in = h1[0]; s.c1_in = c1[0]; s.h2_in = h2[0]; s.c2_in = c2[0];
        s.h1_out = h1[1]; s.c1_out = c1[1]; s.h2_out = h2[1]; s.c2_out = c2[1];
        return this->step(s, st);
    };
    auto gather = [&](bool compact) {
        hipLaunchKernelGGL(beam_gather_kernel, dim3(cdiv(H, 1024), rows), dim3(256), 0, st, bm.src_row, H, h1[1], c1[1], h2[1], c2[1],
                           h1[0], c1[0], h2[0], c2[0], compact ? k : 1);
    };
    return bm.search(n_img, k, max_steps, true, logits, dims.V, pad_vocab(dims.V), it, seqs_out, lens_out, o, d, scores_out, st, step, gather);
}

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
