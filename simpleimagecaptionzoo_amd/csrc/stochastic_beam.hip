// Stochastic beam search (beyond the reference; include/icz.h: icz_*_sample_distinct; Kool, van Hoof and Welling, "Stochastic Beams
// and Where to Find Them", ICML 2019): n distinct captions per image, a sample without replacement from the model's sequence
// distribution, on the decoder seams the beam search runs on (DecodeMember, decoder_core.h).  Every step: the members' decoder step,
// the ensemble's combine where there is one, sbs_rowtopk_kernel (Gumbel-perturbed row top-n), sbs_merge_kernel (conditioning on the
// parents' perturbed values, the image's n best) and the members' state gather.  The beam kernels and BeamBuf::search are not touched.
#include <cmath>

#include "sbs_kernels.h"

namespace icz {

int sample_distinct_check(const char* who, int n_img, int n, int max_len, float temperature, int V, int max_rows, int first_image) {
    ICZ_REQUIRE(n >= 1 && n <= SBS_MAX_N && (V < 0 || n <= V), "%s: n=%d hypotheses per image outside 1..%d or above the vocabulary (%d)", who, n,
                SBS_MAX_N, V);
    ICZ_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "%s: temperature %g not positive or not finite", who, (double)temperature);
    ICZ_REQUIRE(max_len >= 1 && max_len <= 256, "%s: max_len %d outside 1..256", who, max_len);
    ICZ_REQUIRE(max_rows < 0 || (n_img > 0 && (long)n_img * n <= max_rows), "%s: %d images x %d hypotheses exceed row capacity %d", who, n_img, n,
                max_rows);
    ICZ_REQUIRE(first_image >= 0 && (long)first_image + (n_img > 0 ? n_img : 0) <= SBS_MAX_IMAGES, "%s: first_image %d negative or first_image + n_img above %d", who,
                first_image, SBS_MAX_IMAGES);
    return ICZ_OK;
}

// sized once for the owner's row capacity and the longest search (256 steps: 2 x rows x 1 KiB of sequences), so no search re-allocates;
// the pinned read-back word is allocated with them
int SbsBuf::ensure(DeviceBuffers& m, int max_rows) {
    if (cap_rows >= max_rows) return ICZ_OK;
    const size_t R_ = max_rows, L_ = SBS_MAX_LEN;
    ICZ_TRY(m.alloc((void**)&occ, sizeof(int) * R_));
    ICZ_TRY(m.alloc((void**)&len, sizeof(int) * R_));
    ICZ_TRY(m.alloc((void**)&n_live, sizeof(int) * 260));
    ICZ_TRY(m.alloc((void**)&frozen, R_));
    ICZ_TRY(m.alloc((void**)&phi, sizeof(float) * R_));
    ICZ_TRY(m.alloc((void**)&G, sizeof(double) * R_));
    ICZ_TRY(m.alloc((void**)&seqs[0], sizeof(int32_t) * R_ * L_));
    ICZ_TRY(m.alloc((void**)&seqs[1], sizeof(int32_t) * R_ * L_));
    ICZ_TRY(m.alloc((void**)&src_row, sizeof(int32_t) * R_));
    ICZ_TRY(m.alloc((void**)&img_of_row, sizeof(int32_t) * R_));
    ICZ_TRY(m.alloc((void**)&it, sizeof(int64_t) * R_));
    ICZ_TRY(m.alloc((void**)&cand_g, sizeof(float) * R_ * SBS_MAX_N));
    ICZ_TRY(m.alloc((void**)&cand_phi, sizeof(float) * R_ * SBS_MAX_N));
    ICZ_TRY(m.alloc((void**)&cand_idx, sizeof(int) * R_ * SBS_MAX_N));
    if (!n_live_host) ICZ_CHECK_HIP(hipHostMalloc((void**)&n_live_host, sizeof(int) * 4, 0));
    ICZ_TRY(m.synced());
    cap_rows = (int)R_;
    return ICZ_OK;
}

static void launch_sbs_init(int n_img, int n, const float* root_uniforms, uint64_t seed, int img0, int* occ, uint8_t* frozen, float* phi, double* G, int* len,
                            int64_t* it, int32_t* img_of_row, int32_t* src_row, hipStream_t st) {
    hipLaunchKernelGGL(sbs_init_kernel, dim3(cdiv(n_img * n, 256)), dim3(256), 0, st, n_img, n, root_uniforms, seed, img0, occ, frozen, phi, G, len, it,
                       img_of_row, src_row);
}

static void launch_sbs_finalize(int n_img, int n, int L, const int* occ, const uint8_t* frozen, const float* phi, const double* G, const int* len,
                                const int32_t* seqs, const icz_sample_distinct_out* o, hipStream_t st) {
    hipLaunchKernelGGL(sbs_finalize_kernel, dim3(n_img), dim3(64), 0, st, n, L, occ, frozen, phi, G, len, seqs, o->ids, o->lens, o->finished, o->phi,
                       o->g);
}

// Every check runs before the first allocation or launch: a refused call queues nothing.  The start state precedes the prologues:
// NIC's (and so an ensemble's) reads img_of_row, which the init kernel writes.
int sample_distinct(const char* who, DecodeMember* const* m, int M, const BeamCombine* ens, const float* const* feats, int n_img, int n,
                    int max_len, float temperature, uint64_t seed, int first_image, const float* uniforms, const float* root_uniforms,
                    const icz_sample_distinct_out* out, hipStream_t st) {
    const int V = m[0]->vocab(), cap = ens ? ens->cap : m[0]->row_capacity();
    ICZ_TRY(sample_distinct_check(who, n_img, n, max_len, temperature, V, cap, first_image));
    if (ens) ICZ_TRY(check_members(who, m, M, feats, n_img * n));
    else ICZ_REQUIRE(m[0]->refreshed(), "%s: call icz_*_refresh_weights after binding/updating parameters", who);
    SbsBuf& b = ens ? *ens->sbs : m[0]->sbs;
    const int rows = n_img * n, L = max_len;
    ICZ_TRY(b.ensure(ens ? *ens->mem : m[0]->buffers(), cap));
    ICZ_CHECK_HIP(hipMemsetAsync(b.n_live, 0, sizeof(int) * 260, st));
    launch_sbs_init(n_img, n, root_uniforms, seed, first_image, b.occ, b.frozen, b.phi, b.G, b.len, b.it, b.img_of_row, b.src_row, st);
    for (int i = 0; i < M; ++i) ICZ_TRY(m[i]->prologue(feats[i], n_img, n, b.img_of_row, st));
    bool compact_first = true;
    for (int i = 0; i < M; ++i) compact_first = compact_first && m[i]->compact_step();
    LogitsView lv[ENS_MAX_M];
    int sb = 0;
    for (int s = 1; s <= max_len; ++s) {
        // Step 1 (compact): the decoder runs ONE row per image (row img of the buffers); the row kernel reads image img's logits from
        // row img and the state gather fans row img out to the image's n rows.
        const bool compact = compact_first && s == 1 && n > 1;
        const int r = compact ? n_img : rows;
        // the row kernel sums split-K slabs itself (LogitsView), as the sampling and scoring kernels do
        for (int i = 0; i < M; ++i) ICZ_TRY(m[i]->step(r, b.it, compact ? nullptr : b.img_of_row, compact ? 1 : n, 0, true, &lv[i], st));
        if (ens) ens->run(lv, r);
        SbsRowArgs ra = {};
        ra.lv = ens ? LogitsView{ens->lp, nullptr, 0, ens->ld, 1} : lv[0];
        ra.V = V; ra.n = n; ra.step = s; ra.compact = compact ? 1 : 0; ra.temperature = temperature;
        ra.occ = b.occ; ra.frozen = b.frozen; ra.phi = b.phi;
        ra.uniforms = uniforms ? uniforms + (size_t)(s - 1) * rows * V : nullptr;
        ra.seed = seed; ra.img0 = first_image;
        ra.cand_g = b.cand_g; ra.cand_phi = b.cand_phi; ra.cand_idx = b.cand_idx;
        hipLaunchKernelGGL(sbs_rowtopk_kernel, dim3(rows), dim3(256), 0, st, ra);
        const SbsMergeArgs ma = {V, n, s, L, b.occ, b.frozen, b.phi, b.G, b.len, b.seqs[sb], b.seqs[sb ^ 1], b.src_row, b.it, b.n_live + s,
                                 b.cand_g, b.cand_phi, b.cand_idx};
        hipLaunchKernelGGL(sbs_merge_kernel, dim3(n_img), dim3(64), 0, st, ma);
        for (int i = 0; i < M; ++i) m[i]->gather(b.src_row, rows, compact ? n : 1, st);
        sb ^= 1;
        if (s >= 6 && (s % 3) == 0 && s < max_len) {
            ICZ_CHECK_HIP(hipMemcpyAsync(b.n_live_host, b.n_live + s, sizeof(int), hipMemcpyDeviceToHost, st));
            ICZ_CHECK_HIP(hipStreamSynchronize(st));
            if (b.n_live_host[0] == 0) break;
        }
    }
    launch_sbs_finalize(n_img, n, L, b.occ, b.frozen, b.phi, b.G, b.len, b.seqs[sb], out, st);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// A family's icz_*_sample_distinct on its member m (null for a null handle): rules 1 - 5 here, the rest in sample_distinct
static int sample_distinct_entry(const char* who, DecodeMember* m, const float* feats, int n_img, int n, int max_len, float temperature,
                                 uint64_t seed, int first_image, const float* uniforms, const float* root_uniforms, const icz_sample_distinct_out* out, void* stream) {
    ICZ_TRY(sample_distinct_check(who, n_img, n, max_len, temperature, m ? m->vocab() : -1, -1, 0));
    ICZ_REQUIRE(feats && out && out->ids && out->lens && out->finished && out->phi && out->g && (uniforms == nullptr) == (root_uniforms == nullptr),
                "%s: null argument (uniforms and root_uniforms: both or neither)", who);
    ICZ_REQUIRE(m, "%s: null handle", who);
    return sample_distinct(who, &m, 1, nullptr, &feats, n_img, n, max_len, temperature, seed, first_image, uniforms, root_uniforms, out, (hipStream_t)stream);
}

}  // namespace icz

// ================================================================================================
using namespace icz;
extern "C" {

int icz_sample_distinct_check(int32_t n_img, int32_t n, int32_t max_len, float temperature, int32_t V, int32_t max_rows) {
    return sample_distinct_check("icz_sample_distinct_check", n_img, n, max_len, temperature, V, max_rows, 0);
}

int icz_butd_sample_distinct(icz_butd_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, float temperature, uint64_t seed,
                             int32_t first_image, const float* uniforms, const float* root_uniforms, const icz_sample_distinct_out* out, void* stream) {
    return sample_distinct_entry("icz_butd_sample_distinct", h ? butd_member(h) : nullptr, feats, n_img, n, max_len, temperature, seed, first_image,
                                 uniforms, root_uniforms, out, stream);
}
int icz_aoa_sample_distinct(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, float temperature, uint64_t seed,
                            int32_t first_image, const float* uniforms, const float* root_uniforms, const icz_sample_distinct_out* out, void* stream) {
    return sample_distinct_entry("icz_aoa_sample_distinct", h ? aoa_member(h) : nullptr, feats, n_img, n, max_len, temperature, seed, first_image,
                                 uniforms, root_uniforms, out, stream);
}
int icz_nic_sample_distinct(icz_nic_t* h, const float* features, int32_t n_img, int32_t n, int32_t max_len, float temperature, uint64_t seed,
                            int32_t first_image, const float* uniforms, const float* root_uniforms, const icz_sample_distinct_out* out, void* stream) {
    return sample_distinct_entry("icz_nic_sample_distinct", h ? nic_member(h) : nullptr, features, n_img, n, max_len, temperature, seed, first_image,
                                 uniforms, root_uniforms, out, stream);
}

// ------------------------------------------------------------------------------------------------
// Test entries of the kernels (include/icz.h): the arguments are checked on the host, then the kernels are launched with the grids of
// sample_distinct, nothing more.
static int sbs_test_shape(const char* who, const float* logits, const float* bias, int nsplit, int ld, int n_img, int n, int V, int step, int compact,
                          float temperature) {
    ICZ_REQUIRE(n >= 1 && n <= SBS_MAX_N, "%s: n=%d outside 1..%d", who, n, SBS_MAX_N);
    ICZ_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "%s: temperature %g not positive or not finite", who, (double)temperature);
    ICZ_REQUIRE(n_img >= 1 && (long)n_img * n <= (1 << 20), "%s: n_img=%d", who, n_img);
    ICZ_REQUIRE(step >= 1 && step <= 256, "%s: step=%d outside 1..256", who, step);
    ICZ_REQUIRE(compact == 0 || (compact == 1 && step == 1), "%s: compact=%d at step %d (0, or 1 at step 1)", who, compact, step);
    ICZ_REQUIRE(V >= 1 && ld >= V && (long)V * SBS_MAX_N < 0x7fffffff, "%s: V=%d, ld=%d", who, V, ld);
    ICZ_REQUIRE(logits && nsplit >= 1 && (nsplit == 1 || bias), "%s: null logits, nsplit < 1 or split-K slabs without a bias", who);
    return ICZ_OK;
}

static SbsRowArgs sbs_test_row_args(const float* logits, const float* bias, int nsplit, int ld, int n_img, int n, int V, int step, int compact,
                                    float temperature, const int* occ, const uint8_t* frozen, const float* phi, const float* uniforms, uint64_t seed,
                                    int img0, float* cand_g, float* cand_phi, int* cand_idx) {
    SbsRowArgs ra = {};
    const size_t R = compact ? n_img : (size_t)n_img * n;
    ra.lv = LogitsView{logits, nsplit > 1 ? bias : nullptr, R * ld, ld, nsplit};
    ra.V = V; ra.n = n; ra.step = step; ra.compact = compact; ra.temperature = temperature;
    ra.occ = occ; ra.frozen = frozen; ra.phi = phi; ra.uniforms = uniforms; ra.seed = seed; ra.img0 = img0;
    ra.cand_g = cand_g; ra.cand_phi = cand_phi; ra.cand_idx = cand_idx;
    return ra;
}

int icz_test_sbs_rowtopk(const float* logits, const float* bias, int32_t nsplit, int32_t ld, int32_t n_img, int32_t n, int32_t V, int32_t step,
                         int32_t compact, float temperature, const int32_t* occ, const uint8_t* frozen, const float* phi,
                         const float* uniforms, uint64_t seed, int32_t first_image, float* cand_g, float* cand_phi, int32_t* cand_idx, void* stream) {
    const char* who = "icz_test_sbs_rowtopk";
    ICZ_REQUIRE(occ && frozen && phi && cand_g && cand_phi && cand_idx, "%s: null argument", who);
    ICZ_TRY(sbs_test_shape(who, logits, bias, nsplit, ld, n_img, n, V, step, compact, temperature));
    const SbsRowArgs ra = sbs_test_row_args(logits, bias, nsplit, ld, n_img, n, V, step, compact, temperature, occ, frozen, phi, uniforms, seed,
                                            first_image, cand_g, cand_phi, cand_idx);
    hipLaunchKernelGGL(sbs_rowtopk_kernel, dim3(n_img * n), dim3(256), 0, (hipStream_t)stream, ra);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_sbs_step(const icz_sbs_step_state* s, int32_t nsplit, int32_t ld, int32_t n_img, int32_t n, int32_t V, int32_t step, int32_t L,
                      int32_t compact, float temperature, uint64_t seed, int32_t first_image, void* stream) {
    const char* who = "icz_test_sbs_step";
    ICZ_REQUIRE(s, "%s: null state", who);
    ICZ_REQUIRE(s->occ && s->frozen && s->phi && s->G && s->len && s->seqs_in && s->seqs_out && s->src_row && s->it_next && s->n_live && s->cand_g &&
                    s->cand_phi && s->cand_idx,
                "%s: null argument", who);
    ICZ_REQUIRE(s->seqs_in != s->seqs_out, "%s: seqs_in and seqs_out are the same buffer", who);
    ICZ_TRY(sbs_test_shape(who, s->logits, s->bias, nsplit, ld, n_img, n, V, step, compact, temperature));
    ICZ_REQUIRE(L >= step, "%s: step=%d above L=%d", who, step, L);
    hipStream_t st = (hipStream_t)stream;
    const SbsRowArgs ra = sbs_test_row_args(s->logits, s->bias, nsplit, ld, n_img, n, V, step, compact, temperature, s->occ, s->frozen, s->phi,
                                            s->uniforms, seed, first_image, s->cand_g, s->cand_phi, s->cand_idx);
    hipLaunchKernelGGL(sbs_rowtopk_kernel, dim3(n_img * n), dim3(256), 0, st, ra);
    const SbsMergeArgs ma = {V, n, step, L, s->occ, s->frozen, s->phi, s->G, s->len, s->seqs_in, s->seqs_out, s->src_row, s->it_next, s->n_live,
                             s->cand_g, s->cand_phi, s->cand_idx};
    hipLaunchKernelGGL(sbs_merge_kernel, dim3(n_img), dim3(64), 0, st, ma);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_sbs_init(int32_t n_img, int32_t n, const float* root_uniforms, uint64_t seed, int32_t first_image, int32_t* occ, uint8_t* frozen, float* phi, double* G,
                      int32_t* len, int64_t* it, int32_t* img_of_row, int32_t* src_row, void* stream) {
    const char* who = "icz_test_sbs_init";
    ICZ_REQUIRE(n >= 1 && n <= SBS_MAX_N && n_img >= 1 && (long)n_img * n <= (1 << 20), "%s: n=%d, n_img=%d", who, n, n_img);
    ICZ_REQUIRE(occ && frozen && phi && G && len && it && img_of_row && src_row, "%s: null argument", who);
    launch_sbs_init(n_img, n, root_uniforms, seed, first_image, occ, frozen, phi, G, len, it, img_of_row, src_row, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_sbs_finalize(int32_t n_img, int32_t n, int32_t L, const int32_t* occ, const uint8_t* frozen, const float* phi, const double* G,
                          const int32_t* len, const int32_t* seqs, const icz_sample_distinct_out* out, void* stream) {
    const char* who = "icz_test_sbs_finalize";
    ICZ_REQUIRE(n >= 1 && n <= SBS_MAX_N && n_img >= 1 && (long)n_img * n <= (1 << 20) && L >= 1, "%s: n=%d, n_img=%d, L=%d", who, n, n_img, L);
    ICZ_REQUIRE(occ && frozen && phi && G && len && seqs && out && out->ids && out->lens && out->finished && out->phi && out->g, "%s: null argument",
                who);
    launch_sbs_finalize(n_img, n, L, occ, frozen, phi, G, len, seqs, out, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
