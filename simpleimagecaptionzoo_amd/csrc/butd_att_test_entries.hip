// Test entries of the kernels in butd_kernels.h, each on given operands (include/icz.h: icz_test_att_mean, icz_test_att_scores,
// icz_test_att_ctx, icz_test_att_saved_alphas, icz_test_att_bwd_dalpha, icz_test_att_bwd_ddec, icz_test_att_bwd_denc;
// tests/test_gpu_butd_att_kernels.py): the arguments are checked on the host, then the kernel goes through the launch helper of
// butd_impl.h that Butd::step and the BPTT go through -- the same template instance, grid rule and dynamic LDS size.
#include <vector>

#include "butd_impl.h"

namespace icz {

static inline bool at_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr int AT_MAX_ROWS = 65535;        // a grid dimension the kernels put rows / parts on stays far below its limit
constexpr int AT_MAX_SLABS = 32;          // the cap of gemm_pick_split
constexpr size_t AT_MAX_LDS = 60 * 1024;  // dynamic LDS of one workgroup (beside the kernels' static arrays)

// icz_test_drop -> DropCfg; every attention kernel reads four keep flags with one 4-byte load
static int at_drop(const char* who, const icz_test_drop* t, DropCfg* out) {
    *out = DropCfg{0, nullptr, nullptr, 0, 0, 0};
    if (!t) return ICZ_OK;
    ICZ_REQUIRE(t->mode >= 0 && t->mode <= 2, "%s: dropout mode %d (0 off, 1 keep flags, 2 Philox)", who, t->mode);
    ICZ_REQUIRE(t->mode != 1 || t->mask, "%s: dropout mode 1 without keep flags", who);
    ICZ_REQUIRE(t->mode != 1 || ((uintptr_t)t->mask & 3) == 0, "%s: dropout keep flags must be 4-byte aligned (four are read at once)", who);
    ICZ_REQUIRE(t->mode != 2 || t->seed, "%s: dropout mode 2 without a device seed", who);
    ICZ_REQUIRE(t->row0 >= 0, "%s: dropout row0=%d is negative", who, t->row0);
    *out = DropCfg{t->mode, t->mask, t->seed, t->stream, t->step, t->row0};
    return ICZ_OK;
}
// regions, images and the instance: <true> where counts are given or R > 64 (Butd::adaptive)
static int at_regions(const char* who, int n_img, int R, const int32_t* counts, bool* ad) {
    ICZ_REQUIRE(n_img >= 1 && n_img <= AT_MAX_ROWS, "%s: n_img=%d outside 1..%d", who, n_img, AT_MAX_ROWS);
    ICZ_REQUIRE(R >= 1 && R <= ATT_MAX_R, "%s: R=%d outside 1..%d", who, R, ATT_MAX_R);
    *ad = counts != nullptr || R > 64;
    return ICZ_OK;
}
static int at_width(const char* who, const char* name, int W) {
    ICZ_REQUIRE(W >= 4 && W % 4 == 0, "%s: %s=%d is not a positive multiple of 4", who, name, W);
    return ICZ_OK;
}
// device index arrays are read back and checked before the launch: counts [n_img] in 1..R, img_of_row [rows] in 0..n_img-1 (grouped
// kernels take row / G as the image: an img_of_row handed to them must say the same)
static int at_indices(const char* who, const int32_t* counts, int n_img, int R, const int32_t* img_of_row, int rows, int G, hipStream_t st) {
    if (!counts && !img_of_row) return ICZ_OK;
    ICZ_CHECK_HIP(hipStreamSynchronize(st));
    std::vector<int32_t> host;
    if (counts) {
        host.resize(n_img);
        ICZ_CHECK_HIP(hipMemcpy(host.data(), counts, sizeof(int32_t) * n_img, hipMemcpyDeviceToHost));
        for (int i = 0; i < n_img; ++i) ICZ_REQUIRE(host[i] >= 1 && host[i] <= R, "%s: image %d has %d regions (1..%d)", who, i, host[i], R);
    }
    if (img_of_row) {
        host.resize(rows);
        ICZ_CHECK_HIP(hipMemcpy(host.data(), img_of_row, sizeof(int32_t) * rows, hipMemcpyDeviceToHost));
        for (int r = 0; r < rows; ++r) {
            ICZ_REQUIRE(host[r] >= 0 && host[r] < n_img, "%s: img_of_row[%d]=%d outside 0..n_img-1 (n_img=%d)", who, r, host[r], n_img);
            ICZ_REQUIRE(G <= 0 || host[r] == r / G, "%s: img_of_row[%d]=%d, a grouped kernel takes row / G = %d", who, r, host[r], r / G);
        }
    }
    return ICZ_OK;
}
static int at_rows(const char* who, int rows, int n_img, bool identity) {
    ICZ_REQUIRE(rows >= 1 && rows <= AT_MAX_ROWS, "%s: rows=%d outside 1..%d", who, rows, AT_MAX_ROWS);
    ICZ_REQUIRE(!identity || rows <= n_img, "%s: %d rows over %d images without img_of_row", who, rows, n_img);
    return ICZ_OK;
}
static int at_group(const char* who, int rows, int G, int n_img) {
    ICZ_REQUIRE(G >= 1 && G <= ATT_CTX_MAX_G, "%s: G=%d outside 1..%d", who, G, ATT_CTX_MAX_G);
    ICZ_REQUIRE(rows % G == 0 && rows / G <= n_img, "%s: rows=%d are not G=%d rows of each of at most n_img=%d images", who, rows, G, n_img);
    return ICZ_OK;
}

}  // namespace icz

extern "C" {

int icz_test_att_mean(const float* feats, int32_t n_img, int32_t R, int32_t D, const int32_t* counts, float* mean, void* stream) {
    using namespace icz;
    const char* who = "icz_test_att_mean";
    ICZ_REQUIRE(feats && mean, "%s: null feats or mean", who);
    bool ad;
    ICZ_TRY(at_regions(who, n_img, R, counts, &ad));
    ICZ_TRY(at_width(who, "D", D));
    ICZ_REQUIRE(at_al16(feats) && at_al16(mean), "%s: feats and mean must be 16-byte aligned", who);
    hipStream_t const st = (hipStream_t)stream;
    ICZ_TRY(at_indices(who, counts, n_img, R, nullptr, 0, 0, st));
    launch_mean_feats(feats, mean, n_img, R, D, counts, st);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_att_scores(int32_t route, const icz_test_att_scores_args* s, const icz_test_drop* drop, int32_t G, int32_t parts, void* stream) {
    using namespace icz;
    const char* who = "icz_test_att_scores";
    ICZ_REQUIRE(s, "%s: null arguments", who);
    ICZ_REQUIRE(route >= 0 && route <= 2, "%s: route=%d (0 per row, 1 grouped, 2 grouped with dropout and early-out)", who, route);
    ICZ_REQUIRE(s->enc_ctx && s->dec_slab && s->b_dec && s->w_aff && s->b_aff && s->scores, "%s: null argument", who);
    bool ad;
    ICZ_TRY(at_regions(who, s->n_img, s->R, s->counts, &ad));
    ICZ_TRY(at_width(who, "A", s->A));
    ICZ_TRY(at_rows(who, s->rows, s->n_img, route == 0 && !s->img_of_row));
    ICZ_REQUIRE(s->nsplit >= 1 && s->nsplit <= AT_MAX_SLABS, "%s: nsplit=%d outside 1..%d", who, s->nsplit, AT_MAX_SLABS);
    ICZ_REQUIRE(parts >= 0 && parts <= AT_MAX_ROWS, "%s: parts=%d outside 0..%d (0: ATT_PARTS)", who, parts, AT_MAX_ROWS);
    ICZ_REQUIRE(at_al16(s->enc_ctx) && at_al16(s->dec_slab) && at_al16(s->b_dec) && at_al16(s->w_aff) && at_al16(s->dec_ctx_out),
                "%s: enc_ctx, dec_slab, b_dec, w_aff and dec_ctx_out must be 16-byte aligned", who);
    DropCfg dc;
    ICZ_TRY(at_drop(who, drop, &dc));
    if (route == 0) {
        ICZ_REQUIRE(G == 0 || G == 1, "%s: G=%d with the per-row kernel", who, G);
        ICZ_REQUIRE(sizeof(float) * s->A <= AT_MAX_LDS, "%s: A=%d does not fit the LDS row of dec_ctx", who, s->A);
    } else {
        ICZ_TRY(at_group(who, s->rows, G, s->n_img));
        ICZ_REQUIRE(att_scores_group_fits(s->rows, G, s->A), "%s: G=%d rows of A=%d floats exceed the grouped kernel's %zu bytes of LDS", who, G, s->A,
                    ATT_GROUP_LDS);
        ICZ_REQUIRE(route == 2 || (dc.mode == 0 && !s->live), "%s: the grouped evaluation kernel takes neither dropout nor live", who);
        ICZ_REQUIRE(dc.row0 == 0, "%s: dropout row0=%d (the grouped kernels have no evaluation-mode rows in front)", who, dc.row0);
    }
    hipStream_t const st = (hipStream_t)stream;
    ICZ_TRY(at_indices(who, s->counts, s->n_img, s->R, s->img_of_row, s->rows, route == 0 ? 0 : G, st));
    const AttScoreArgs a = {s->enc_ctx, s->img_of_row, s->dec_slab, s->nsplit, s->b_dec, s->w_aff, s->b_aff, s->dec_ctx_out, s->scores,
                            s->rows, s->R, s->A, s->live, s->counts};
    launch_att_scores((AttRoute)route, ad, a, dc, route == 0 ? 1 : G, parts ? parts : Butd::ATT_PARTS, st);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_att_ctx(const float* feats, int32_t n_img, const int32_t* img_of_row, const float* scores, float* alpha_out, float* alpha_out2,
                     int32_t alpha2_stride, float* ctx, int32_t rows, int32_t R, int32_t D, int32_t G, const int32_t* live, const int32_t* counts,
                     void* stream) {
    using namespace icz;
    const char* who = "icz_test_att_ctx";
    ICZ_REQUIRE(feats && scores && alpha_out && ctx, "%s: null argument", who);
    bool ad;
    ICZ_TRY(at_regions(who, n_img, R, counts, &ad));
    ICZ_TRY(at_width(who, "D", D));
    ICZ_TRY(at_rows(who, rows, n_img, G == 0 && !img_of_row));
    ICZ_REQUIRE(at_al16(feats) && at_al16(ctx), "%s: feats and ctx must be 16-byte aligned", who);
    ICZ_REQUIRE(G >= 0, "%s: G=%d (0: the per-row kernel)", who, G);
    if (G > 0) {
        ICZ_TRY(at_group(who, rows, G, n_img));
        ICZ_REQUIRE(!alpha_out2, "%s: the grouped kernel has no second alpha output", who);
    } else {
        ICZ_REQUIRE(!alpha_out2 || alpha2_stride >= R, "%s: alpha2_stride=%d below R=%d", who, alpha2_stride, R);
    }
    hipStream_t const st = (hipStream_t)stream;
    ICZ_TRY(at_indices(who, counts, n_img, R, img_of_row, rows, G, st));
    launch_att_ctx(ad, feats, img_of_row, scores, alpha_out, alpha_out2, alpha2_stride, ctx, rows, R, D, G, live, counts, st);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_att_saved_alphas(const float* src, int32_t T, int32_t B, int32_t NH, int32_t R, float* out, void* stream) {
    using namespace icz;
    const char* who = "icz_test_att_saved_alphas";
    ICZ_REQUIRE(src && out, "%s: null argument", who);
    ICZ_REQUIRE(T >= 1 && B >= 1 && NH >= 1 && R >= 1 && (long long)T * B * R * NH < (1LL << 31), "%s: T=%d, B=%d, NH=%d, R=%d", who, T, B, NH, R);
    launch_saved_alphas(src, T, B, NH, R, out, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_att_bwd_dalpha(const float* dctx, int32_t ns, int32_t ldc, int32_t rows, const float* feats, int32_t n_img, int32_t R, int32_t D,
                            float* dalpha_part, const int32_t* live, const int32_t* img_of_row, const int32_t* counts, void* stream) {
    using namespace icz;
    const char* who = "icz_test_att_bwd_dalpha";
    ICZ_REQUIRE(dctx && feats && dalpha_part, "%s: null argument", who);
    bool ad;
    ICZ_TRY(at_regions(who, n_img, R, counts, &ad));
    ICZ_TRY(at_width(who, "D", D));
    ICZ_TRY(at_rows(who, rows, n_img, !img_of_row));
    ICZ_REQUIRE(ns >= 1 && ns <= AT_MAX_SLABS, "%s: ns=%d outside 1..%d", who, ns, AT_MAX_SLABS);
    ICZ_REQUIRE(ldc >= D && ldc % 4 == 0, "%s: ldc=%d is below D=%d or no multiple of 4", who, ldc, D);
    ICZ_REQUIRE(at_al16(dctx) && at_al16(feats), "%s: dctx and feats must be 16-byte aligned", who);
    hipStream_t const st = (hipStream_t)stream;
    ICZ_TRY(at_indices(who, counts, n_img, R, img_of_row, rows, 0, st));
    launch_att_bwd_dalpha(ad, dctx, ns, ldc, rows, feats, R, D, dalpha_part, live, img_of_row, counts, st);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_att_bwd_ddec(const icz_test_att_ddec_args* s, const icz_test_drop* drop, void* stream) {
    using namespace icz;
    const char* who = "icz_test_att_bwd_ddec";
    ICZ_REQUIRE(s, "%s: null arguments", who);
    ICZ_REQUIRE(s->enc_ctx && s->dec_ctx && s->w_aff && s->alpha && s->dalpha && s->ddec && s->ds_out, "%s: null argument", who);
    bool ad;
    ICZ_TRY(at_regions(who, s->n_img, s->R, s->counts, &ad));
    ICZ_TRY(at_width(who, "A", s->A));
    ICZ_TRY(at_rows(who, s->rows, s->n_img, !s->img_of_row));
    ICZ_REQUIRE(s->nparts >= 1 && s->nparts <= AT_MAX_ROWS, "%s: nparts=%d outside 1..%d", who, s->nparts, AT_MAX_ROWS);
    ICZ_REQUIRE(at_al16(s->enc_ctx) && at_al16(s->dec_ctx) && at_al16(s->w_aff) && at_al16(s->ddec),
                "%s: enc_ctx, dec_ctx, w_aff and ddec must be 16-byte aligned", who);
    DropCfg dc;
    ICZ_TRY(at_drop(who, drop, &dc));
    ICZ_REQUIRE(dc.row0 == 0, "%s: dropout row0=%d (the backward runs over the sampled rows alone)", who, dc.row0);
    hipStream_t const st = (hipStream_t)stream;
    ICZ_TRY(at_indices(who, s->counts, s->n_img, s->R, s->img_of_row, s->rows, 0, st));
    const AttBwdDdecArgs a = {s->enc_ctx, s->dec_ctx, s->w_aff, s->alpha, s->dalpha, s->ddec, s->ds_out, s->R, s->A, s->nparts, s->live, s->img_of_row,
                              s->counts};
    launch_att_bwd_ddec(ad, a, dc, s->rows, st);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_att_bwd_denc(const icz_test_att_denc_args* s, int32_t G, int32_t parts, int32_t* parts_out, void* stream) {
    using namespace icz;
    const char* who = "icz_test_att_bwd_denc";
    ICZ_REQUIRE(s, "%s: null arguments", who);
    ICZ_REQUIRE(s->enc_ctx && s->dec_all && s->ds_all && s->w_aff && s->denc && s->dwaff_part, "%s: null argument", who);
    bool ad;
    ICZ_TRY(at_regions(who, s->n_img, s->R, s->counts, &ad));
    ICZ_TRY(at_width(who, "A", s->A));
    ICZ_TRY(at_rows(who, s->B, s->n_img, G == 0 && !s->img_of_row));
    ICZ_REQUIRE(s->T >= 1 && sizeof(float) * s->T * s->R <= AT_MAX_LDS, "%s: T=%d steps of R=%d regions (at least one, at most %zu bytes of LDS)", who, s->T,
                s->R, AT_MAX_LDS);
    ICZ_REQUIRE(s->Bs == 0 || s->Bs >= s->B, "%s: Bs=%d below B=%d (0: B)", who, s->Bs, s->B);
    ICZ_REQUIRE(s->mode >= 0 && s->mode <= 2, "%s: dropout mode %d (0 off, 1 keep flags, 2 Philox)", who, s->mode);
    ICZ_REQUIRE(s->mode != 1 || (s->mask && ((uintptr_t)s->mask & 3) == 0 && s->mask_step % 4 == 0 && s->mask_step >= (int64_t)s->B * s->R * s->A),
                "%s: dropout mode 1 needs 4-byte aligned keep flags, mask_step a multiple of 4 and at least B R A", who);
    ICZ_REQUIRE(s->mode != 2 || s->seed, "%s: dropout mode 2 without a device seed", who);
    ICZ_REQUIRE(at_al16(s->enc_ctx) && at_al16(s->dec_all) && at_al16(s->w_aff) && at_al16(s->denc) && at_al16(s->dwaff_part),
                "%s: enc_ctx, dec_all, w_aff, denc and dwaff_part must be 16-byte aligned", who);
    ICZ_REQUIRE(G >= 0 && parts >= 0 && parts <= AT_MAX_ROWS, "%s: G=%d, parts=%d (0: the per-row kernel; 0: the library's rule)", who, G, parts);
    int np = parts ? parts : Butd::ATT_PARTS;
    if (G > 0) {
        ICZ_REQUIRE(!s->img_of_row, "%s: the grouped kernel takes row / G as the image, not img_of_row", who);
        ICZ_REQUIRE(s->B % G == 0 && s->B / G <= s->n_img, "%s: B=%d rows are not G=%d rows of each of at most n_img=%d images", who, s->B, G, s->n_img);
        if (!parts) np = att_denc_group_parts(s->R, Butd::ATT_PARTS);
        ICZ_REQUIRE(np * DENC_GROUP_REGS >= s->R, "%s: %d parts of %d regions do not cover R=%d", who, np, DENC_GROUP_REGS, s->R);
    }
    hipStream_t const st = (hipStream_t)stream;
    ICZ_TRY(at_indices(who, s->counts, s->n_img, s->R, s->img_of_row, s->B, 0, st));
    if (parts_out) *parts_out = np;
    const AttBwdDencArgs a = {s->enc_ctx, s->dec_all, s->ds_all, s->w_aff, s->denc, s->dwaff_part, s->B, s->R, s->A, s->T,
                              s->mode, s->mask, (size_t)s->mask_step, s->seed, s->stream, s->Bs, s->img_of_row, s->counts};
    launch_att_bwd_denc(ad, a, G > 0 ? s->B / G : s->B, G, np, st);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
