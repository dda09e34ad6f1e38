// What the kernel-alone test entries of the AoA family share (icz_test_aoa_*, include/icz.h): the dropout argument, the per-image region
// counts, the shape checks.  Included by the files that define entries, nowhere else.
#pragma once
#include "aoa_impl.h"

namespace icz {

static inline bool aoa_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int aoa_test_dropp(const char* who, const icz_test_dropp* t, DropP* out) {
    if (!t) { *out = aoa_dropp(0, nullptr, nullptr, 0, 0, 0.f); return ICZ_OK; }
    ICZ_REQUIRE(t->mode >= 0 && t->mode <= 2, "%s: dropout mode %d (0 off, 1 keep-mask, 2 Philox)", who, t->mode);
    ICZ_REQUIRE(t->mode == 0 || (t->p >= 0.f && t->p < 1.f), "%s: dropout probability %g outside [0, 1)", who, (double)t->p);
    ICZ_REQUIRE(t->mode != 1 || t->mask, "%s: dropout mode 1 without a keep-mask", who);
    ICZ_REQUIRE(t->mode != 2 || t->seed, "%s: dropout mode 2 without a device seed", who);
    *out = aoa_dropp(t->mode, t->mask, t->seed, t->stream, (int)t->step, t->mode ? t->p : 0.f, t->idx0);
    return ICZ_OK;
}
// Device counts [n_img] (null: every image has R regions) -> RegionRows: off / rowmap built by aoa_offsets_kernel as Aoa::refine builds them.
// The counts are read back and checked (1..R) first; the scratch lives until the entry returns (the destructor waits for the stream).
struct AoaTestRegions {
    int32_t* buf = nullptr;
    std::vector<int32_t> host;
    hipStream_t st = nullptr;
    ~AoaTestRegions() { if (buf) { (void)hipStreamSynchronize(st); (void)hipFree(buf); } }
    int build(const char* who, const int32_t* counts, int n_img, int R, hipStream_t stream, RegionRows* rr) {
        st = stream;
        if (!counts) { *rr = RegionRows{nullptr, nullptr, nullptr, R}; return ICZ_OK; }
        host.resize(n_img);
        ICZ_CHECK_HIP(hipMemcpy(host.data(), counts, sizeof(int32_t) * n_img, hipMemcpyDeviceToHost));
        for (int i = 0; i < n_img; ++i) {
            ICZ_REQUIRE(host[i] >= 1 && host[i] <= R, "%s: image %d has %d regions (1..%d)", who, i, host[i], R);
        }
        ICZ_CHECK_HIP(hipMalloc((void**)&buf, sizeof(int32_t) * ((size_t)n_img + 1 + (size_t)n_img * R)));
        hipLaunchKernelGGL(aoa_offsets_kernel, dim3(1), dim3(256), 0, st, counts, n_img, R, buf, buf + n_img + 1);
        *rr = RegionRows{buf, buf + n_img + 1, counts, R};
        return ICZ_OK;
    }
};
// device int32 values read back for a host check (img_of_row)
static inline int aoa_test_read_i32(const int32_t* dev, int n, std::vector<int32_t>* out) {
    out->resize(n);
    ICZ_CHECK_HIP(hipMemcpy(out->data(), dev, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return ICZ_OK;
}

static inline int aoa_test_heads(const char* who, int R, int Hd, int NH) {
    ICZ_REQUIRE(R >= 1 && R <= 128, "%s: %d regions per image (1..128)", who, R);
    ICZ_REQUIRE(NH >= 1 && Hd >= 4 && Hd % NH == 0 && (Hd / NH) % 4 == 0, "%s: hidden size %d must split into %d heads of a multiple of 4 columns", who, Hd, NH);
    return ICZ_OK;
}

}  // namespace icz
