// Shared helpers for the libicz HIP sources (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/icz.h"

namespace icz {

void set_error(const char* fmt, ...);

#define ICZ_CHECK_HIP(expr)                                                                    \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            icz::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return ICZ_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

#define ICZ_REQUIRE(cond, ...)                    \
    do {                                          \
        if (!(cond)) {                            \
            icz::set_error(__VA_ARGS__);          \
            return ICZ_ERR_INVALID;               \
        }                                         \
    } while (0)

#define ICZ_TRY(expr)                   \
    do {                                \
        int s_ = (expr);                \
        if (s_ != ICZ_OK) return s_;    \
    } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// event pairs around groups of small kernels (icz_kprof_begin / icz_kprof_end, include/icz.h); no-ops unless enabled, never inside a capture
enum { KP_ATTENTION = 0, KP_GREEDY_SELECT = 1, KP_SAMPLE_SELECT = 2, KP_LSTM_POINT = 3, KP_GROUPS = 4 };
void kprof_mark(int group, bool begin, hipStream_t st);
// padded vocabulary size (row stride of logits, rows of the materialised predict weight): a multiple of 64 so that
// V can be the K dimension of a GEMM on the fast (tail-free) path; pad entries are kept at zero
static inline int pad_vocab(int V) { return (V + 63) & ~63; }

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide helpers (256 threads)
__device__ __forceinline__ float block_max_256(float v, float* sm) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_sum_256(float v, float* sm) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    __syncthreads();
    return r;
}

// Softmax over the entries a wave holds, one per lane: x is the lane's entry, or -inf where the lane holds none (in = false), and
// the lane's weight comes back (0 without an entry).  The attention kernels of BUTD and of the AoA refiner share this expression.
__device__ __forceinline__ float wave_softmax(float x, bool in) {
    const float mx = wave_max(x);
    const float e = in ? expf(x - mx) : 0.f;
    const float sum = wave_sum(e);
    return e / sum;
}
// The same with two entries per lane (lane and lane + 64): with no second entry anywhere it is wave_softmax bit for bit, the
// second entry being the identity of both reductions.
__device__ __forceinline__ void wave_softmax2(float x0, bool in0, float x1, bool in1, float& p0, float& p1) {
    const float mx = wave_max(fmaxf(x0, x1));
    const float e0 = in0 ? expf(x0 - mx) : 0.f;
    const float e1 = in1 ? expf(x1 - mx) : 0.f;
    const float sum = wave_sum(e0 + e1);
    p0 = e0 / sum;
    p1 = e1 / sum;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// sum of ns split-K slabs at one element, loads issued four at a time (independent), added in slab order
__device__ __forceinline__ float sum_slabs1(const float* __restrict__ p, int ns, size_t stride, size_t off) {
    float s = 0.f;
    int z = 0;
    for (; z + 4 <= ns; z += 4) {
        const float a = p[(size_t)z * stride + off], b = p[(size_t)(z + 1) * stride + off];
        const float c = p[(size_t)(z + 2) * stride + off], d = p[(size_t)(z + 3) * stride + off];
        s += a; s += b; s += c; s += d;
    }
    for (; z < ns; ++z) s += p[(size_t)z * stride + off];
    return s;
}
// four consecutive elements (16-byte loads): slab 0, then slabs 1 .. ns - 1 added in slab order; no slabs (p null): zeros
__device__ __forceinline__ f32x4 sum_slabs4(const float* p, int ns, size_t slab_stride, size_t off) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (!p) return s;
    s = *reinterpret_cast<const f32x4*>(p + off);
    for (int z = 1; z < ns; ++z) s += *reinterpret_cast<const f32x4*>(p + (size_t)z * slab_stride + off);
    return s;
}

// Early-out of the rollout / BPTT steps behind the reference's break (`if unfinished.sum() == 0: break`, BUTD_Model.py:233,
// AoA_Model.py:400, NIC_Model.py:150): `live` points at the number of rows still unfinished after the PREVIOUS step of the
// sampled rollout (a device counter written by that step's sample_select_kernel); 0 = the reference never ran this step.  Every
// kernel of such a step returns at entry (producers of buffers that a later batched GEMM reads write zeros first); null = always
// live (greedy / beam / XE).  The address is a kernel argument: one scalar load, uniform branch.
__device__ __forceinline__ bool step_dead(const int* live) { return live != nullptr && *live == 0; }
// The same test in two parts for the hot kernels: live_flag() at the TOP of the kernel issues the scalar load, flag_dead() sits
// BEHIND the kernel's first batch of global loads and in front of its first write -- the flag's round trip passes while those
// loads are in flight, so a live step does not wait for it (tested at the top of every 5 - 9 us kernel it cost 0.3 us per launch:
// +1.2 % on the SCST step, same box, round 5), and a dead step leaves with loads outstanding.  The empty asm is a compiler
// barrier: the vector loads in front of it are not sunk below the branch.
__device__ __forceinline__ int live_flag(const int* live) { return live != nullptr ? *live : 1; }
__device__ __forceinline__ bool flag_dead(int flag) {
    asm volatile("" ::: "memory");
    return flag == 0;
}

}  // namespace icz
