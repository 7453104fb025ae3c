// Shared by the decoder translation units (mlp.hip with its headers mlp_params.h .. mlp_f32.h, mlp_wgrad.hip, mlp_affine.hip directly; mlp_deep.hip and mlp_h128.hip through mlp_native.h, which adds
// the tile code those two share; nothing else includes it): what more than one of them uses.
// The transposed-MFMA scheme of the decoders is described at the top of mlp.hip.
#pragma once
#include "common.h"
#include <algorithm>
#include <type_traits>

// What crosses translation units: a kernel is launched from the file that defines it (no relocatable device code), so the file that owns
// a kernel other files need exports a host launcher for it
namespace pagmlp {

constexpr int WG_MAX_BATCH = 6;         // layers per weight-gradient launch (grid.y)
constexpr int WG_SLAB_COLS = 96;        // floats per weight-gradient slab row: columns 0..63 dW, column 64 db
constexpr int NUM_CU = 256;             // MI355X: the persistent kernels launch at most one workgroup per CU and grid-stride over their batches
constexpr int WT = 72;                  // row stride (bf16) of the transposed [column][64 samples] weight-gradient images (mlp_native.h, mlp_h128_lds.h)

struct FinishParams {
    const float *slabs;
    int n_blocks, n_out, rows_pad, n_in, grp_L, grp_F;
    float *dW, *db;
};
struct FinishBatch {
    FinishParams p[WG_MAX_BATCH];
};
// mlp.hip: wgrad_finish_kernel over layers 0 .. n_layers - 1 of `fb`, max_out = their largest n_out
void launch_wgrad_finish(const FinishBatch &fb, int max_out, int n_layers, hipStream_t st);

}  // namespace pagmlp

namespace {
using namespace pagmlp;

typedef bf16_t bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16_t bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// a region of the dynamic LDS segment at a byte offset taken from the kernel's layout (mlp_lds.h)
template <typename T>
__device__ __forceinline__ T *lds_at(unsigned char *smem, int byte_offset) { return reinterpret_cast<T *>(smem) + byte_offset / (int)sizeof(T); }

__device__ __forceinline__ int rho(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }
// bits 2 and 3 exchanged: the input index of every weight image that is multiplied with register fragments (rho's row order against the hardware's k order)
__host__ __device__ __forceinline__ int swap23(int a) { return (a & ~12) | ((a & 4) << 1) | ((a & 8) >> 1); }
// staged position (8*g + e) of the XCD8 layout -> column level*F + f of the [M, L*F] feature row, or -1 (padding)
// (a / d for the wave-uniform divisors of the staging loops: a shift when d is a power of two - the feature width and the pad sizes always
// are - instead of the ~40-instruction software division; the loops below were bound by those: 25 k of a launch's clocks per workgroup)
__device__ __forceinline__ int udiv_uniform(int a, int d) { return (d & (d - 1)) == 0 ? a >> (31 - __clz(d)) : a / d; }
__device__ __forceinline__ int grp_col(int pos, int L, int F) {
    const int g = pos >> 3, e = pos & 7;
    const int j = udiv_uniform(e, F), f = e - j * F;
    const int level = xcd8_level(g, j);
    return (j < (L + 7) / 8 && level < L) ? level * F + f : -1;
}
__device__ __forceinline__ bf16x8 load8(const float *p) {
    f32x4 a = *reinterpret_cast<const f32x4 *>(p);
    f32x4 b = *reinterpret_cast<const f32x4 *>(p + 4);
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r[j] = (bf16_t)a[j];
        r[j + 4] = (bf16_t)b[j];
    }
    return r;
}
__device__ __forceinline__ bf16x8 load8(const bf16_t *p) { return *reinterpret_cast<const bf16x8 *>(p); }

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (bf16_t)0.0f;
    return r;
}

// Kernels that ask for more than 64 KiB of dynamic LDS opt in once per kernel and process (gfx950 has 160 KiB per workgroup)
template <auto Kernel>
void raise_lds_limit(int bytes) {
    static const hipError_t once = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    (void)once;
}

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

}  // namespace
