// The 32-sample tile code of the decoders that keep whole activation planes (mlp_deep.hip, mlp_h128.hip; nothing else includes this): the MFMA product
// of a staged weight image with register fragments, the accumulator <-> fragment conversions, and the "native" plane layout those decoders save their
// activations and dz in.  The transposed-MFMA scheme itself is described at the top of mlp.hip.
//
// Native layout of a [samples x width] bf16 plane: per 32-sample tile and 32-column block, the 8-byte chunk (g, lane), g = 0 .. 3, holds columns
// 32 blk + 8 g + 4 (lane >> 5) + 0..3 of sample (lane & 31) - exactly registers 4g .. 4g+3 of the accumulator block, so stores and the backward's loads
// are whole 512-B wave transactions.  A tile's blocks follow each other (chunk index ((tile * nblk + blk) * 4 + g) * 64 + lane), a plane's tiles follow
// each other.  store_native writes it, mask_frags and stage_transposed read it, and ops._native_plane undoes it on the host.
#pragma once
#include "mlp_common.h"

namespace {

// acc[blk] += W[32 blk .. 32 blk + 31][16 s ..] . b[s]: A fragments from the staged image (row stride `stride`), B fragments from registers
// FENCE: the scheduler keeps each k step's loads with its MFMAs (a 7-block output layer: all 56 fragments ahead of their use do not fit the registers)
template <int NB, int KS, bool FENCE = false>
__device__ __forceinline__ void mm(f32x16 (&acc)[NB], const bf16x8 *b, const bf16_t *w, int stride, int lane) {
    const bf16_t *base = w + (lane & 31) * stride + 8 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
            const bf16x8 a = *reinterpret_cast<const bf16x8 *>(base + blk * 32 * stride + 16 * s);
            acc[blk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[s], acc[blk], 0, 0, 0);
        }
        if (FENCE) __builtin_amdgcn_sched_barrier(0);
    }
}

template <int NB>
__device__ __forceinline__ void init_bias(f32x16 (&acc)[NB], const float *bias, int h) {
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[blk][q] = bias[32 * blk + rho(q, h)];
}

template <int NB>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[NB]) {
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[blk][q] = 0.0f;
}

// accumulator blocks -> the next product's B fragments (2 per block), optionally through ReLU
template <int NB>
__device__ __forceinline__ void pack_frags(const f32x16 (&acc)[NB], bf16x8 *out, bool relu) {
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = acc[blk][8 * s + j];
                out[2 * blk + s][j] = (bf16_t)(relu ? fmaxf(v, 0.0f) : v);
            }
}

// backward: dz = acc where the saved activation is positive (native plane), rounded to bf16
template <int NB>
__device__ __forceinline__ void mask_frags(const f32x16 (&acc)[NB], const bf16_t *plane, int64_t tile, int lane, bf16x8 *out) {
    const bf16x4 *p = reinterpret_cast<const bf16x4 *>(plane) + tile * (NB * 256) + lane;
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bf16x4 a = p[(blk * 4 + g) * 64];
#pragma unroll
            for (int i = 0; i < 4; ++i) out[2 * blk + (g >> 1)][4 * (g & 1) + i] = (bf16_t)((float)a[i] > 0.0f ? acc[blk][4 * g + i] : 0.0f);
        }
}

template <int NB>
__device__ __forceinline__ void store_native(bf16_t *plane, int64_t tile, int lane, const bf16x8 *f) {
    bf16x4 *p = reinterpret_cast<bf16x4 *>(plane) + tile * (NB * 256) + lane;
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bf16x8 v = f[2 * blk + (g >> 1)];
            bf16x4 c;
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = v[4 * (g & 1) + i];
            p[(blk * 4 + g) * 64] = c;
        }
}

__device__ __forceinline__ bf16x4 zero4() {
    bf16x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (bf16_t)0.0f;
    return r;
}

// The weight-gradient kernels' operands: dst[(column) * WT + sample] from `nblk_take` column blocks (first: blk0) of a native plane with nblk_plane
// blocks, for the two tiles 2 pair, 2 pair + 1 (zeros past ntile).  WG: threads of the workgroup, all of which take part
template <int WG>
__device__ __forceinline__ void stage_transposed(bf16_t *dst, const bf16_t *plane, int nblk_plane, int blk0, int nblk_take, int64_t pair, int64_t ntile) {
    const int n = nblk_take * 256;
    for (int idx = threadIdx.x; idx < 2 * n; idx += WG) {
        const int sub = idx >= n, c = idx - sub * n;
        const int64_t t = 2 * pair + sub;
        bf16x4 v = zero4();
        if (t < ntile) v = reinterpret_cast<const bf16x4 *>(plane)[(t * nblk_plane + blk0) * 256 + c];
        const int ln = c & 63, g = (c >> 6) & 3, blk = c >> 8;
        bf16_t *d = dst + (32 * blk + 8 * g + 4 * (ln >> 5)) * WT + sub * 32 + (ln & 31);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i * WT] = v[i];
    }
}

}  // namespace
