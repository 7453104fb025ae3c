// The tile code that more than one decoder family of mlp.hip uses (mlp.hip and mlp_generic.h include this; nothing else does):
// weight staging, accumulator-block and tile I/O through the wave's staging buffer, the rank-1 upstream gradient, the pinned MFMA chains, the
// swizzled tiles of the fused weight gradients and the buffer-descriptor pieces of the straight-line kernels.  A helper that ONE family uses
// stands with that family instead (mlp_generic.h; the narrow decoders' and the wide head's in mlp.hip).
// The transposed-MFMA scheme is described at the top of mlp.hip.
#pragma once
#include "mlp_common.h"
#include "mlp_lds.h"

namespace {

// Stage W [n_out x n_in] f32 row-major into LDS as bf16 [rows_pad][stride]; zero padding;
// optional bit-2/3 swap of the column index (see the scheme at the top of mlp.hip).
// Every decoder kernel starts with 3 - 8 of these matrices.  As a loop of one element per iteration (a predicated load, then its store) the
// prologue ran at one L2 round trip per element - 80 dependent round trips per thread, 23 - 27 k clocks = 10 us per launch whatever the batch
// (in-kernel clocks: profiles/README.md, round 3).  Here eight loads are issued back to back - unconditionally, from clamped addresses, so that no branch separates them -
// and the padding is applied to the values afterwards.
constexpr int STAGE_BATCH = 8;      // 16: slower (registers / code size)
__device__ void stage_weight(bf16_t *dst, int stride, int rows_pad, int cols_pad, const float *W, int n_out, int n_in,
                             bool permute, int grp_L = 0, int grp_F = 0) {
    const int total = rows_pad * cols_pad, step = (int)blockDim.x, last = n_out * n_in - 1;
    for (int e0 = threadIdx.x; e0 < total; e0 += STAGE_BATCH * step) {
        float v[STAGE_BATCH];
        int at[STAGE_BATCH];
#pragma unroll
        for (int k = 0; k < STAGE_BATCH; ++k) {
            const int e = e0 + k * step;
            const int o = udiv_uniform(e, cols_pad), a = e - o * cols_pad;
            const int col = grp_L ? grp_col(a, grp_L, grp_F) : a;
            const bool ok = e < total && o < n_out && col >= 0 && col < n_in;
            at[k] = e < total ? o * stride + (permute ? swap23(a) : a) : -1;
            v[k] = W[min(max(o * n_in + col, 0), last)];
            v[k] = ok ? v[k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < STAGE_BATCH; ++k)
            if (at[k] >= 0) dst[at[k]] = (bf16_t)v[k];
    }
}
// Stage W^T: dst[row = input a][col = output o (permuted)]
__device__ void stage_weight_t(bf16_t *dst, int stride, int rows_pad, int cols_pad, const float *W, int n_out, int n_in,
                               int grp_L = 0, int grp_F = 0) {
    const int total = rows_pad * cols_pad, step = (int)blockDim.x, last = n_out * n_in - 1;
    for (int e0 = threadIdx.x; e0 < total; e0 += STAGE_BATCH * step) {
        float v[STAGE_BATCH];
        int at[STAGE_BATCH];
#pragma unroll
        for (int k = 0; k < STAGE_BATCH; ++k) {
            const int e = e0 + k * step;
            const int o = udiv_uniform(e, rows_pad), a = e - o * rows_pad;      // W's own row-major order (input index fastest): whole cache lines per
                                                                                // wave load, the transposition happens in the 2-byte LDS stores
            const int col = grp_L ? grp_col(a, grp_L, grp_F) : a;
            const bool ok = e < total && o < n_out && col >= 0 && col < n_in;
            at[k] = e < total ? a * stride + swap23(o) : -1;
            v[k] = W[min(max(o * n_in + col, 0), last)];
            v[k] = ok ? v[k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < STAGE_BATCH; ++k)
            if (at[k] >= 0) dst[at[k]] = (bf16_t)v[k];
    }
}

// Both images of one matrix from ONE pass over it: the natural image (as stage_weight: dst_s[o][a], optionally with the bit-2/3 swap) and the
// transposed one (as stage_weight_t: dst_t[a][o permuted]).  The backward kernels need W_0 (and W_1) both ways - recomputed forward and W^T chain.
__device__ void stage_weight_both(bf16_t *dst_s, int stride_s, bool permute_s, bf16_t *dst_t, int stride_t, int out_pad, int in_pad, const float *W,
                                  int n_out, int n_in, int grp_L = 0, int grp_F = 0) {
    const int total = out_pad * in_pad, step = (int)blockDim.x, last = n_out * n_in - 1;
    for (int e0 = threadIdx.x; e0 < total; e0 += STAGE_BATCH * step) {
        float v[STAGE_BATCH];
        int as[STAGE_BATCH], at[STAGE_BATCH];
#pragma unroll
        for (int k = 0; k < STAGE_BATCH; ++k) {
            const int e = e0 + k * step;
            const int o = udiv_uniform(e, in_pad), a = e - o * in_pad;
            const int col = grp_L ? grp_col(a, grp_L, grp_F) : a;
            const bool ok = e < total && o < n_out && col >= 0 && col < n_in;
            as[k] = e < total ? o * stride_s + (permute_s ? swap23(a) : a) : -1;
            at[k] = a * stride_t + swap23(o);
            v[k] = W[min(max(o * n_in + col, 0), last)];
            v[k] = ok ? v[k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < STAGE_BATCH; ++k)
            if (as[k] >= 0) {
                dst_s[as[k]] = (bf16_t)v[k];
                dst_t[at[k]] = (bf16_t)v[k];
            }
    }
}

// accumulator block -> two B fragments (k-steps 2*blk, 2*blk+1)
__device__ __forceinline__ void pack_block(const f32x16 &acc, bf16x8 &lo, bf16x8 &hi) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        lo[j] = (bf16_t)acc[j];
        hi[j] = (bf16_t)acc[8 + j];
    }
}

template <typename T>
__device__ __forceinline__ void store_block_full(T *row_ptr, int ch_base, int h, const f32x16 &acc);

// store one 32-row accumulator block of sample m as 4 groups of 4 consecutive channels
template <typename T>
__device__ __forceinline__ void store_block(T *row_ptr, int ch_base, int h, const f32x16 &acc, int n_valid, bool vec_ok) {
    if (vec_ok && ch_base + 32 <= n_valid) {
        store_block_full(row_ptr, ch_base, h, acc);
    } else if (vec_ok) {      // n_valid % 4 == 0: whole groups only
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = ch_base + 8 * g + 4 * h;
            if (c0 < n_valid) {
                if constexpr (sizeof(T) == 4) {
                    f32x4 v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                    *reinterpret_cast<f32x4 *>(row_ptr + c0) = v;
                } else {
                    bf16x4 v = {(bf16_t)acc[4 * g], (bf16_t)acc[4 * g + 1], (bf16_t)acc[4 * g + 2], (bf16_t)acc[4 * g + 3]};
                    *reinterpret_cast<bf16x4 *>(row_ptr + c0) = v;
                }
            }
        }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = ch_base + 8 * g + 4 * h;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j < n_valid) pag_st(row_ptr + c0 + j, acc[4 * g + j]);
        }
    }
}

// the four-channel group a block is stored as (and mlp_generic.h's load_block_raw loads)
template <typename T> struct RawVec { typedef f32x4 type; };
template <> struct RawVec<bf16_t> { typedef bf16x4 type; };

template <typename T>
__device__ __forceinline__ void store_block_full(T *row_ptr, int ch_base, int h, const f32x16 &acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        typename RawVec<T>::type v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (T)acc[4 * g + j];
        *reinterpret_cast<typename RawVec<T>::type *>(row_ptr + ch_base + 8 * g + 4 * h) = v;
    }
}

template <typename V>
__device__ __forceinline__ void raw_to_block(const V (&raw)[4], f32x16 &acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[4 * g + j] = (float)raw[g][j];
}

// ---------------------------------------------------------------------------------------- LDS staging
// In the accumulator layout every lane owns ONE sample row, so a direct global access touches 32 different rows per
// wave-instruction: rocprofv3 showed the texture-address unit busy 75-85 % of these kernels' time (TA_BUSY_avr vs
// GRBM_GUI_ACTIVE).  Row-major [M,64] bf16 tiles (32 rows = 4 KiB contiguous) and 32-column blocks of the wide
// [M,W] tensors therefore go through a wave-private LDS buffer: global side = fully coalesced 16-byte-per-lane
// accesses, register side = ds_read/ds_write_b64 in accumulator layout.

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// accumulator blocks acc[0..1] (64 columns) of a 32-row tile -> row-major [M,64] bf16 at gtile (= tensor + tile*32*64)
__device__ __forceinline__ void tile64_store(bf16_t *stg, bf16_t *gtile, int rows_valid, int lane, int r, int h, const f32x16 (&acc)[2]) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x4 v = {(bf16_t)acc[mb][4 * g], (bf16_t)acc[mb][4 * g + 1], (bf16_t)acc[mb][4 * g + 2], (bf16_t)acc[mb][4 * g + 3]};
            *reinterpret_cast<bf16x4 *>(stg + r * ST_RS + 32 * mb + 8 * g + 4 * h) = v;
        }
    wave_lds_sync();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), c = (lane & 7) * 8;
        bf16x8 v = *reinterpret_cast<const bf16x8 *>(stg + row * ST_RS + c);
        if (row < rows_valid) *reinterpret_cast<bf16x8 *>(gtile + row * HID + c) = v;
    }
    wave_lds_sync();
}

// tile64_load (mlp_generic.h) in two phases so that the global request of the NEXT tile can be in flight during the current tile's work
// (these kernels run 2 waves per SIMD: an exposed round trip per tile costs more than anything else in them)
__device__ __forceinline__ void tile64_fetch(const bf16_t *gtile, int rows_valid, int lane, bf16x8 (&v)[4]) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), c = (lane & 7) * 8;
        v[it] = zero8();
        if (row < rows_valid) v[it] = *reinterpret_cast<const bf16x8 *>(gtile + row * HID + c);
    }
}
__device__ __forceinline__ void tile64_unstage(bf16_t *stg, const bf16x8 (&v)[4], int lane, int r, int h, bf16x4 (&raw)[2][4]) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), c = (lane & 7) * 8;
        *reinterpret_cast<bf16x8 *>(stg + row * ST_RS + c) = v[it];
    }
    wave_lds_sync();
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int g = 0; g < 4; ++g) raw[mb][g] = *reinterpret_cast<const bf16x4 *>(stg + r * ST_RS + 32 * mb + 8 * g + 4 * h);
    wave_lds_sync();
}

// accumulator-layout pieces of the LDS columns [lcol, lcol+32) that block32_stage_in (mlp.hip) staged
__device__ __forceinline__ void block32_read(const bf16_t *stg, int lcol, int r, int h, bf16x4 (&raw)[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) raw[g] = *reinterpret_cast<const bf16x4 *>(stg + r * ST_RS + lcol + 8 * g + 4 * h);
}
// accumulator block -> columns [col0, col0+32) of the row-major [M,W] bf16 tensor
__device__ __forceinline__ void block32_store(bf16_t *stg, bf16_t *gtile, int W, int col0, int rows_valid, int lane, int r, int h, const f32x16 &acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        bf16x4 v = {(bf16_t)acc[4 * g], (bf16_t)acc[4 * g + 1], (bf16_t)acc[4 * g + 2], (bf16_t)acc[4 * g + 3]};
        *reinterpret_cast<bf16x4 *>(stg + r * ST_RS + 8 * g + 4 * h) = v;
    }
    wave_lds_sync();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int row = it * 16 + (lane >> 2), c = (lane & 3) * 8;
        bf16x8 v = *reinterpret_cast<const bf16x8 *>(stg + row * ST_RS + c);
        if (row < rows_valid && col0 + c < W) *reinterpret_cast<bf16x8 *>(gtile + (int64_t)row * W + col0 + c) = v;
    }
    wave_lds_sync();
}

// upstream gradient block in rank-1 form: z[q] = scale * g_row[32ob + rho(q,h)] (g_row = this sample's ray row, f32 [n])
__device__ __forceinline__ void rank1_block(const float *g_row, float scale, int ch_base, int h, int n_valid, f32x16 &z) {
    const bool vec = (n_valid & 3) == 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int c0 = ch_base + 8 * g + 4 * h;
        if (vec) {
            const bool ok = c0 < n_valid;
            f32x4 v = *reinterpret_cast<const f32x4 *>(g_row + (ok ? c0 : 0));
#pragma unroll
            for (int j = 0; j < 4; ++j) z[4 * g + j] = ok ? scale * v[j] : 0.0f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) z[4 * g + j] = (c0 + j < n_valid) ? scale * g_row[c0 + j] : 0.0f;
        }
    }
}

// A layer's MFMA chain for the one-wave-per-SIMD fused backward kernels, with the instruction order PINNED (hidden_layer in
// mlp_generic.h is the form that leaves the order to the scheduler).  Left to itself the scheduler emits
// "ds_read fragment, s_waitcnt lgkmcnt(0), v_mfma" once per k-step - a full LDS round trip in front of every MFMA, and a lone wave
// has nothing else to run meanwhile (20 such steps were half of a tile's time).  Here: every read of the first two k-steps first,
// then per k-step its two MFMAs (independent accumulators) while the reads two steps ahead are in flight.
template <int MBS, int NS, int LEAD_READS>
__device__ __forceinline__ void mfma_chain_pinned(const bf16_t *Wt, int stride, const bf16x8 (&frag)[NS], int r, int h, f32x16 (&acc)[2]) {
    bf16x8 a[MBS][NS];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int mb = 0; mb < MBS; ++mb) a[mb][s] = *reinterpret_cast<const bf16x8 *>(Wt + (32 * mb + r) * stride + 16 * s + 8 * h);
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int mb = 0; mb < MBS; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mb][s], frag[s], acc[mb], 0, 0, 0);
    constexpr int AHEAD = NS < 2 ? NS : 2;
    __builtin_amdgcn_sched_group_barrier(0x100, LEAD_READS + AHEAD * MBS, 0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        __builtin_amdgcn_sched_group_barrier(0x008, MBS, 0);
        if (s + AHEAD < NS) __builtin_amdgcn_sched_group_barrier(0x100, MBS, 0);
    }
}
template <int NS>
__device__ __forceinline__ void hidden_layer_pinned(const bf16_t *Ws, const float *bs, const bf16x8 (&frag)[NS], int r, int h, f32x16 (&acc)[2]) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[mb][q] = bs[32 * mb + rho(q, h)];
    mfma_chain_pinned<2, NS, 8>(Ws, RS, frag, r, h, acc);          // 8 leading reads: the bias blocks (4 x 16 bytes per block)
    __builtin_amdgcn_sched_barrier(0);
}

// ---------------------------------------------------------------------- swizzled tiles for the fused weight gradients
// dW = dz^T . a sums over the SAMPLES, which sit on the lanes in every register layout of the backward kernel - both MFMA
// operands need one transpose.  A wave keeps its 32-sample tiles ([32 samples][64 channels] bf16, 128-byte rows, 4 KiB) in LDS
// and reads operand fragments with ds_read_b64_tr_b16 (a 4-row x 16-column block per 16 lanes, delivered column-major).
// 8-byte chunk `c` of row `s` lives at chunk position c ^ tw_f(s): the accumulator-layout stores (lane = sample, 16 lanes =
// 16 rows, one chunk column) land in 16 different bank pairs, and the 4 rows of a transposed block use 4 different chunk
// groups, so neither access pattern has bank conflicts (the 32-lane ds_read_b64 of a whole column is 2-way).
typedef short i16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int tw_f(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ int tw_off(int row, int chunk) { return row * 64 + ((chunk ^ tw_f(row)) << 2); }
// (the writers stand with the kernels that use them, in mlp.hip: tw_put_frags, tw_put_block, relu_mask_pack_put, tw_put_rows)
// MFMA 32x32x16 operand fragment with k = sample: lane (c = lane & 31, h) gets samples 16ks + 8h .. +7 of channel 32 blk + c
__device__ __forceinline__ bf16x8 tw_frag(const bf16_t *T, int blk, int ks, int lane) {
    typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
    const int li = lane & 15, q = li >> 2, pp = li & 3, g1 = (lane >> 4) & 1, h = lane >> 5;
    const int chunk = 8 * blk + 4 * g1 + pp, row0 = 16 * ks + 8 * h + q;
    const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)(T + tw_off(row0, chunk)));
    const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)(T + tw_off(row0 + 4, chunk)));
    union { i16x4 v[2]; bf16x8 f; } u;
    u.v[0] = lo;
    u.v[1] = hi;
    return u.f;
}

// Buffer-descriptor accesses of the straight-line kernels (mlp.hip says how they use them, in front of mlp_fwd_fast):
// a lane that is out of range adds one of these to its offset - its loads return 0, its stores are dropped
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr unsigned BUF_OOB = 0x80000000u;         // added to an offset < 2^30: past any descriptor's range (tensors here are <= 2^30 bytes:
constexpr unsigned BUF_OOB_ROW = 0x40000000u;     // M <= 2^24 rows of <= 64 bytes).  Dead PIECE + dead ROW = 0xC0000000: the sum must not wrap to 0

__device__ __forceinline__ void out_block_pinned(const bf16_t *WLs, const float *bLs, int ob, const bf16x8 (&hb)[4], int r, int h, f32x16 &o) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 16; ++q) o[q] = bLs[32 * ob + rho(q, h)];
    bf16x8 a[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) a[s] = *reinterpret_cast<const bf16x8 *>(WLs + (32 * ob + r) * RS + 16 * s + 8 * h);
#pragma unroll
    for (int s = 0; s < 4; ++s) o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], hb[s], o, 0, 0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);          // 4 bias reads + 4 weight fragments, then the chain
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    __builtin_amdgcn_sched_barrier(0);
}
// relu + bf16 B fragments of the next layer
__device__ __forceinline__ void relu_pack(f32x16 (&acc)[2], bf16x8 (&hb)[4]) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[mb][q] = fmaxf(acc[mb][q], 0.0f);
        pack_block(acc[mb], hb[2 * mb], hb[2 * mb + 1]);
    }
}
// accumulator blocks (64 columns, 32 rows) -> row-major [M,64] bf16 through the wave's staging buffer; rows past M are dropped
template <typename RS_T>
__device__ __forceinline__ void tile64_store_buf(bf16_t *stg, RS_T rs, unsigned tile_off, int lane, int r, int h, const f32x16 (&acc)[2]) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x4 v = {(bf16_t)acc[mb][4 * g], (bf16_t)acc[mb][4 * g + 1], (bf16_t)acc[mb][4 * g + 2], (bf16_t)acc[mb][4 * g + 3]};
            *reinterpret_cast<bf16x4 *>(stg + r * ST_RS + 32 * mb + 8 * g + 4 * h) = v;
        }
    wave_lds_sync();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), c = (lane & 7) * 8;
        const u32x4 v = *reinterpret_cast<const u32x4 *>(stg + row * ST_RS + c);
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, tile_off + row * (HID * 2) + c * 2, 0, 0);
    }
    wave_lds_sync();
}

}  // namespace
