// The generic decoder kernels of mlp.hip (only mlp.hip includes this): mlp_fwd_mfma and mlp_bwd_mfma serve every layout, dtype, activation and
// output width up to 224 through run-time branches - what runs when a shape has no kernel of its own in mlp.hip - each
// followed by its launcher.  The transposed-MFMA scheme is described at the top of mlp.hip.
//
// Dynamic LDS: a kernel takes its regions from its layout struct in mlp_lds.h (lds_at<T>(smem, L.region)) and its launcher passes the same
// struct's `bytes` - a region is added there, once.  mlp_fwd_mfma here and head_composite_fwd_kernel (mlp.hip) are the exceptions (mlp_lds.h
// says why): their carve-up is still a chain that has to be kept in step with FwdLds / HeadCompLds by hand.
#pragma once
#include "mlp_common.h"
#include "mlp_lds.h"
#include "mlp_params.h"
#include "mlp_tile.h"

namespace {

// load one 32-row block of sample m in two phases: issue every load of a block first (raw registers), convert later, so that
// the compiler can keep all of a tile's loads in flight instead of waiting on each one before its conversion
template <typename T>
__device__ __forceinline__ void load_block_raw(const T *row_ptr, int ch_base, int h, typename RawVec<T>::type (&raw)[4], int n_valid,
                                               bool vec_ok) {
    typedef typename RawVec<T>::type V;
    if (vec_ok && ch_base + 32 <= n_valid) {      // block wholly in range (all but the last block): plain vector loads
#pragma unroll
        for (int g = 0; g < 4; ++g) raw[g] = *reinterpret_cast<const V *>(row_ptr + ch_base + 8 * g + 4 * h);
    } else if (vec_ok) {      // n_valid % 4 == 0: a group is wholly in range or wholly out; branch-free (clamped address + select)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = ch_base + 8 * g + 4 * h;
            const bool ok = c0 < n_valid;
            V v = *reinterpret_cast<const V *>(row_ptr + (ok ? c0 : 0));
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ok ? v[j] : (T)0.0f;
            raw[g] = v;
        }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = ch_base + 8 * g + 4 * h;
            V v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (c0 + j < n_valid) ? row_ptr[c0 + j] : (T)0.0f;
            raw[g] = v;
        }
    }
}

// row-major [M,64] bf16 tile -> accumulator-layout raw pieces raw[mb][g]
__device__ __forceinline__ void tile64_load(bf16_t *stg, const bf16_t *gtile, int rows_valid, int lane, int r, int h, bf16x4 (&raw)[2][4]) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), c = (lane & 7) * 8;
        bf16x8 v = zero8();
        if (row < rows_valid) v = *reinterpret_cast<const bf16x8 *>(gtile + row * HID + c);
        *reinterpret_cast<bf16x8 *>(stg + row * ST_RS + c) = v;
    }
    wave_lds_sync();
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int g = 0; g < 4; ++g) raw[mb][g] = *reinterpret_cast<const bf16x4 *>(stg + r * ST_RS + 32 * mb + 8 * g + 4 * h);
    wave_lds_sync();
}

// rank1_block when every lane of the wave belongs to ONE ray: the row pointer is wave-uniform, so the 8 floats of a group
// (both lane halves) come from scalar loads and each lane picks its half - no vector-memory traffic at all
__device__ __forceinline__ void rank1_block_uniform(const float *g_row_u, float scale, int ch_base, int h, int n_valid, f32x16 &z) {
    // read-only for the whole launch: address space 4 (constant) lets the compiler use s_load for the uniform address
    typedef const float __attribute__((address_space(4))) cfloat;
    cfloat *gc = (cfloat *)(uintptr_t)g_row_u;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int c0 = ch_base + 8 * g;                     // uniform
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (c0 + j < n_valid) ? gc[c0 + j] : 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) z[4 * g + j] = scale * (h ? v[4 + j] : v[j]);
    }
}

// hidden layer: acc[2] = bias + W(64 x K) . frags ; K = 16 * nks
template <int NKS>
__device__ __forceinline__ void hidden_layer(const bf16_t *Ws, const float *bs, const bf16x8 (&frag)[NKS], int nks, int r, int h,
                                             f32x16 (&acc)[2]) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[mb][q] = bs[32 * mb + rho(q, h)];
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            if (s < nks) {
                bf16x8 a = *reinterpret_cast<const bf16x8 *>(Ws + (32 * mb + r) * RS + 16 * s + 8 * h);
                acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, frag[s], acc[mb], 0, 0, 0);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ forward
constexpr int FWD_WAVES_WIDE = 3;
constexpr int FWD_WAVES_NARROW = 1;
template <typename X1T, typename OutT, int NL, int OBMAX>
__global__ __launch_bounds__(256, (OBMAX > 2 ? FWD_WAVES_WIDE : FWD_WAVES_NARROW)) void mlp_fwd_mfma(FwdParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int OB = (p.out_dim + 31) / 32;
    // FwdLds(NL, OB), written as a chain: with the run-time OB, absolute offsets compile to different code (see mlp_lds.h)
    bf16_t *W0s = reinterpret_cast<bf16_t *>(smem);                  // [64][RS] natural k
    bf16_t *W1s = W0s + 64 * RS;                                     // [64][RS] permuted k (NL == 3)
    bf16_t *WLs = W1s + (NL == 3 ? 64 * RS : 0);                     // [OB*32][RS] permuted k
    float *b0s = reinterpret_cast<float *>(WLs + OB * 32 * RS);
    float *b1s = b0s + 64;
    float *bLs = b1s + 64;
    bf16_t *stg = reinterpret_cast<bf16_t *>(bLs + OB * 32) + (threadIdx.x >> 6) * (ST_BYTES / 2);      // wave-private staging tile

    stage_weight(W0s, RS, 64, 64, p.W[0], HID, p.in_dim, false, p.grp_L, p.grp_F);
    if (NL == 3) stage_weight(W1s, RS, 64, 64, p.W[1], HID, HID, true);
    stage_weight(WLs, RS, OB * 32, 64, p.W[NL - 1], p.out_dim, HID, true);
    for (int e = threadIdx.x; e < 64; e += blockDim.x) {
        b0s[e] = p.b[0][e];
        b1s[e] = NL == 3 ? p.b[1][e] : 0.0f;
    }
    for (int e = threadIdx.x; e < OB * 32; e += blockDim.x) bLs[e] = e < p.out_dim ? p.b[NL - 1][e] : 0.0f;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int r = lane & 31, h = lane >> 5;
    const int nks0 = p.in_pad / 16;
    const int64_t ntiles = (p.M + 31) / 32;
    const bool vec_out = (p.out_dim % 4) == 0;
    const X1T *x1 = reinterpret_cast<const X1T *>(p.x1);
    OutT *out = reinterpret_cast<OutT *>(p.out);

    // layer-0 B fragments straight from memory (features 16s + 8h .. +7 of sample m); the NEXT tile's fragments are
    // requested before the current tile is computed so that their HBM latency hides under the MFMA / epilogue work
    auto load_x = [&](int64_t tile, bf16x8 (&xf)[4]) {
        const int64_t m = tile * 32 + r;
        const bool live = tile < ntiles && m < p.M;
        const int64_t mc = live ? m : 0;
        const int32_t ray = (p.x2 && live) ? p.x2_index[mc] : 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int f0 = 16 * s + 8 * h;
            if (p.grp_L && live)
                xf[s] = load8(reinterpret_cast<const bf16_t *>(p.x1) + ((int64_t)(2 * s + h) * p.M + mc) * 8);
            else if (s < nks0 && live && f0 < p.k1)
                xf[s] = load8(x1 + mc * p.k1 + f0);
            else if (s < nks0 && live && f0 < p.k1 + p.k2p)
                xf[s] = load8(p.x2 + (int64_t)ray * p.k2p + (f0 - p.k1));
            else
                xf[s] = zero8();
            // columns at or beyond in_dim are absent, whatever they hold: a NaN there must not meet its zero weight (the group of 8 that
            // straddles in_dim and those behind it; XCD8 has in_dim = levels * feats, its padding positions are the encoders' zeros)
            if (!p.grp_L && f0 + 8 > p.in_dim) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (f0 + j >= p.in_dim) xf[s][j] = (bf16_t)0.0f;
            }
        }
    };
    const int64_t tile_step = (int64_t)gridDim.x * 4;
    bf16x8 xnext[4];
    load_x((int64_t)blockIdx.x * 4 + wave, xnext);
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += tile_step) {
        const int64_t m = tile * 32 + r;
        const bool live = m < p.M;
        bf16x8 xb[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) xb[s] = xnext[s];
        load_x(tile + tile_step, xnext);
        if constexpr (OBMAX <= 2) {     // narrow decoders only (the colour decoder): density = relu(column 0 of its input)
            if (p.col0_relu && h == 0 && live) p.col0_relu[m] = fmaxf((float)xb[0][0], 0.0f);
        }
        if constexpr (OBMAX > 2) {      // keep lane-constant addresses from being hoisted out of the tile loop and spilled
            asm volatile("" : "+v"(r), "+v"(h));
        }
        f32x16 acc[2];
        bf16x8 hb[4];
        hidden_layer<4>(W0s, b0s, xb, nks0, r, h, acc);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[mb][q] = fmaxf(acc[mb][q], 0.0f);
            pack_block(acc[mb], hb[2 * mb], hb[2 * mb + 1]);
        }
        const int rows_valid = (int)min((int64_t)32, p.M - tile * 32);
        if (p.hsave[0]) tile64_store(stg, reinterpret_cast<bf16_t *>(p.hsave[0]) + tile * 32 * HID, rows_valid, lane, r, h, acc);
        if (NL == 3) {
            hidden_layer<4>(W1s, b1s, hb, 4, r, h, acc);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[mb][q] = fmaxf(acc[mb][q], 0.0f);
                pack_block(acc[mb], hb[2 * mb], hb[2 * mb + 1]);
            }
            if (p.hsave[1]) tile64_store(stg, reinterpret_cast<bf16_t *>(p.hsave[1]) + tile * 32 * HID, rows_valid, lane, r, h, acc);
        }
        // ---- output layer
        auto out_block = [&](int ob, f32x16 &o) __attribute__((always_inline)) {      // bias + W_L[32ob .. 32ob+31, :] . h : 4 MFMAs
#pragma unroll
            for (int q = 0; q < 16; ++q) o[q] = bLs[32 * ob + rho(q, h)];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                bf16x8 a = *reinterpret_cast<const bf16x8 *>(WLs + (32 * ob + r) * RS + 16 * s + 8 * h);
                o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hb[s], o, 0, 0, 0);
            }
        };
        constexpr float LOG2E = 1.4426950408889634f;
        if constexpr (OBMAX > 2) {
            // Wide heads (e.g. 200 instance logits): ONE 32-channel block is live at a time.  Softmax is computed online
            // (running max / sum over the blocks), then the blocks are recomputed (4 MFMAs each - the matrix cores are
            // idle anyway) to be normalised and stored.  Holding all 7 blocks took 256 VGPRs = 1 wave per SIMD with every
            // latency exposed; this form fits 128 VGPRs = 4 waves per SIMD.
            float M_ = 0.0f, inv = 1.0f;
            if (p.act == PAG_ACT_SOFTMAX) {
                float mrun = -INFINITY, srun = 0.0f;
                for (int ob = 0; ob < OB; ++ob) {
                    f32x16 o;
                    out_block(ob, o);
                    const bool lastb = ob == OB - 1;
                    float bm = -INFINITY;
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (!lastb || 32 * ob + rho(q, h) < p.out_dim) bm = fmaxf(bm, o[q]);
                    const float mn = fmaxf(mrun, bm);
                    float bs = 0.0f;
                    const float mns = mn * LOG2E;
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (!lastb || 32 * ob + rho(q, h) < p.out_dim) bs += __builtin_amdgcn_exp2f(fmaf(o[q], LOG2E, -mns));
                    srun = srun * __builtin_amdgcn_exp2f((mrun - mn) * LOG2E) + bs;
                    mrun = mn;
                }
                const float mo = __shfl_xor(mrun, 32), so = __shfl_xor(srun, 32);
                M_ = fmaxf(mrun, mo);
                const float S_ = srun * __builtin_amdgcn_exp2f((mrun - M_) * LOG2E) + so * __builtin_amdgcn_exp2f((mo - M_) * LOG2E);
                inv = 1.0f / S_;
            }
            const float Ms = M_ * LOG2E;
            if (p.stats && p.act == PAG_ACT_SOFTMAX && live && h == 0) {
                float2 st2 = {Ms, inv};
                *reinterpret_cast<float2 *>(p.stats + 2 * m) = st2;
            }
            for (int ob = 0; ob < (p.out ? OB : 0); ++ob) {      // out == NULL: statistics only (pag_head_composite_fwd rebuilds)
                f32x16 o;
                out_block(ob, o);
                if (p.act == PAG_ACT_SOFTMAX) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) o[q] = __builtin_amdgcn_exp2f(fmaf(o[q], LOG2E, -Ms)) * inv;
                } else if (p.act == PAG_ACT_SIGMOID) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) o[q] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * o[q]));
                }
                if constexpr (sizeof(OutT) == 2) {
                    if ((p.out_dim & 7) == 0)
                        block32_store(stg, reinterpret_cast<bf16_t *>(p.out) + tile * 32 * p.out_dim, p.out_dim, 32 * ob, rows_valid, lane, r, h, o);
                    else if (live)
                        store_block(out + m * p.out_dim, 32 * ob, h, o, p.out_dim, vec_out);
                } else {
                    if (live) store_block(out + m * p.out_dim, 32 * ob, h, o, p.out_dim, vec_out);
                }
            }
        } else {
            f32x16 o[OBMAX];
#pragma unroll
            for (int ob = 0; ob < OBMAX; ++ob)
                if (ob < OB) out_block(ob, o[ob]);
            // Output activations on the accumulators.  The bf16 path uses the hardware exp2 / rcp (v_exp_f32, v_rcp_f32:
            // ~1 ulp) - an accurate expf() and a true division per element made this epilogue 5400 VALU instructions per
            // 32-sample tile and the kernel VALU-bound (rocprofv3 SQ_INSTS_VALU); only the last block can hold padding rows.
            if (p.act == PAG_ACT_SIGMOID) {
#pragma unroll
                for (int ob = 0; ob < OBMAX; ++ob)
                    if (ob < OB)
#pragma unroll
                        for (int q = 0; q < 16; ++q) o[ob][q] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * o[ob][q]));
            } else if (p.act == PAG_ACT_SOFTMAX) {
                float mx = -INFINITY;
#pragma unroll
                for (int ob = 0; ob < OBMAX; ++ob)
                    if (ob < OB)
#pragma unroll
                        for (int q = 0; q < 16; ++q)
                            if (ob < OB - 1 || 32 * ob + rho(q, h) < p.out_dim) mx = fmaxf(mx, o[ob][q]);
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                const float mxs = mx * LOG2E;
                float sum = 0.0f;
#pragma unroll
                for (int ob = 0; ob < OBMAX; ++ob)
                    if (ob < OB)
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const float e = (ob < OB - 1 || 32 * ob + rho(q, h) < p.out_dim) ? __builtin_amdgcn_exp2f(fmaf(o[ob][q], LOG2E, -mxs)) : 0.0f;
                            o[ob][q] = e;
                            sum += e;
                        }
                sum += __shfl_xor(sum, 32);
                const float inv = 1.0f / sum;
#pragma unroll
                for (int ob = 0; ob < OBMAX; ++ob)
                    if (ob < OB)
#pragma unroll
                        for (int q = 0; q < 16; ++q) o[ob][q] *= inv;
            }
            if (live) {
#pragma unroll
                for (int ob = 0; ob < OBMAX; ++ob)
                    if (ob < OB) store_block(out + m * p.out_dim, 32 * ob, h, o[ob], p.out_dim, vec_out);
            }
        }
    }
}

template <typename X1T, typename OutT, int NL>
void launch_fwd_mfma_nl(const FwdParams &p, hipStream_t st) {
    const dim3 grid(mlp_grid(p.M)), block(256);
    const int OB = (p.out_dim + 31) / 32;
    const size_t lds = FwdLds(NL, OB).bytes;
    if (OB <= 1) hipLaunchKernelGGL((mlp_fwd_mfma<X1T, OutT, NL, 1>), grid, block, lds, st, p);
    else if (OB <= 2) hipLaunchKernelGGL((mlp_fwd_mfma<X1T, OutT, NL, 2>), grid, block, lds, st, p);
    else if (OB <= 4) hipLaunchKernelGGL((mlp_fwd_mfma<X1T, OutT, NL, 4>), grid, block, lds, st, p);
    else hipLaunchKernelGGL((mlp_fwd_mfma<X1T, OutT, NL, 7>), grid, block, lds, st, p);
}
template <typename X1T, typename OutT>
void launch_fwd_mfma(const FwdParams &p, int n_layers, hipStream_t st) {
    if (n_layers == 2) launch_fwd_mfma_nl<X1T, OutT, 2>(p, st);
    else launch_fwd_mfma_nl<X1T, OutT, 3>(p, st);
}

// ----------------------------------------------------------------------------------------- backward
// 2 waves per SIMD: without the bound the 3-layer narrow variants took 252 VGPRs + 36 AGPRs (1 wave per SIMD); asking for 2 makes them fit 254 with no
// scratch.  The 33..64-output variants (OBMAX 2) would spill 150 - 350 B and stay at 1.
constexpr int BWD_WAVES = 2;
template <typename OutT, typename DxT, int NL, int OBMAX>
__global__ __launch_bounds__(256, (OBMAX == 2 ? 1 : BWD_WAVES)) void mlp_bwd_mfma(BwdParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int OB = (p.out_dim + 31) / 32;
    const BwdLds L(NL, OB);
    const int RSL = L.rsl;
    bf16_t *WLt = lds_at<bf16_t>(smem, L.WLt);                   // [64 in][RSL]  k = output channel (permuted)
    bf16_t *W1t = lds_at<bf16_t>(smem, L.W1t);                   // [64][RS]      (NL == 3)
    bf16_t *W0t = lds_at<bf16_t>(smem, L.W0t);                   // [64 in-feature rows][RS]
    stage_weight_t(WLt, RSL, 64, OB * 32, p.W[NL - 1], p.out_dim, HID);
    if (NL == 3) stage_weight_t(W1t, RS, 64, 64, p.W[1], HID, HID);
    if (p.dx1) stage_weight_t(W0t, RS, 64, 64, p.W[0], HID, p.in_dim, p.grp_L, p.grp_F);
    bf16_t *stg = lds_at<bf16_t>(smem, L.stg) + (threadIdx.x >> 6) * (L.stg_stride / 2);      // wave-private staging tile
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int r = lane & 31, h = lane >> 5;
    const int64_t ntiles = (p.M + 31) / 32;
    const bool vec_out = (p.out_dim % 4) == 0;
    const OutT *outp = reinterpret_cast<const OutT *>(p.out);

    typedef typename RawVec<OutT>::type RawO;
    constexpr bool PREFETCH = OBMAX <= 2;          // registers allow keeping the next tile's gradients in flight
    auto load_g = [&](int64_t tile, RawO (&rz)[OBMAX][4], RawO (&ry)[OBMAX][4]) {
        const int64_t m = tile * 32 + r;
        const int64_t mc = (tile < ntiles && m < p.M) ? m : p.M - 1;
        const OutT *gop = reinterpret_cast<const OutT *>(p.grad_out) + mc * p.out_dim;
        if (!p.g_ray) {
#pragma unroll
            for (int ob = 0; ob < OBMAX; ++ob)
                if (ob < OB) load_block_raw(gop, 32 * ob, h, rz[ob], p.out_dim, vec_out);
        }
        if (p.act != PAG_ACT_NONE) {
#pragma unroll
            for (int ob = 0; ob < OBMAX; ++ob)
                if (ob < OB) load_block_raw(outp + mc * p.out_dim, 32 * ob, h, ry[ob], p.out_dim, vec_out);
        }
    };
    const int64_t tile_step = (int64_t)gridDim.x * 4;
    RawO nz[PREFETCH ? OBMAX : 1][4], ny[PREFETCH ? OBMAX : 1][4];
    if constexpr (PREFETCH) load_g((int64_t)blockIdx.x * 4 + wave, nz, ny);
    bf16x8 hnext[PREFETCH ? NL - 1 : 1][4];      // next tile's hidden rows, in flight during the current tile
    auto fetch_h = [&](int64_t tile, bf16x8 (&hn)[PREFETCH ? NL - 1 : 1][4]) __attribute__((always_inline)) {
        if (tile < ntiles) {
            const int rv = (int)min((int64_t)32, p.M - tile * 32);
#pragma unroll
            for (int l = 0; l < NL - 1; ++l)
                tile64_fetch(reinterpret_cast<const bf16_t *>(p.hsave[l]) + tile * 32 * HID, rv, lane, hn[l]);
        }
    };
    if constexpr (PREFETCH) fetch_h((int64_t)blockIdx.x * 4 + wave, hnext);
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += tile_step) {
        if constexpr (OBMAX > 2) {      // keep lane-constant addresses from being hoisted out of the tile loop and spilled
            asm volatile("" : "+v"(r), "+v"(h));
        }
        const int64_t m = tile * 32 + r;
        const bool live = m < p.M;
        const int64_t mc = live ? m : p.M - 1;
        // ReLU masks of the hidden layers: requested first, consumed after the first MFMA chain
        const int rows_valid = (int)min((int64_t)32, p.M - tile * 32);
        bf16x4 hraw[NL - 1][2][4];
        if constexpr (PREFETCH) {
#pragma unroll
            for (int l = 0; l < NL - 1; ++l) tile64_unstage(stg, hnext[l], lane, r, h, hraw[l]);
            fetch_h(tile + tile_step, hnext);
        } else {
#pragma unroll
            for (int l = 0; l < NL - 1; ++l)
                tile64_load(stg, reinterpret_cast<const bf16_t *>(p.hsave[l]) + tile * 32 * HID, rows_valid, lane, r, h, hraw[l]);
        }
        // dx1_accumulate: the other decoder's gradient pieces are requested now and added at the end of the tile
        bf16x4 oldx[2][4];
        if (p.dx1_acc) {
            const bf16_t *dg = reinterpret_cast<const bf16_t *>(p.dx1);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    oldx[mb][g] = *reinterpret_cast<const bf16x4 *>(dg + ((int64_t)(4 * mb + g) * p.M + mc) * 8 + 4 * h);
        }
        // ---- dz of the output layer -> bf16 B fragments (k-steps of the first backward MFMA chain W_L^T . dz_L)
        bf16x8 zb[OBMAX > 2 ? 2 : 2 * OBMAX];          // wide heads consume each block's two fragments immediately
        f32x16 acc[2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[mb][q] = 0.0f;
        const bool tile_full = (tile + 1) * 32 <= p.M;      // wave-uniform: only the last tile has dead lanes
        auto finish_block = [&](int ob, f32x16 &zz) __attribute__((always_inline)) {      // zero dead lanes, store dz, pack
            if (!tile_full) {
#pragma unroll
                for (int q = 0; q < 16; ++q) zz[q] = live ? zz[q] : 0.0f;
            }
            const int zi = OBMAX > 2 ? 0 : 2 * ob;
            pack_block(zz, zb[zi], zb[zi + 1]);
            if (OBMAX > 2 && (p.out_dim & 7) == 0)
                block32_store(stg, reinterpret_cast<bf16_t *>(p.dz[NL - 1]) + tile * 32 * p.out_dim, p.out_dim, 32 * ob, rows_valid, lane, r, h, zz);
            else if (live)
                store_block(reinterpret_cast<bf16_t *>(p.dz[NL - 1]) + m * p.out_dim, 32 * ob, h, zz, p.out_dim, vec_out);
            if constexpr (OBMAX > 2) {
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        bf16x8 a = *reinterpret_cast<const bf16x8 *>(WLt + (32 * mb + r) * RSL + 16 * (2 * ob + half) + 8 * h);
                        acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, zb[half], acc[mb], 0, 0, 0);
                    }
            }
        };
        if constexpr (PREFETCH) {
            f32x16 z[OBMAX];
            RawO rz[OBMAX][4], ry[OBMAX][4];
#pragma unroll
            for (int ob = 0; ob < OBMAX; ++ob)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    rz[ob][g] = nz[ob][g];
                    ry[ob][g] = ny[ob][g];
                }
            load_g(tile + tile_step, nz, ny);
#pragma unroll
            for (int ob = 0; ob < OBMAX; ++ob)
                if (ob < OB) raw_to_block(rz[ob], z[ob]);
            if (p.g_ray) {
                const int gi = p.g_index[mc], gi0 = __builtin_amdgcn_readfirstlane(gi);
                const float sc = p.g_ray_scale ? __fmul_rn(p.g_scale[mc], p.g_ray_scale[gi]) : p.g_scale[mc];
                if (__all(gi == gi0)) {
                    const float *g_row_u = p.g_ray + (int64_t)gi0 * p.out_dim;
#pragma unroll
                    for (int ob = 0; ob < OBMAX; ++ob)
                        if (ob < OB) rank1_block_uniform(g_row_u, sc, 32 * ob, h, p.out_dim, z[ob]);
                } else {
                    const float *g_row = p.g_ray + (int64_t)gi * p.out_dim;
#pragma unroll
                    for (int ob = 0; ob < OBMAX; ++ob)
                        if (ob < OB) rank1_block(g_row, sc, 32 * ob, h, p.out_dim, z[ob]);
                }
            }
            if (p.act == PAG_ACT_SIGMOID) {
#pragma unroll
                for (int ob = 0; ob < OBMAX; ++ob)
                    if (ob < OB)
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const float y = (float)ry[ob][q >> 2][q & 3];
                            z[ob][q] = z[ob][q] * y * (1.0f - y);
                        }
            } else if (p.act == PAG_ACT_SOFTMAX) {
                float dot = 0.0f;
#pragma unroll
                for (int ob = 0; ob < OBMAX; ++ob)
                    if (ob < OB)
#pragma unroll
                        for (int q = 0; q < 16; ++q) dot += z[ob][q] * (float)ry[ob][q >> 2][q & 3];
                dot += __shfl_xor(dot, 32);
#pragma unroll
                for (int ob = 0; ob < OBMAX; ++ob)
                    if (ob < OB)
#pragma unroll
                        for (int q = 0; q < 16; ++q) z[ob][q] = (float)ry[ob][q >> 2][q & 3] * (z[ob][q] - dot);
            }
#pragma unroll
            for (int ob = 0; ob < OBMAX; ++ob) {
                if (ob < OB) {
                    finish_block(ob, z[ob]);
                } else {
                    zb[2 * ob] = zero8();
                    zb[2 * ob + 1] = zero8();
                }
            }
        } else {
            // wide heads: two passes over the gradient / probability rows (dot product for the softmax backward, then dz)
            // keep only ONE 32-channel block live at a time instead of all of them (256 VGPRs -> 1 wave per SIMD before).
            // The passes form one software pipeline over 2*OB steps: the global loads of step s+1 (16 bytes per lane,
            // fully coalesced) are in flight while step s goes through the LDS staging tile and the MFMAs - profiling
            // showed this kernel parked on memory 69 % of the time with one exposed round trip per block.
            const int g_idx1 = p.g_ray ? p.g_index[mc] : 0;
            const int g_idx0 = __builtin_amdgcn_readfirstlane(g_idx1);
            const bool g_uni = __all(g_idx1 == g_idx0);      // whole tile inside one ray (the common case)
            const float *g_row1 = p.g_ray ? p.g_ray + (int64_t)g_idx1 * p.out_dim : nullptr;
            const float *g_row_u = p.g_ray ? p.g_ray + (int64_t)g_idx0 * p.out_dim : nullptr;
            const float g_sc1 = p.g_ray ? (p.g_ray_scale ? __fmul_rn(p.g_scale[mc], p.g_ray_scale[g_idx1]) : p.g_scale[mc]) : 0.0f;
            const bool r1 = p.g_ray != nullptr;
            const bool need_y = p.act != PAG_ACT_NONE;
            const int n1 = p.act == PAG_ACT_SOFTMAX ? OB : 0, n_steps = n1 + OB;
            float dot = 0.0f;
            bool fast = false;
            if constexpr (sizeof(OutT) == 2) fast = (p.out_dim & 7) == 0;
            if (fast) {
                const bf16_t *gtile_g = reinterpret_cast<const bf16_t *>(p.grad_out) + tile * 32 * p.out_dim;
                const bf16_t *gtile_y = reinterpret_cast<const bf16_t *>(p.out) + tile * 32 * p.out_dim;
                bf16x8 cz[2], cy[2], nzr[2], nyr[2];
                auto gfetch = [&](int ob, bf16x8 (&fz)[2], bf16x8 (&fy)[2]) __attribute__((always_inline)) {
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        const int row = it * 16 + (lane >> 2), c = 32 * ob + (lane & 3) * 8;
                        const bool ok = row < rows_valid && c < p.out_dim;
                        fz[it] = (ok && !r1) ? *reinterpret_cast<const bf16x8 *>(gtile_g + (int64_t)row * p.out_dim + c) : zero8();
                        fy[it] = (ok && need_y) ? *reinterpret_cast<const bf16x8 *>(gtile_y + (int64_t)row * p.out_dim + c) : zero8();
                    }
                };
                gfetch(0, cz, cy);
                for (int step = 0; step < n_steps; ++step) {
                    const int ob = step < n1 ? step : step - n1;
                    if (step + 1 < n_steps) gfetch(step + 1 < n1 ? step + 1 : step + 1 - n1, nzr, nyr);
                    bf16x4 rz1[4], ry1[4];
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        const int row = it * 16 + (lane >> 2), c = (lane & 3) * 8;
                        *reinterpret_cast<bf16x8 *>(stg + row * ST_RS + c) = cz[it];
                        *reinterpret_cast<bf16x8 *>(stg + row * ST_RS + 32 + c) = cy[it];
                    }
                    wave_lds_sync();
                    block32_read(stg, 0, r, h, rz1);
                    block32_read(stg, 32, r, h, ry1);
                    wave_lds_sync();
                    f32x16 zz;
                    if (r1 && g_uni) rank1_block_uniform(g_row_u, g_sc1, 32 * ob, h, p.out_dim, zz);
                    else if (r1) rank1_block(g_row1, g_sc1, 32 * ob, h, p.out_dim, zz);
                    else raw_to_block(rz1, zz);
                    if (step < n1) {
#pragma unroll
                        for (int q = 0; q < 16; ++q) dot += zz[q] * (float)ry1[q >> 2][q & 3];
                        if (step == n1 - 1) dot += __shfl_xor(dot, 32);
                    } else {
                        if (p.act == PAG_ACT_SIGMOID) {
#pragma unroll
                            for (int q = 0; q < 16; ++q) {
                                const float y = (float)ry1[q >> 2][q & 3];
                                zz[q] = zz[q] * y * (1.0f - y);
                            }
                        } else if (p.act == PAG_ACT_SOFTMAX) {
#pragma unroll
                            for (int q = 0; q < 16; ++q) zz[q] = (float)ry1[q >> 2][q & 3] * (zz[q] - dot);
                        }
                        finish_block(ob, zz);
                    }
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        cz[it] = nzr[it];
                        cy[it] = nyr[it];
                    }
                }
            } else {      // generic wide path (fp32 outputs or out_dim % 8 != 0): direct per-lane row accesses
                const OutT *gop = reinterpret_cast<const OutT *>(p.grad_out) + mc * p.out_dim;
                const OutT *yop = outp + mc * p.out_dim;
                for (int step = 0; step < n_steps; ++step) {
                    const int ob = step < n1 ? step : step - n1;
                    RawO rz1[4], ry1[4];
                    if (!r1) load_block_raw(gop, 32 * ob, h, rz1, p.out_dim, vec_out);
                    if (need_y) load_block_raw(yop, 32 * ob, h, ry1, p.out_dim, vec_out);
                    f32x16 zz;
                    if (r1) rank1_block(g_row1, g_sc1, 32 * ob, h, p.out_dim, zz);
                    else raw_to_block(rz1, zz);
                    if (step < n1) {
#pragma unroll
                        for (int q = 0; q < 16; ++q) dot += zz[q] * (float)ry1[q >> 2][q & 3];
                        if (step == n1 - 1) dot += __shfl_xor(dot, 32);
                    } else {
                        if (p.act == PAG_ACT_SIGMOID) {
#pragma unroll
                            for (int q = 0; q < 16; ++q) {
                                const float y = (float)ry1[q >> 2][q & 3];
                                zz[q] = zz[q] * y * (1.0f - y);
                            }
                        } else if (p.act == PAG_ACT_SOFTMAX) {
#pragma unroll
                            for (int q = 0; q < 16; ++q) zz[q] = (float)ry1[q >> 2][q & 3] * (zz[q] - dot);
                        }
                        finish_block(ob, zz);
                    }
                }
            }
        }
        // ---- back through the output layer: dA = W_L^T . dz_L (already accumulated per block for wide heads),
        //      masked by the saved ReLU output
        bf16x8 hb[4];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            if constexpr (OBMAX <= 2) {
#pragma unroll
                for (int s = 0; s < 2 * OBMAX; ++s) {
                    if (s < 2 * OB) {
                        bf16x8 a = *reinterpret_cast<const bf16x8 *>(WLt + (32 * mb + r) * RSL + 16 * s + 8 * h);
                        acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, zb[s], acc[mb], 0, 0, 0);
                    }
                }
            }
            f32x16 hv;
            raw_to_block(hraw[NL - 2][mb], hv);
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[mb][q] = (hv[q] > 0.0f && live) ? acc[mb][q] : 0.0f;
            pack_block(acc[mb], hb[2 * mb], hb[2 * mb + 1]);
        }
        tile64_store(stg, reinterpret_cast<bf16_t *>(p.dz[NL - 2]) + tile * 32 * HID, rows_valid, lane, r, h, acc);
        if (NL == 3) {
            bf16x8 hb2[4];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[mb][q] = 0.0f;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    bf16x8 a = *reinterpret_cast<const bf16x8 *>(W1t + (32 * mb + r) * RS + 16 * s + 8 * h);
                    acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hb[s], acc[mb], 0, 0, 0);
                }
                f32x16 hv;
                raw_to_block(hraw[0][mb], hv);
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[mb][q] = (hv[q] > 0.0f && live) ? acc[mb][q] : 0.0f;
                pack_block(acc[mb], hb2[2 * mb], hb2[2 * mb + 1]);
            }
            tile64_store(stg, reinterpret_cast<bf16_t *>(p.dz[0]) + tile * 32 * HID, rows_valid, lane, r, h, acc);
#pragma unroll
            for (int s = 0; s < 4; ++s) hb[s] = hb2[s];
        }
        // ---- dx1 = (W_0^T . dz_0)[0:k1]
        if (p.dx1) {
            DxT *dx = reinterpret_cast<DxT *>(p.dx1);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                if (32 * mb < p.k1) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[mb][q] = 0.0f;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        bf16x8 a = *reinterpret_cast<const bf16x8 *>(W0t + (32 * mb + r) * RS + 16 * s + 8 * h);
                        acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hb[s], acc[mb], 0, 0, 0);
                    }
                    if (live && !p.grp_L) {
                        // extra gradient of input column 0 (the density read off the density decoder's first output,
                        // pc_nerf/panoptic_delta_nef.py:188): added here instead of a zero-padded [M,k1] tensor + add pass
                        if (p.dx_col0 && mb == 0 && h == 0 && (!p.dx_col0_gate || p.dx_col0_gate[m] > 0.0f)) acc[0][0] += p.dx_col0[m];
                        store_block(dx + m * p.k1, 32 * mb, h, acc[mb], p.k1, true);
                    }
                    if (live && p.grp_L) {      // XCD8: row 32mb + 8g + 4h + j of dx^T -> piece [4mb + g][m][4h + j]
                        bf16_t *dg = reinterpret_cast<bf16_t *>(p.dx1);
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            bf16x4 *dst = reinterpret_cast<bf16x4 *>(dg + ((int64_t)(4 * mb + g) * p.M + m) * 8 + 4 * h);
                            if (p.dx1_acc) {      // second decoder on the same input: add to the first one's gradient in place
#pragma unroll
                                for (int j = 0; j < 4; ++j) acc[mb][4 * g + j] += (float)oldx[mb][g][j];
                            }
                            bf16x4 v = {(bf16_t)acc[mb][4 * g], (bf16_t)acc[mb][4 * g + 1], (bf16_t)acc[mb][4 * g + 2], (bf16_t)acc[mb][4 * g + 3]};
                            *dst = v;
                        }
                    }
                }
            }
        }
    }
}

template <typename OutT, typename DxT, int NL>
void launch_bwd_mfma_nl(const BwdParams &p, hipStream_t st) {
    const dim3 grid(mlp_grid(p.M)), block(256);
    const int OB = (p.out_dim + 31) / 32;
    const size_t lds = BwdLds(NL, OB).bytes;
    if (OB <= 1) hipLaunchKernelGGL((mlp_bwd_mfma<OutT, DxT, NL, 1>), grid, block, lds, st, p);
    else if (OB <= 2) hipLaunchKernelGGL((mlp_bwd_mfma<OutT, DxT, NL, 2>), grid, block, lds, st, p);
    else if (OB <= 4) hipLaunchKernelGGL((mlp_bwd_mfma<OutT, DxT, NL, 4>), grid, block, lds, st, p);
    else hipLaunchKernelGGL((mlp_bwd_mfma<OutT, DxT, NL, 7>), grid, block, lds, st, p);
}
template <typename OutT, typename DxT>
void launch_bwd_mfma(const BwdParams &p, int n_layers, hipStream_t st) {
    if (n_layers == 2) launch_bwd_mfma_nl<OutT, DxT, 2>(p, st);
    else launch_bwd_mfma_nl<OutT, DxT, 3>(p, st);
}

}  // namespace
