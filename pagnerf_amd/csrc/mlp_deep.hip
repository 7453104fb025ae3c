// Semantic-NeRF decoder for gfx950 (pc_nerf/semantic_nerf.py: PE10 -> eight Linear + ReLU at width 256 with a skip into layer 5 -> lout -> three
// heads), the first decoder here that is bound by arithmetic and not by activation bandwidth.
//
// The transposed-MFMA scheme of mlp.hip carries over: H^T[neurons x samples] = W[out x in] . X^T[in x samples] with v_mfma_f32_32x32x16_bf16, the
// sample on the lane, so a layer's accumulator blocks - after bias / ReLU and a pairwise conversion to bf16 - ARE the next layer's B operand; the
// weights' input index is staged with bits 2 and 3 swapped (swap23) so that the hardware's k order matches the accumulator's row order.
//   * one workgroup = 8 waves x 32 samples = 256 samples per staged layer.  A wave holds its tile's 256 x 32 activations as 16 B fragments (64 VGPRs)
//     and the layer's output as 8 accumulator blocks (128 VGPRs); every MFMA takes its A fragment from LDS with one ds_read_b128, which at 8 waves is
//     half of the LDS read rate.
//   * one 256 x 256 bf16 layer (rows padded by 16 B: 132 KiB, 133 KiB with its fp32 bias) is resident at a time.  The weights are converted, permuted and padded ONCE per call into
//     a packed image (deep_pack_kernel), so staging a layer is a flat 16-B copy L2 -> LDS.  256 samples per staged layer = 2 . 256^3 FLOP per 128 KiB
//     = 256 FLOP per byte pulled from L2; a workgroup walks its batches one after another (grid = one workgroup per CU).
//   * the positional encodings are computed in the kernel with the accurate sincosf (arguments reach 512 rad), written to a per-wave LDS scratch and
//     read back in the B-fragment layout.
// Training: the forward keeps every Linear's bf16 input ("native" layout, mlp_native.h), deep_bwd_kernel runs the data gradients through the chain on the
// transposed weights and writes every layer's dz (bf16), deep_wgrad_kernel forms dz^T . input per (layer, 128 input columns, slice of the samples)
// into slabs and deep_wgrad_finish_kernel adds the slices in a fixed order: no atomics, two runs give the same bits.
// The tile helpers (mm, init_bias, pack_frags, mask_frags, store_native, stage_transposed) are mlp_native.h's, shared with mlp_h128.hip.
#include "mlp_native.h"

namespace {

constexpr int DH = 256, DHH = 128;
constexpr int S256 = 264, S128 = 136, S64 = 72, S16 = 24;      // LDS row strides (bf16 elements): width + 16 B
constexpr int DEEP_WG = 512;
constexpr int MAX_SPLIT = 32;

// forward image (bytes)
constexpr int SZ_L0 = DH * S64 * 2 + DH * 4;
constexpr int SZ_LH = DH * S256 * 2 + DH * 4;
constexpr int SZ_L5E = DH * S64 * 2;
constexpr int HA_WD = 0, HA_BD = 32 * S256 * 2, HA_WS1 = HA_BD + 128, HA_BS1 = HA_WS1 + DHH * S256 * 2, HA_WS2 = HA_BS1 + DHH * 4,
              HA_BS2 = HA_WS2 + 32 * S128 * 2, SZ_HA = HA_BS2 + 128;
constexpr int HB_WC1F = 0, HB_BC1 = DHH * S256 * 2, HB_WC1V = HB_BC1 + DHH * 4, HB_WC2 = HB_WC1V + DHH * S64 * 2, HB_BC2 = HB_WC2 + 32 * S128 * 2,
              SZ_HB = HB_BC2 + 128;
__host__ __device__ constexpr int64_t f_layer(int l) { return (int64_t)SZ_L0 + (int64_t)(l - 1) * SZ_LH + (l > 5 ? SZ_L5E : 0); }   // l = 1 .. 8
constexpr int64_t F_L5E = f_layer(5) + SZ_LH, F_HA = f_layer(8) + SZ_LH, F_HB = F_HA + SZ_HA, F_TOTAL = F_HB + SZ_HB;
// backward image
constexpr int TB_WC2T = 0, TB_WC1T = DHH * S16 * 2, SZ_TB = TB_WC1T + DH * S128 * 2;
constexpr int TA_WS2T = 0, TA_WS1T = DHH * S16 * 2, TA_WD = TA_WS1T + DH * S128 * 2, SZ_TA = TA_WD + DH * 4;
constexpr int SZ_T = DH * S256 * 2;
constexpr int64_t B_TB = 0, B_TA = SZ_TB;
__host__ __device__ constexpr int64_t b_layer(int l) { return (int64_t)SZ_TB + SZ_TA + (int64_t)(l - 1) * SZ_T; }                  // l = 1 .. 8
constexpr int64_t B_TOTAL = b_layer(8) + SZ_T;
constexpr int SCRATCH_OFF = 96 * 1024;       // per-wave PE scratch [32][S64], above the two images that are resident while it is used
static_assert(SZ_L0 <= SCRATCH_OFF && SZ_HB <= SCRATCH_OFF && SCRATCH_OFF + 8 * 32 * S64 * 2 <= SZ_LH, "PE scratch overlaps a staged image");
static_assert(SZ_LH <= 160 * 1024 && SZ_T <= SZ_LH && SZ_TA <= SZ_LH, "LDS");
static_assert(SZ_L0 % 16 == 0 && SZ_LH % 16 == 0 && SZ_L5E % 16 == 0 && SZ_HA % 16 == 0 && SZ_HB % 16 == 0 && SZ_TB % 16 == 0 && SZ_TA % 16 == 0, "16-B copies");

// saved planes (columns before the plane, per sample): e, view PE, h0 .. h7, feats, semantic hidden, colour hidden
constexpr int SV_E = 0, SV_V = 64, SV_HS = 128 + 9 * DH, SV_HC = SV_HS + DHH, SV_TOTAL = SV_HC + DHH;
__host__ __device__ constexpr int sv_h(int l) { return 128 + l * DH; }                 // l = 0 .. 8 (8 = feats)
// dz planes: dz0 .. dz8, semantic hidden, colour hidden, semantic out (32), colour out (32), density (32)
constexpr int DZ_S1 = 9 * DH, DZ_C1 = DZ_S1 + DHH, DZ_S2 = DZ_C1 + DHH, DZ_C2 = DZ_S2 + 32, DZ_D = DZ_C2 + 32, DZ_TOTAL = DZ_D + 32;

// ------------------------------------------------------------------------------------------------------------------------- weight images
struct PackJob {
    int64_t dst;
    const float *W;
    int rows_pad, stride, n_out, ld, col0, ncols, mode;      // mode 0: [out][in permuted], 1: transposed [in][out permuted], 2: f32 copy of n_out values
};
constexpr int MAX_PACK = 48;
struct PackJobs {
    PackJob j[MAX_PACK];
};

__global__ void deep_pack_kernel(PackJobs jobs, char *blob) {
    const PackJob J = jobs.j[blockIdx.y];
    const int step = (int)(gridDim.x * blockDim.x);
    if (J.mode == 2) {
        float *d = reinterpret_cast<float *>(blob + J.dst);
        for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < J.rows_pad; i += step) d[i] = i < J.n_out ? J.W[i] : 0.0f;
        return;
    }
    bf16_t *d = reinterpret_cast<bf16_t *>(blob + J.dst);
    const int total = J.rows_pad * J.stride;
    for (int e = (int)(blockIdx.x * blockDim.x + threadIdx.x); e < total; e += step) {
        const int row = e / J.stride, k = swap23(e - row * J.stride);
        float v = 0.0f;
        if (J.mode == 0) {
            if (row < J.n_out && k < J.ncols) v = J.W[(int64_t)row * J.ld + J.col0 + k];
        } else {
            if (row < J.ncols && k < J.n_out) v = J.W[(int64_t)k * J.ld + J.col0 + row];
        }
        d[e] = (bf16_t)v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------- shared pieces
__device__ __forceinline__ void stage(char *lds, const char *src, int bytes) {
#pragma unroll 4
    for (int o = (int)threadIdx.x * 16; o < bytes; o += DEEP_WG * 16) *reinterpret_cast<uint4 *>(lds + o) = *reinterpret_cast<const uint4 *>(src + o);
}

// PE10 of one sample (x, sin(x 2^k) frequency-major, cos(x 2^k)) into the wave's scratch row; lane half h takes the
// frequencies of its parity.  Column 63 is padding.
__device__ __forceinline__ void pe_write(bf16_t *row, int h, float x0, float x1, float x2) {
    if (h == 0) {
        row[0] = (bf16_t)x0;
        row[1] = (bf16_t)x1;
        row[2] = (bf16_t)x2;
    } else {
        row[63] = (bf16_t)0.0f;
    }
#pragma unroll
    for (int kk = 0; kk < 5; ++kk) {
        const int k = 2 * kk + h;
        const float sc = (float)(1 << k);
        float s, c;
        sincosf(x0 * sc, &s, &c);
        row[3 + 3 * k] = (bf16_t)s;
        row[33 + 3 * k] = (bf16_t)c;
        sincosf(x1 * sc, &s, &c);
        row[4 + 3 * k] = (bf16_t)s;
        row[34 + 3 * k] = (bf16_t)c;
        sincosf(x2 * sc, &s, &c);
        row[5 + 3 * k] = (bf16_t)s;
        row[35 + 3 * k] = (bf16_t)c;
    }
}
__device__ __forceinline__ void pe_read(const bf16_t *row, int h, bf16x8 (&e)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const bf16x4 lo = *reinterpret_cast<const bf16x4 *>(row + 16 * s + 4 * h);
        const bf16x4 hi = *reinterpret_cast<const bf16x4 *>(row + 16 * s + 8 + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            e[s][i] = lo[i];
            e[s][4 + i] = hi[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------- forward
struct DeepFwdParams {
    const float *coords, *ray_d;
    int64_t M, ntile;            // ntile: 32-sample tiles, a multiple of 8
    int C, channels;
    const char *blob;
    float *density, *rgb, *sem;
    bf16_t *save;                // NULL, or the planes' base
};

__global__ __launch_bounds__(DEEP_WG) void deep_fwd_kernel(DeepFwdParams P) {
    __shared__ __attribute__((aligned(16))) char lds[SZ_LH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    bf16_t *scr = reinterpret_cast<bf16_t *>(lds + SCRATCH_OFF) + (wave * 32 + r) * S64;
    const bf16_t *W = reinterpret_cast<const bf16_t *>(lds);
    const int64_t nbatch = P.ntile / 8, plane = P.ntile * 32;
    for (int64_t batch = blockIdx.x; batch < nbatch; batch += gridDim.x) {
        const int64_t tile = batch * 8 + wave, m = tile * 32 + r;
        const bool ok = m < P.M;
        const int64_t mc = ok ? m : P.M - 1;
        const float x0 = P.coords[mc * 3], x1 = P.coords[mc * 3 + 1], x2 = P.coords[mc * 3 + 2];
        __syncthreads();
        stage(lds, P.blob, SZ_L0);
        pe_write(scr, h, x0, x1, x2);
        __syncthreads();
        bf16x8 e[4], hin[16];
        f32x16 acc[8];
        pe_read(scr, h, e);
        if (P.save) store_native<2>(P.save + plane * SV_E, tile, lane, e);
        init_bias<8>(acc, reinterpret_cast<const float *>(lds + DH * S64 * 2), h);
        mm<8, 4>(acc, e, W, S64, lane);
        pack_frags<8>(acc, hin, true);
        if (P.save) store_native<8>(P.save + plane * sv_h(0), tile, lane, hin);
#pragma unroll 1
        for (int l = 1; l <= 8; ++l) {
            __syncthreads();
            stage(lds, P.blob + f_layer(l), SZ_LH);
            __syncthreads();
            init_bias<8>(acc, reinterpret_cast<const float *>(lds + DH * S256 * 2), h);
            mm<8, 16>(acc, hin, W, S256, lane);
            if (l == 5) {
                __syncthreads();
                stage(lds, P.blob + F_L5E, SZ_L5E);
                __syncthreads();
                mm<8, 4>(acc, e, W, S64, lane);
            }
            pack_frags<8>(acc, hin, l < 8);
            if (P.save) store_native<8>(P.save + plane * sv_h(l), tile, lane, hin);
        }
        // hin = feats (bf16).  Density and semantics
        if (P.channels & (PAG_DEEP_DENSITY | PAG_DEEP_SEMANTICS)) {
            __syncthreads();
            stage(lds, P.blob + F_HA, SZ_HA);
            __syncthreads();
            if (P.channels & PAG_DEEP_DENSITY) {
                f32x16 d[1];
                init_bias<1>(d, reinterpret_cast<const float *>(lds + HA_BD), h);
                mm<1, 16>(d, hin, reinterpret_cast<const bf16_t *>(lds + HA_WD), S256, lane);
                if (ok && h == 0) P.density[m] = fmaxf(d[0][0], 0.0f);
            }
            if (P.channels & PAG_DEEP_SEMANTICS) {
                f32x16 a[4], o[1];
                bf16x8 h2[8];
                init_bias<4>(a, reinterpret_cast<const float *>(lds + HA_BS1), h);
                mm<4, 16>(a, hin, reinterpret_cast<const bf16_t *>(lds + HA_WS1), S256, lane);
                pack_frags<4>(a, h2, true);
                if (P.save) store_native<4>(P.save + plane * SV_HS, tile, lane, h2);
                init_bias<1>(o, reinterpret_cast<const float *>(lds + HA_BS2), h);
                mm<1, 8>(o, h2, reinterpret_cast<const bf16_t *>(lds + HA_WS2), S128, lane);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int row = rho(q, h);
                    if (ok && row < P.C) P.sem[m * P.C + row] = o[0][q];
                }
            }
        }
        if (P.channels & PAG_DEEP_RGB) {
            const float d0 = -P.ray_d[mc * 3], d1 = -P.ray_d[mc * 3 + 1], d2 = -P.ray_d[mc * 3 + 2];
            __syncthreads();
            stage(lds, P.blob + F_HB, SZ_HB);
            pe_write(scr, h, d0, d1, d2);
            __syncthreads();
            bf16x8 v[4], h2[8];
            f32x16 a[4], o[1];
            pe_read(scr, h, v);
            if (P.save) store_native<2>(P.save + plane * SV_V, tile, lane, v);
            init_bias<4>(a, reinterpret_cast<const float *>(lds + HB_BC1), h);
            mm<4, 16>(a, hin, reinterpret_cast<const bf16_t *>(lds + HB_WC1F), S256, lane);
            mm<4, 4>(a, v, reinterpret_cast<const bf16_t *>(lds + HB_WC1V), S64, lane);
            pack_frags<4>(a, h2, true);
            if (P.save) store_native<4>(P.save + plane * SV_HC, tile, lane, h2);
            init_bias<1>(o, reinterpret_cast<const float *>(lds + HB_BC2), h);
            mm<1, 8>(o, h2, reinterpret_cast<const bf16_t *>(lds + HB_WC2), S128, lane);
            if (ok && h == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) P.rgb[m * 3 + c] = 1.0f / (1.0f + expf(-o[0][c]));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ backward: data gradients
struct DeepBwdParams {
    int64_t M, ntile;
    int C;
    const char *blob;
    const float *g_den, *g_rgb, *g_sem, *density, *rgb;
    const bf16_t *save;
    bf16_t *dz;
};

__device__ __forceinline__ float round_bf16(float v) { return (float)(bf16_t)v; }

__global__ __launch_bounds__(DEEP_WG) void deep_bwd_kernel(DeepBwdParams P) {
    __shared__ __attribute__((aligned(16))) char lds[SZ_T];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t nbatch = P.ntile / 8, plane = P.ntile * 32;
    for (int64_t batch = blockIdx.x; batch < nbatch; batch += gridDim.x) {
        const int64_t tile = batch * 8 + wave, m = tile * 32 + r;
        const bool ok = m < P.M;
        f32x16 acc[8];
        bf16x8 hin[16];
        zero_acc<8>(acc);
        __syncthreads();
        stage(lds, P.blob + B_TB, SZ_TB);
        __syncthreads();
        {   // colour head: rgb = sigmoid(z)
            f32x16 v[1], a[4];
            bf16x8 z1[2], z2[8];
            zero_acc<1>(v);
            if (ok && h == 0 && P.g_rgb) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float y = P.rgb[m * 3 + c];
                    v[0][c] = P.g_rgb[m * 3 + c] * y * (1.0f - y);
                }
            }
            pack_frags<1>(v, z1, false);
            store_native<1>(P.dz + plane * DZ_C2, tile, lane, z1);
            zero_acc<4>(a);
            mm<4, 1>(a, z1, reinterpret_cast<const bf16_t *>(lds + TB_WC2T), S16, lane);
            mask_frags<4>(a, P.save + plane * SV_HC, tile, lane, z2);
            store_native<4>(P.dz + plane * DZ_C1, tile, lane, z2);
            mm<8, 8>(acc, z2, reinterpret_cast<const bf16_t *>(lds + TB_WC1T), S128, lane);
        }
        __syncthreads();
        stage(lds, P.blob + B_TA, SZ_TA);
        __syncthreads();
        {   // semantic head (raw logits) and density
            f32x16 v[1], a[4];
            bf16x8 z1[2], z2[8];
            zero_acc<1>(v);
            if (ok && P.g_sem) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int row = rho(q, h);
                    if (row < P.C) v[0][q] = P.g_sem[m * P.C + row];
                }
            }
            pack_frags<1>(v, z1, false);
            store_native<1>(P.dz + plane * DZ_S2, tile, lane, z1);
            zero_acc<4>(a);
            mm<4, 1>(a, z1, reinterpret_cast<const bf16_t *>(lds + TA_WS2T), S16, lane);
            mask_frags<4>(a, P.save + plane * SV_HS, tile, lane, z2);
            store_native<4>(P.dz + plane * DZ_S1, tile, lane, z2);
            mm<8, 8>(acc, z2, reinterpret_cast<const bf16_t *>(lds + TA_WS1T), S128, lane);
            float gd = 0.0f;
            if (ok && P.g_den) gd = P.density[m] > 0.0f ? round_bf16(P.g_den[m]) : 0.0f;
            zero_acc<1>(v);
            if (h == 0) v[0][0] = gd;
            pack_frags<1>(v, z1, false);
            store_native<1>(P.dz + plane * DZ_D, tile, lane, z1);
            const float *wd = reinterpret_cast<const float *>(lds + TA_WD);
#pragma unroll
            for (int blk = 0; blk < 8; ++blk)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[blk][q] += round_bf16(wd[32 * blk + rho(q, h)]) * gd;
        }
        pack_frags<8>(acc, hin, false);                                  // dz of lout = d feats
        store_native<8>(P.dz + plane * (8 * DH), tile, lane, hin);
#pragma unroll 1
        for (int l = 8; l >= 1; --l) {
            __syncthreads();
            stage(lds, P.blob + b_layer(l), SZ_T);
            __syncthreads();
            zero_acc<8>(acc);
            mm<8, 16>(acc, hin, reinterpret_cast<const bf16_t *>(lds), S256, lane);
            mask_frags<8>(acc, P.save + plane * sv_h(l - 1), tile, lane, hin);
            store_native<8>(P.dz + plane * ((l - 1) * DH), tile, lane, hin);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- backward: weight gradients
struct WgUnit {
    const bf16_t *dz, *a;
    float *slab, *dW, *db;
    int dz_nblk, a_nblk, a_blk0, n_cb, n_out, ld, col0, ncols;
};
constexpr int MAX_UNITS = 32;
struct WgUnits {
    WgUnit u[MAX_UNITS];
};
__global__ __launch_bounds__(DEEP_WG) void deep_wgrad_kernel(WgUnits U, int64_t ntile, int n_split) {
    __shared__ __attribute__((aligned(16))) bf16_t zT[DH * WT];
    __shared__ __attribute__((aligned(16))) bf16_t aT[128 * WT];
    const WgUnit u = U.u[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t npair = (ntile + 1) / 2, per = (npair + n_split - 1) / n_split;
    const int64_t p0 = (int64_t)blockIdx.x * per, p1 = min(npair, p0 + per);
    const int rows_pad = u.dz_nblk * 32;
    f32x16 acc[4];
    zero_acc<4>(acc);
    float bsum = 0.0f;
    for (int64_t p = p0; p < p1; ++p) {
        __syncthreads();
        stage_transposed<DEEP_WG>(zT, u.dz, u.dz_nblk, 0, u.dz_nblk, p, ntile);
        stage_transposed<DEEP_WG>(aT, u.a, u.a_nblk, u.a_blk0, u.n_cb, p, ntile);
        __syncthreads();
        if (wave < u.dz_nblk) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 A = *reinterpret_cast<const bf16x8 *>(zT + (32 * wave + r) * WT + 16 * ks + 8 * h);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
                    if (cb < u.n_cb) {
                        const bf16x8 B = *reinterpret_cast<const bf16x8 *>(aT + (32 * cb + r) * WT + 16 * ks + 8 * h);
                        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, acc[cb], 0, 0, 0);
                    }
            }
        }
        if (u.db && (int)threadIdx.x < rows_pad) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bf16x8 v = *reinterpret_cast<const bf16x8 *>(zT + threadIdx.x * WT + 8 * j);
#pragma unroll
                for (int i = 0; i < 8; ++i) bsum += (float)v[i];
            }
        }
    }
    float *S = u.slab + (int64_t)blockIdx.x * rows_pad * 128;
    if (wave < u.dz_nblk) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
            if (cb < u.n_cb) {
#pragma unroll
                for (int q = 0; q < 16; ++q) S[(32 * wave + rho(q, h)) * 128 + 32 * cb + r] = acc[cb][q];
            }
    }
    if (u.db && (int)threadIdx.x < rows_pad) (u.slab + (int64_t)n_split * rows_pad * 128)[(int64_t)blockIdx.x * rows_pad + threadIdx.x] = bsum;
}

__global__ void deep_wgrad_finish_kernel(WgUnits U, int n_split) {
    const WgUnit u = U.u[blockIdx.y];
    const int rows_pad = u.dz_nblk * 32, idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= rows_pad * 128) return;
    const int row = idx >> 7, col = idx & 127;
    if (row < u.n_out && col < u.ncols) {
        float s = 0.0f;
        for (int k = 0; k < n_split; ++k) s += u.slab[(int64_t)k * rows_pad * 128 + idx];
        u.dW[(int64_t)row * u.ld + u.col0 + col] = s;
    }
    if (u.db && idx < u.n_out) {
        const float *B = u.slab + (int64_t)n_split * rows_pad * 128;
        float s = 0.0f;
        for (int k = 0; k < n_split; ++k) s += B[(int64_t)k * rows_pad + idx];
        u.db[idx] = s;
    }
}

// -------------------------------------------------------------------------------------------------------------------------------- host
int64_t tiles_padded(int64_t M) { return (M + 255) / 256 * 8; }
int split_of(int64_t M) {
    const int64_t npair = ((M + 31) / 32 + 1) / 2;
    return (int)std::max<int64_t>(1, std::min<int64_t>(MAX_SPLIT, npair));
}
// in-dims of the 14 Linears for C classes
void linear_shape(int i, int C, int *n_out, int *n_in) {
    static const int in[14] = {63, 256, 256, 256, 256, 319, 256, 256, 256, 256, 319, 128, 256, 128};
    static const int out[14] = {256, 256, 256, 256, 256, 256, 256, 256, 256, 1, 128, 3, 128, 0};
    *n_in = in[i];
    *n_out = i == 13 ? C : out[i];
}

struct Unit {
    int dz_col, dz_nblk, a_col, a_nblk, w, wcol0, nvalid, bias;
};
// (dz plane, input plane, Linear, first weight column, columns) of every weight-gradient product
const Unit kJobs[] = {
    {0, 8, SV_E, 2, 0, 0, 63, 1},
    {1 * DH, 8, sv_h(0), 8, 1, 0, 256, 1}, {2 * DH, 8, sv_h(1), 8, 2, 0, 256, 1}, {3 * DH, 8, sv_h(2), 8, 3, 0, 256, 1}, {4 * DH, 8, sv_h(3), 8, 4, 0, 256, 1},
    {5 * DH, 8, SV_E, 2, 5, 0, 63, 1}, {5 * DH, 8, sv_h(4), 8, 5, 63, 256, 0},
    {6 * DH, 8, sv_h(5), 8, 6, 0, 256, 1}, {7 * DH, 8, sv_h(6), 8, 7, 0, 256, 1}, {8 * DH, 8, sv_h(7), 8, 8, 0, 256, 1},
    {DZ_D, 1, sv_h(8), 8, 9, 0, 256, 1},
    {DZ_C1, 4, sv_h(8), 8, 10, 0, 256, 1}, {DZ_C1, 4, SV_V, 2, 10, 256, 63, 0}, {DZ_C2, 1, SV_HC, 4, 11, 0, 128, 1},
    {DZ_S1, 4, sv_h(8), 8, 12, 0, 256, 1}, {DZ_S2, 1, SV_HS, 4, 13, 0, 128, 1},
};
constexpr int N_JOBS = sizeof(kJobs) / sizeof(kJobs[0]);

int64_t slab_floats(int n_split) {
    int64_t total = 0;
    for (int j = 0; j < N_JOBS; ++j) {
        const int chunks = (kJobs[j].a_nblk + 3) / 4;
        total += (int64_t)chunks * n_split * (kJobs[j].dz_nblk * 32) * 129;
    }
    return total;
}

int check_common(const pag_deep_mlp_args *a, int64_t M, const char *name) {
    PAG_CHECK_ARG(a != nullptr, "%s: NULL args", name);
    PAG_CHECK_ARG(M >= 0, "%s: M %lld < 0", name, (long long)M);
    PAG_CHECK_ARG(pag_deep_mlp_supported(a->hidden, a->num_classes), "%s: hidden %d / num_classes %d not supported by the fused path (hidden 256, 1..16 classes)",
                  name, a->hidden, a->num_classes);
    PAG_CHECK_ARG(a->channels > 0 && a->channels < 8, "%s: channels mask %d", name, a->channels);
    return PAG_OK;
}

void add_pack(PackJobs &J, int &n, int64_t dst, const void *W, int rows_pad, int stride, int n_out, int ld, int col0, int ncols, int mode) {
    PackJob &p = J.j[n++];
    p.dst = dst;
    p.W = static_cast<const float *>(W);
    p.rows_pad = rows_pad, p.stride = stride, p.n_out = n_out, p.ld = ld, p.col0 = col0, p.ncols = ncols, p.mode = mode;
}

}  // namespace

extern "C" int pag_deep_mlp_supported(int hidden, int num_classes) { return hidden == 256 && num_classes >= 1 && num_classes <= 16; }

extern "C" int64_t pag_deep_mlp_workspace_bytes(int64_t M, int hidden, int num_classes, int mode) {
    if (M < 0 || mode < 0 || mode > 2 || !pag_deep_mlp_supported(hidden, num_classes)) {
        pag_set_error("pag_deep_mlp_workspace_bytes: M %lld, hidden %d, num_classes %d, mode %d", (long long)M, hidden, num_classes, mode);
        return -1;
    }
    const int64_t samples = tiles_padded(M) * 32;
    if (mode == 0) return align256(F_TOTAL);
    if (mode == 1) return align256(F_TOTAL) + align256(samples * SV_TOTAL * 2);
    return align256(B_TOTAL) + align256(samples * DZ_TOTAL * 2) + align256(slab_floats(split_of(M)) * 4);
}

extern "C" int pag_deep_mlp_fwd(const pag_deep_mlp_args *a, int64_t M, void *stream) {
    if (int rc = check_common(a, M, "pag_deep_mlp_fwd")) return rc;
    PAG_CHECK_ARG(!a->save || a->channels == 7, "pag_deep_mlp_fwd: save = 1 needs all three channels (mask %d)", a->channels);
    if (M == 0) return PAG_OK;
    const int64_t need = pag_deep_mlp_workspace_bytes(M, a->hidden, a->num_classes, a->save ? 1 : 0);
    PAG_CHECK_ARG(a->workspace != nullptr && ((uintptr_t)a->workspace & 255) == 0, "pag_deep_mlp_fwd: NULL or unaligned workspace");
    PAG_CHECK_ARG(a->workspace_bytes >= need, "pag_deep_mlp_fwd: workspace %lld bytes < %lld", (long long)a->workspace_bytes, (long long)need);
    PAG_CHECK_ARG(a->coords != nullptr, "pag_deep_mlp_fwd: NULL coords");
    PAG_CHECK_ARG(!(a->channels & PAG_DEEP_RGB) || (a->ray_d != nullptr && a->rgb != nullptr), "pag_deep_mlp_fwd: NULL ray_d / rgb");
    PAG_CHECK_ARG(!(a->channels & PAG_DEEP_DENSITY) || a->density != nullptr, "pag_deep_mlp_fwd: NULL density");
    PAG_CHECK_ARG(!(a->channels & PAG_DEEP_SEMANTICS) || a->semantics != nullptr, "pag_deep_mlp_fwd: NULL semantics");
    for (int i = 0; i < 14; ++i) PAG_CHECK_ARG(a->W[i] != nullptr && a->b[i] != nullptr, "pag_deep_mlp_fwd: NULL weight / bias %d", i);
    const int C = a->num_classes;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *blob = static_cast<char *>(a->workspace);
    PackJobs J;
    int n = 0;
    add_pack(J, n, 0, a->W[0], DH, S64, 256, 63, 0, 63, 0);
    add_pack(J, n, DH * S64 * 2, a->b[0], DH, 0, 256, 0, 0, 0, 2);
    for (int l = 1; l <= 8; ++l) {
        const int ld = l == 5 ? 319 : 256;
        add_pack(J, n, f_layer(l), a->W[l], DH, S256, 256, ld, l == 5 ? 63 : 0, 256, 0);
        add_pack(J, n, f_layer(l) + DH * S256 * 2, a->b[l], DH, 0, 256, 0, 0, 0, 2);
    }
    add_pack(J, n, F_L5E, a->W[5], DH, S64, 256, 319, 0, 63, 0);
    add_pack(J, n, F_HA + HA_WD, a->W[9], 32, S256, 1, 256, 0, 256, 0);
    add_pack(J, n, F_HA + HA_BD, a->b[9], 32, 0, 1, 0, 0, 0, 2);
    add_pack(J, n, F_HA + HA_WS1, a->W[12], DHH, S256, 128, 256, 0, 256, 0);
    add_pack(J, n, F_HA + HA_BS1, a->b[12], DHH, 0, 128, 0, 0, 0, 2);
    add_pack(J, n, F_HA + HA_WS2, a->W[13], 32, S128, C, 128, 0, 128, 0);
    add_pack(J, n, F_HA + HA_BS2, a->b[13], 32, 0, C, 0, 0, 0, 2);
    add_pack(J, n, F_HB + HB_WC1F, a->W[10], DHH, S256, 128, 319, 0, 256, 0);
    add_pack(J, n, F_HB + HB_BC1, a->b[10], DHH, 0, 128, 0, 0, 0, 2);
    add_pack(J, n, F_HB + HB_WC1V, a->W[10], DHH, S64, 128, 319, 256, 63, 0);
    add_pack(J, n, F_HB + HB_WC2, a->W[11], 32, S128, 3, 128, 0, 128, 0);
    add_pack(J, n, F_HB + HB_BC2, a->b[11], 32, 0, 3, 0, 0, 0, 2);
    hipLaunchKernelGGL(deep_pack_kernel, dim3(16, n), dim3(256), 0, st, J, blob);
    PAG_CHECK_LAUNCH("deep_pack_kernel");
    DeepFwdParams P;
    P.coords = static_cast<const float *>(a->coords), P.ray_d = static_cast<const float *>(a->ray_d);
    P.M = M, P.ntile = tiles_padded(M), P.C = C, P.channels = a->channels, P.blob = blob;
    P.density = static_cast<float *>(a->density), P.rgb = static_cast<float *>(a->rgb), P.sem = static_cast<float *>(a->semantics);
    P.save = a->save ? reinterpret_cast<bf16_t *>(blob + align256(F_TOTAL)) : nullptr;
    const int grid = (int)std::min<int64_t>(P.ntile / 8, NUM_CU);
    hipLaunchKernelGGL(deep_fwd_kernel, dim3(grid), dim3(DEEP_WG), 0, st, P);
    PAG_CHECK_LAUNCH("deep_fwd_kernel");
    return PAG_OK;
}

extern "C" int pag_deep_mlp_bwd(const pag_deep_mlp_args *a, int64_t M, void *stream) {
    if (int rc = check_common(a, M, "pag_deep_mlp_bwd")) return rc;
    if (M == 0) return PAG_OK;
    const int C = a->num_classes;
    const int64_t need_f = pag_deep_mlp_workspace_bytes(M, a->hidden, C, 1), need_b = pag_deep_mlp_workspace_bytes(M, a->hidden, C, 2);
    PAG_CHECK_ARG(a->workspace != nullptr && ((uintptr_t)a->workspace & 255) == 0 && a->bwd_workspace != nullptr && ((uintptr_t)a->bwd_workspace & 255) == 0,
                  "pag_deep_mlp_bwd: NULL or unaligned workspace");
    PAG_CHECK_ARG(a->workspace_bytes >= need_f, "pag_deep_mlp_bwd: forward workspace %lld bytes < %lld", (long long)a->workspace_bytes, (long long)need_f);
    PAG_CHECK_ARG(a->bwd_workspace_bytes >= need_b, "pag_deep_mlp_bwd: workspace %lld bytes < %lld", (long long)a->bwd_workspace_bytes, (long long)need_b);
    PAG_CHECK_ARG(a->density != nullptr && a->rgb != nullptr, "pag_deep_mlp_bwd: NULL density / rgb (the forward's outputs)");
    for (int i = 0; i < 14; ++i)
        PAG_CHECK_ARG(a->W[i] != nullptr && a->dW[i] != nullptr && a->db[i] != nullptr, "pag_deep_mlp_bwd: NULL weight / gradient buffer %d", i);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *blob = static_cast<char *>(a->bwd_workspace);
    PackJobs J;
    int n = 0;
    add_pack(J, n, B_TB + TB_WC2T, a->W[11], DHH, S16, 3, 128, 0, 128, 1);
    add_pack(J, n, B_TB + TB_WC1T, a->W[10], DH, S128, 128, 319, 0, 256, 1);
    add_pack(J, n, B_TA + TA_WS2T, a->W[13], DHH, S16, C, 128, 0, 128, 1);
    add_pack(J, n, B_TA + TA_WS1T, a->W[12], DH, S128, 128, 256, 0, 256, 1);
    add_pack(J, n, B_TA + TA_WD, a->W[9], DH, 0, 256, 0, 0, 0, 2);
    for (int l = 1; l <= 8; ++l) add_pack(J, n, b_layer(l), a->W[l], DH, S256, 256, l == 5 ? 319 : 256, l == 5 ? 63 : 0, 256, 1);
    hipLaunchKernelGGL(deep_pack_kernel, dim3(16, n), dim3(256), 0, st, J, blob);
    PAG_CHECK_LAUNCH("deep_pack_kernel");
    const int64_t ntile_pad = tiles_padded(M), plane = ntile_pad * 32;
    const bf16_t *save = reinterpret_cast<const bf16_t *>(static_cast<const char *>(a->workspace) + align256(F_TOTAL));
    bf16_t *dz = reinterpret_cast<bf16_t *>(blob + align256(B_TOTAL));
    float *slabs = reinterpret_cast<float *>(blob + align256(B_TOTAL) + align256(plane * DZ_TOTAL * 2));
    DeepBwdParams P;
    P.M = M, P.ntile = ntile_pad, P.C = C, P.blob = blob;
    P.g_den = static_cast<const float *>(a->g_density), P.g_rgb = static_cast<const float *>(a->g_rgb), P.g_sem = static_cast<const float *>(a->g_semantics);
    P.density = static_cast<const float *>(a->density), P.rgb = static_cast<const float *>(a->rgb);
    P.save = save, P.dz = dz;
    hipLaunchKernelGGL(deep_bwd_kernel, dim3((int)std::min<int64_t>(ntile_pad / 8, NUM_CU)), dim3(DEEP_WG), 0, st, P);
    PAG_CHECK_LAUNCH("deep_bwd_kernel");
    const int n_split = split_of(M);
    WgUnits U;
    int nu = 0, max_rows = 0;
    float *slab = slabs;
    for (int j = 0; j < N_JOBS; ++j) {
        const Unit &k = kJobs[j];
        int n_out, n_in;
        linear_shape(k.w, C, &n_out, &n_in);
        for (int cb0 = 0; cb0 < k.a_nblk; cb0 += 4) {
            WgUnit &u = U.u[nu++];
            u.dz = dz + plane * k.dz_col, u.a = save + plane * k.a_col;
            u.slab = slab, u.dW = static_cast<float *>(a->dW[k.w]), u.db = (k.bias && cb0 == 0) ? static_cast<float *>(a->db[k.w]) : nullptr;
            u.dz_nblk = k.dz_nblk, u.a_nblk = k.a_nblk, u.a_blk0 = cb0, u.n_cb = std::min(4, k.a_nblk - cb0);
            u.n_out = n_out, u.ld = n_in, u.col0 = k.wcol0 + cb0 * 32, u.ncols = std::max(0, std::min(128, k.nvalid - cb0 * 32));
            slab += (int64_t)n_split * (k.dz_nblk * 32) * 129;
            max_rows = std::max(max_rows, k.dz_nblk * 32);
        }
    }
    const int64_t ntile = (M + 31) / 32;
    hipLaunchKernelGGL(deep_wgrad_kernel, dim3(n_split, nu), dim3(DEEP_WG), 0, st, U, ntile, n_split);
    PAG_CHECK_LAUNCH("deep_wgrad_kernel");
    hipLaunchKernelGGL(deep_wgrad_finish_kernel, dim3(max_rows * 128 / 256, nu), dim3(256), 0, st, U, n_split);
    PAG_CHECK_LAUNCH("deep_wgrad_finish_kernel");
    return PAG_OK;
}
