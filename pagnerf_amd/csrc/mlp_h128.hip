// 128-wide decoders for gfx950: one wisp BasicDecoder (pc_nerf/panoptic_nef.py:114-164 with hidden_dim / inst_hidden_dim = 128 - the other half of
// main_hp_tunning.py's grid and config_parser.py's default) per call: 1 - 3 Linear + ReLU layers of width 128, then lout (out_dim <= 224) with no
// activation, sigmoid or softmax.  The 64-wide family (mlp.hip) is untouched; none of its cross-decoder fusions exists here.
//
// The transposed-MFMA scheme of mlp.hip / mlp_deep.hip: H^T[neurons x samples] = W[out x in] . X^T[in x samples] with v_mfma_f32_32x32x16_bf16, the sample
// on the lane, so a layer's accumulator blocks - after bias / ReLU and conversion to bf16 - ARE the next layer's B operand; the weights' input index is
// staged with bits 2 and 3 swapped (swap23) so that the hardware's k order matches the accumulator's row order.  At width 128 a wave holds 4 accumulator
// blocks (64 VGPRs) and 8 B fragments (32 VGPRs) per 32-sample tile.
//   * one workgroup = 8 waves x 32 samples = 256 samples per batch; at most one workgroup per CU, grid-striding over its batches.
//   * EVERY layer's image stays in LDS for the whole launch (mlp_h128_lds.h: at most 148 KiB for 3 hidden layers + a 224-row output layer), rows padded by
//     16 B so that the ds_read_b128 of an A fragment is conflict-free.  A workgroup converts, permutes and pads the f32 nn.Linear weights itself while
//     staging (they come from L2): no packed copy, so an inference forward needs no workspace at all.
//   * the layer-0 input (XCD8 bf16 [8][M][8], strided [M,k1] bf16 / f32, optionally followed by per-ray f32 rows x2[x2_index[m]]) is read straight into
//     B fragments: a fragment half is 4 consecutive input positions = one 8-byte (bf16) or 16-byte (f32) load.
// Training: the forward keeps the layer-0 input and every hidden layer's post-ReLU output (bf16, "native" layout, mlp_native.h); h128_bwd_kernel runs the data
// gradients through the chain on the transposed weights, writes every layer's dz (bf16) and d x1 in the input's form; h128_wgrad_kernel forms
// dz^T . input per (layer, slice of the samples) into slabs and h128_wgrad_finish_kernel adds the slices in a fixed order: no atomics, two runs give the
// same bits.  Every sample offset is 64-bit.
// The tile helpers (mm, init_bias, pack_frags, mask_frags, store_native, stage_transposed) are mlp_native.h's, shared with mlp_deep.hip.
#include "mlp_native.h"
#include "mlp_h128_lds.h"

namespace {
using namespace pagmlp128;

constexpr int H128_WG = 512;
constexpr int H128_BATCH = 256;         // samples per workgroup batch
constexpr float LOG2E = 1.44269504088896340736f;
// sample slices of a weight-gradient unit (2 - 4 units per launch: 256 - 512 workgroups).  A constant: which tile pairs a slice adds, and in which order
// the slices are added, must not depend on M (h128_wgrad_kernel)
constexpr int N_SPLIT = 128;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// how the layer-0 input is addressed (forward: x1 / x2; backward: dx1)
struct InForm {
    int xcd8, bf16, k1, levels, feats, k2p, in_dim;
};
// input position -> column of W_0 (XCD8: the staged position's feature column), or -1 when the position carries nothing
__device__ __forceinline__ int in_col(const InForm &f, int pos) {
    const int c = f.xcd8 ? grp_col(pos, f.levels, f.feats) : pos;
    return (c >= 0 && c < f.in_dim) ? c : -1;
}

// ------------------------------------------------------------------------------------------------------------------------- weight images
// dst [rows_pad][stride] bf16 = W [n_out][ld] with the input index permuted; a wave per row, a lane per column.  first: layer 0 (input positions)
__device__ __forceinline__ void stage_w(bf16_t *dst, const float *W, int rows_pad, int stride, int n_out, int ld, bool first, const InForm &f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = wave; row < rows_pad; row += H128_WG / 64)
        for (int c = lane; c < stride; c += 64) {
            const int k = swap23(c);
            const int col = first ? (k < K0 ? in_col(f, k) : -1) : (k < ld ? k : -1);
            dst[row * stride + c] = (bf16_t)((row < n_out && col >= 0) ? W[(int64_t)row * ld + col] : 0.0f);
        }
}
// transposed: dst [rows_pad = inputs][stride] = W^T, the OUTPUT index permuted; a wave per image column (= one row of W, read along its
// length: coalesced), a lane per image row
__device__ __forceinline__ void stage_wt(bf16_t *dst, const float *W, int rows_pad, int stride, int n_out, int ld, bool first, const InForm &f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < stride; c += H128_WG / 64) {
        const int k = swap23(c);
        for (int row = lane; row < rows_pad; row += 64) {
            const int col = first ? in_col(f, row) : (row < ld ? row : -1);
            dst[row * stride + c] = (bf16_t)((k < n_out && col >= 0) ? W[(int64_t)k * ld + col] : 0.0f);
        }
    }
}
// a[i] without a run-time index into the kernel's argument block
__device__ __forceinline__ const float *pick(const float *const *a, int i) { return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3]; }
__device__ __forceinline__ void stage_bias(float *dst, const float *b, int rows_pad, int n_out, float pad) {
    for (int i = threadIdx.x; i < rows_pad; i += H128_WG) dst[i] = i < n_out ? b[i] : pad;
}

// ------------------------------------------------------------------------------------------------------------------------- shared pieces
__device__ __forceinline__ bf16x4 cvt4(const f32x4 v) {
    bf16x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (bf16_t)v[i];
    return r;
}
// the other half-wave's value (rows 4h .. of every 8 are on lane r + 32 h)
__device__ __forceinline__ float other_half(float v) { return __shfl_xor(v, 32); }

// saved planes (columns before the plane, per sample): the layer-0 input (64 positions), h_0 .. h_(n_hidden-1)
__host__ __device__ constexpr int sv_h(int l) { return K0 + l * WH; }
// dz planes: dz_0 .. dz_(n_hidden-1), then the output layer's (ob * 32 columns)
__host__ __device__ constexpr int dz_col(int l) { return l * WH; }

// ------------------------------------------------------------------------------------------------------------------------------- forward
struct FwdParams {
    InForm in;
    const void *x1;
    const float *x2;
    const int32_t *x2_index;
    int n_hidden, out_dim, out_act, out_bf16;
    const float *W[MAX_HIDDEN + 1], *b[MAX_HIDDEN + 1];
    void *out;
    bf16_t *save;                // NULL, or the planes' base
    int64_t M, ntile;            // ntile: 32-sample tiles, a multiple of 8
};

// input positions c0 .. c0 + 3 (c0 % 4 == 0) of sample m
__device__ __forceinline__ bf16x4 load_in4(const FwdParams &P, int64_t m, int64_t x2row, int c0) {
    const InForm &f = P.in;
    if (f.xcd8) return reinterpret_cast<const bf16x4 *>(P.x1)[((int64_t)(c0 >> 3) * P.M + m) * 2 + ((c0 >> 2) & 1)];
    if (c0 < f.k1) {
        if (f.bf16) return *reinterpret_cast<const bf16x4 *>(static_cast<const bf16_t *>(P.x1) + m * f.k1 + c0);
        return cvt4(*reinterpret_cast<const f32x4 *>(static_cast<const float *>(P.x1) + m * f.k1 + c0));
    }
    if (c0 < f.k1 + f.k2p) return cvt4(*reinterpret_cast<const f32x4 *>(P.x2 + x2row * f.k2p + (c0 - f.k1)));
    return zero4();
}

// ACT is a template parameter: with a run-time activation the compiler keeps the logits AND both activations' results of all 16 NBO registers live
template <int NBO, int ACT>
__global__ __launch_bounds__(H128_WG) void h128_fwd_kernel(FwdParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const FwdLds L(P.n_hidden, NBO);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
#pragma unroll 1
    for (int l = 0; l <= P.n_hidden; ++l) {      // one copy of the staging code: layer 0, the hidden layers, the output layer
        const bool first = l == 0, last = l == P.n_hidden;
        stage_w(lds_at<bf16_t>(smem, first ? L.W0 : last ? L.WL : L.hidden_image(l)), pick(P.W, l), last ? NBO * 32 : WH, first ? S64 : S128,
                last ? P.out_dim : WH, first ? P.in.in_dim : WH, first, P.in);
        // a softmax's padding rows get the bias -inf (zero weights: logit -inf, probability 0 without a row test)
        stage_bias(lds_at<float>(smem, last ? L.bL : L.b + l * WH * 4), pick(P.b, l), last ? NBO * 32 : WH, last ? P.out_dim : WH,
                   last && ACT == PAG_ACT_SOFTMAX ? -INFINITY : 0.0f);
    }
    // bit masks of this lane's 32 input elements (fragment s, element j: position 16 s + 8 (j >> 2) + 4 h + (j & 3)): all ones where the position
    // carries a value - what lies in padding positions and in columns >= in_dim is never multiplied
    u32x4 live[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int p = 16 * s + 8 * (d >> 1) + 4 * h + 2 * (d & 1);
            live[s][d] = (in_col(P.in, p) >= 0 ? 0xffffu : 0u) | (in_col(P.in, p + 1) >= 0 ? 0xffff0000u : 0u);
        }
    __syncthreads();
    const int64_t nbatch = P.ntile / 8, plane = P.ntile * 32;
    for (int64_t batch = blockIdx.x; batch < nbatch; batch += gridDim.x) {
        // the images in LDS do not change, but their reads stay inside the loop (hoisted, a layer's A fragments would live in registers)
        asm volatile("" ::: "memory");
        int lim = P.out_dim - 4 * h;          // output column 32 blk + 8 g + 4 h + i exists when 32 blk + 8 g + i < lim
        asm volatile("" : "+v"(lim));
        const int64_t tile = batch * 8 + wave, m = tile * 32 + r;
        const bool ok = m < P.M;
        const int64_t mc = ok ? m : P.M - 1;
        const int64_t x2row = P.x2 ? P.x2_index[mc] : 0;
        bf16x8 x[4], hin[8];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bf16x4 lo = load_in4(P, mc, x2row, 16 * s + 4 * h), hi = load_in4(P, mc, x2row, 16 * s + 8 + 4 * h);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[s][i] = lo[i];
                x[s][4 + i] = hi[i];
            }
            x[s] = __builtin_bit_cast(bf16x8, __builtin_bit_cast(u32x4, x[s]) & live[s]);
        }
        if (P.save) store_native<2>(P.save, tile, lane, x);
        {
            f32x16 acc[4];
            init_bias<4>(acc, lds_at<float>(smem, L.b), h);
            mm<4, 4>(acc, x, lds_at<bf16_t>(smem, L.W0), S64, lane);
            pack_frags<4>(acc, hin, true);
            if (P.save) store_native<4>(P.save + plane * sv_h(0), tile, lane, hin);
#pragma unroll 1
            for (int l = 1; l < P.n_hidden; ++l) {
                init_bias<4>(acc, lds_at<float>(smem, L.b) + l * WH, h);
                mm<4, 8>(acc, hin, lds_at<bf16_t>(smem, L.hidden_image(l)), S128, lane);
                pack_frags<4>(acc, hin, true);
                if (P.save) store_native<4>(P.save + plane * sv_h(l), tile, lane, hin);
            }
        }
        f32x16 o[NBO];
        init_bias<NBO>(o, lds_at<float>(smem, L.bL), h);
        mm<NBO, 8, (NBO > 4)>(o, hin, lds_at<bf16_t>(smem, L.WL), S128, lane);
        // the hardware exp2 / rcp (~1 ulp), as the 64-wide epilogues: an accurate expf() and a true division per element do not fit the registers at 7 blocks
        if (ACT == PAG_ACT_SIGMOID) {
#pragma unroll
            for (int blk = 0; blk < NBO; ++blk)
#pragma unroll
                for (int q = 0; q < 16; ++q) o[blk][q] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * o[blk][q]));
        } else if (ACT == PAG_ACT_SOFTMAX) {
            float mx = -INFINITY;
#pragma unroll
            for (int blk = 0; blk < NBO; ++blk)
#pragma unroll
                for (int q = 0; q < 16; ++q) mx = fmaxf(mx, o[blk][q]);
            const float mxs = fmaxf(mx, other_half(mx)) * LOG2E;
            float sum = 0.0f;
#pragma unroll
            for (int blk = 0; blk < NBO; ++blk)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    o[blk][q] = __builtin_amdgcn_exp2f(fmaf(o[blk][q], LOG2E, -mxs));
                    sum += o[blk][q];
                }
            sum += other_half(sum);
            const float inv = 1.0f / sum;
#pragma unroll
            for (int blk = 0; blk < NBO; ++blk)
#pragma unroll
                for (int q = 0; q < 16; ++q) o[blk][q] *= inv;
        }
        if (ok) {
            const bool vec = (P.out_dim & 3) == 0;
            // one base address per sample; the column is a constant offset
            bf16_t *const ob = static_cast<bf16_t *>(P.out) + m * P.out_dim + 4 * h;
            float *const of = static_cast<float *>(P.out) + m * P.out_dim + 4 * h;
#pragma unroll
            for (int blk = 0; blk < NBO; ++blk)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int cl = 32 * blk + 8 * g;
                    if (cl >= lim) continue;
                    f32x4 v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = o[blk][4 * g + i];
                    if (vec) {
                        if (P.out_bf16) *reinterpret_cast<bf16x4 *>(ob + cl) = cvt4(v);
                        else *reinterpret_cast<f32x4 *>(of + cl) = v;
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (cl + i < lim) {
                                if (P.out_bf16) ob[cl + i] = (bf16_t)v[i];
                                else of[cl + i] = v[i];
                            }
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ backward: data gradients
struct BwdParams {
    InForm in;                   // the form of dx1 (bf16: dx1's dtype)
    const void *grad_out, *out;
    int n_hidden, out_dim, out_act, out_bf16, accumulate;
    const float *W[MAX_HIDDEN + 1];
    const bf16_t *save;
    bf16_t *dz;
    void *dx1;
    int64_t M, ntile;
};

// 4 values of an [M, out_dim] row at element `at`; vec: one aligned load, else element by element while cl + i < lim
__device__ __forceinline__ f32x4 load_out4(const void *p, int bf16, int64_t at, int cl, int lim, bool vec) {
    f32x4 v;
    if (vec) {
        if (bf16) {
            const bf16x4 t = *reinterpret_cast<const bf16x4 *>(static_cast<const bf16_t *>(p) + at);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (float)t[i];
        } else {
            v = *reinterpret_cast<const f32x4 *>(static_cast<const float *>(p) + at);
        }
        return v;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = cl + i < lim ? (bf16 ? (float)static_cast<const bf16_t *>(p)[at + i] : static_cast<const float *>(p)[at + i]) : 0.0f;
    return v;
}

template <int NBO>
__global__ __launch_bounds__(H128_WG) void h128_bwd_kernel(BwdParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const BwdLds L(P.n_hidden, NBO);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
#pragma unroll 1
    for (int l = P.dx1 ? 0 : 1; l <= P.n_hidden; ++l) {
        const bool first = l == 0, last = l == P.n_hidden;
        stage_wt(lds_at<bf16_t>(smem, first ? L.W0t : last ? L.WLt : L.hidden_image(l)), pick(P.W, l), first ? K0 : WH, last ? L.rsl : S128,
                 last ? P.out_dim : WH, first ? P.in.in_dim : WH, first, P.in);
    }
    __syncthreads();
    const int64_t nbatch = P.ntile / 8, plane = P.ntile * 32;
    const bool vec = (P.out_dim & 3) == 0;
    for (int64_t batch = blockIdx.x; batch < nbatch; batch += gridDim.x) {
        asm volatile("" ::: "memory");        // as in the forward: the images' reads stay inside the loop
        const int64_t tile = batch * 8 + wave, m = tile * 32 + r;
        const bool ok = m < P.M;
        int lim = ok ? P.out_dim - 4 * h : 0;          // output column 32 blk + 8 g + 4 h + i of this sample exists when 32 blk + 8 g + i < lim
        asm volatile("" : "+v"(lim));
        bf16x8 hin[8];
        f32x16 acc[4];
        {   // the output layer: dz = d loss / d (pre-activation); samples past M get zeros, which is all the weight gradients see of them
            f32x16 v[NBO];
            bf16x8 zo[2 * NBO];
            zero_acc<NBO>(v);
            float dot = 0.0f;
            const int64_t row = m * P.out_dim + 4 * h;      // one base address per sample; the column is a constant offset
#pragma unroll
            for (int blk = 0; blk < NBO; ++blk)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int cl = 32 * blk + 8 * g;
                    if (cl >= lim) continue;
                    const int64_t at = row + cl;
                    const f32x4 go = load_out4(P.grad_out, P.out_bf16, at, cl, lim, vec);
                    if (P.out_act == PAG_ACT_NONE) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[blk][4 * g + i] = go[i];
                    } else {
                        const f32x4 y = load_out4(P.out, P.out_bf16, at, cl, lim, vec);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            dot += go[i] * y[i];
                            v[blk][4 * g + i] = P.out_act == PAG_ACT_SIGMOID ? go[i] * y[i] * (1.0f - y[i]) : go[i];
                        }
                    }
                }
            if (P.out_act == PAG_ACT_SOFTMAX) {      // dz = y (g - sum g y): the saved probabilities once more
                dot += other_half(dot);
#pragma unroll
                for (int blk = 0; blk < NBO; ++blk)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int cl = 32 * blk + 8 * g;
                        if (cl >= lim) continue;
                        const f32x4 y = load_out4(P.out, P.out_bf16, row + cl, cl, lim, vec);
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[blk][4 * g + i] = y[i] * (v[blk][4 * g + i] - dot);
                    }
            }
            pack_frags<NBO>(v, zo, false);
            store_native<NBO>(P.dz + plane * dz_col(P.n_hidden), tile, lane, zo);
            zero_acc<4>(acc);
            mm<4, 2 * NBO>(acc, zo, lds_at<bf16_t>(smem, L.WLt), L.rsl, lane);
        }
        mask_frags<4>(acc, P.save + plane * sv_h(P.n_hidden - 1), tile, lane, hin);
        store_native<4>(P.dz + plane * dz_col(P.n_hidden - 1), tile, lane, hin);
#pragma unroll 1
        for (int l = P.n_hidden - 1; l >= 1; --l) {
            zero_acc<4>(acc);
            mm<4, 8>(acc, hin, lds_at<bf16_t>(smem, L.hidden_image(l)), S128, lane);
            mask_frags<4>(acc, P.save + plane * sv_h(l - 1), tile, lane, hin);
            store_native<4>(P.dz + plane * dz_col(l - 1), tile, lane, hin);
        }
        if (P.dx1) {      // d x1 = W_0^T dz_0 at the 64 input positions; positions that carry nothing have zero weights
            // the product runs on the WHOLE wave (a lane also holds a row of the weight block: no MFMA or fragment load under a per-sample branch)
            f32x16 d[2];
            zero_acc<2>(d);
            mm<2, 8>(d, hin, lds_at<bf16_t>(smem, L.W0t), S128, lane);
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (!ok) continue;
                    const int p0 = 32 * blk + 8 * g + 4 * h;
                    f32x4 v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = d[blk][4 * g + i];
                    if (P.in.xcd8) {
                        bf16x4 *dst = reinterpret_cast<bf16x4 *>(P.dx1) + ((int64_t)(p0 >> 3) * P.M + m) * 2 + h;
                        if (P.accumulate) {
                            const bf16x4 old = *dst;
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[i] += (float)old[i];
                        }
                        *dst = cvt4(v);
                    } else if (p0 < P.in.k1) {
                        if (P.in.bf16) *reinterpret_cast<bf16x4 *>(static_cast<bf16_t *>(P.dx1) + m * P.in.k1 + p0) = cvt4(v);
                        else *reinterpret_cast<f32x4 *>(static_cast<float *>(P.dx1) + m * P.in.k1 + p0) = v;
                    }
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- backward: weight gradients
struct WgUnit {
    const bf16_t *dz, *a;        // native planes: dz_nblk column blocks (rows of dW), a_nblk column blocks (columns of dW)
    float *slab, *dW, *db;
    int dz_nblk, a_nblk, n_out, ld, first;
};
struct WgUnits {
    WgUnit u[MAX_HIDDEN + 1];
    InForm in;
};

// slab [n_split][rows_pad][128] f32 partial dW, then [n_split][rows_pad] partial db; workgroup (x, y) = slice x of the samples of unit y
__global__ __launch_bounds__(H128_WG) void h128_wgrad_kernel(WgUnits U, int64_t ntile, int n_split) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WgradLds L;
    bf16_t *zT = lds_at<bf16_t>(smem, L.zT), *aT = lds_at<bf16_t>(smem, L.aT);
    const WgUnit u = U.u[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    // slice x takes the tile pairs x, x + n_split, ...: which pairs a slice adds and in which order does not depend on M, so a batch padded with
    // samples of zero gradient (the captured step's static buffers) gives the bits of the unpadded one
    const int64_t npair = (ntile + 1) / 2;
    const int rows_pad = u.dz_nblk * 32;
    f32x16 acc[4];
    zero_acc<4>(acc);
    float bsum = 0.0f;
    for (int64_t p = blockIdx.x; p < npair; p += n_split) {
        __syncthreads();
        stage_transposed<H128_WG>(zT, u.dz, u.dz_nblk, 0, u.dz_nblk, p, ntile);
        stage_transposed<H128_WG>(aT, u.a, u.a_nblk, 0, u.a_nblk, p, ntile);
        __syncthreads();
        if (wave < u.dz_nblk) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 A = *reinterpret_cast<const bf16x8 *>(zT + (32 * wave + r) * WT + 16 * ks + 8 * h);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
                    if (cb < u.a_nblk) {
                        const bf16x8 B = *reinterpret_cast<const bf16x8 *>(aT + (32 * cb + r) * WT + 16 * ks + 8 * h);
                        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, acc[cb], 0, 0, 0);
                    }
            }
        }
        if ((int)threadIdx.x < rows_pad) {
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
            if (cb < u.a_nblk) {
#pragma unroll
                for (int q = 0; q < 16; ++q) S[(32 * wave + rho(q, h)) * 128 + 32 * cb + r] = acc[cb][q];
            }
    }
    if ((int)threadIdx.x < rows_pad) (u.slab + (int64_t)n_split * rows_pad * 128)[(int64_t)blockIdx.x * rows_pad + threadIdx.x] = bsum;
}

// adds the slices in their order; layer 0: slab column = input position -> column of W_0 (XCD8: level * F + f, as pag_mlp_wgrad_finish)
__global__ void h128_wgrad_finish_kernel(WgUnits U, int n_split) {
    const WgUnit u = U.u[blockIdx.y];
    const int rows_pad = u.dz_nblk * 32, idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx >= rows_pad * 128) return;
    const int row = idx >> 7, pos = idx & 127;
    const int col = u.first ? (pos < K0 ? in_col(U.in, pos) : -1) : (pos < u.ld ? pos : -1);
    if (row < u.n_out && col >= 0) {
        float s = 0.0f;
        for (int k = 0; k < n_split; ++k) s += u.slab[(int64_t)k * rows_pad * 128 + idx];
        u.dW[(int64_t)row * u.ld + col] = s;
    }
    if (idx < u.n_out) {
        const float *B = u.slab + (int64_t)n_split * rows_pad * 128;
        float s = 0.0f;
        for (int k = 0; k < n_split; ++k) s += B[(int64_t)k * rows_pad + idx];
        u.db[idx] = s;
    }
}

// -------------------------------------------------------------------------------------------------------------------------------- host
int64_t tiles_padded(int64_t M) { return (M + H128_BATCH - 1) / H128_BATCH * 8; }
// 32-row blocks the kernels are built for: 1, 4 or 7
int out_blocks(int out_dim) { return out_dim <= 32 ? 1 : out_dim <= 128 ? 4 : OB_MAX; }
int64_t slab_floats(int n_hidden, int ob, int n_split) { return (int64_t)n_split * (n_hidden * WH + ob * 32) * 129; }
int64_t save_bytes(int64_t M, int n_hidden) { return align256(tiles_padded(M) * 32 * sv_h(n_hidden) * 2); }
int64_t dz_bytes(int64_t M, int n_hidden, int ob) { return align256(tiles_padded(M) * 32 * (dz_col(n_hidden) + ob * 32) * 2); }

int check_shape(const char *name, int n_hidden, int hidden, int in_dim, int out_dim, int64_t M) {
    PAG_CHECK_ARG(M >= 0 && M <= PAG_MLP128_MAX_M, "%s: M %lld outside [0, %lld]", name, (long long)M, (long long)PAG_MLP128_MAX_M);
    PAG_CHECK_ARG(hidden == WH, "%s: hidden %d (this family is 128 wide)", name, hidden);
    PAG_CHECK_ARG(n_hidden >= 1 && n_hidden <= MAX_HIDDEN, "%s: n_hidden %d outside [1, 3]", name, n_hidden);
    PAG_CHECK_ARG(in_dim >= 1 && in_dim <= K0, "%s: in_dim %d outside [1, 64]", name, in_dim);
    PAG_CHECK_ARG(out_dim >= 1 && out_dim <= OB_MAX * 32, "%s: out_dim %d outside [1, 224]", name, out_dim);
    return PAG_OK;
}

int check_form(const char *name, int layout, int dtype, int k1, int levels, int feats, int k2p, int in_dim, InForm *f) {
    PAG_CHECK_ARG(layout == PAG_LAYOUT_STRIDED || layout == PAG_LAYOUT_XCD8, "%s: x1_layout %d", name, layout);
    PAG_CHECK_ARG(dtype == PAG_BF16 || (dtype == PAG_F32 && layout == PAG_LAYOUT_STRIDED), "%s: x1_dtype %d (bf16; f32 for a strided x1)", name, dtype);
    PAG_CHECK_ARG(k2p >= 0 && k2p % 8 == 0, "%s: k2p %d is not a multiple of 8", name, k2p);
    if (layout == PAG_LAYOUT_XCD8) {
        PAG_CHECK_ARG(k1 == K0, "%s: k1 %d with the XCD8 layout (64)", name, k1);
        PAG_CHECK_ARG(feats >= 1 && levels >= 1 && (feats & (feats - 1)) == 0 && feats <= 8 && levels * feats <= K0 && levels * feats == in_dim && k2p == 0,
                      "%s: x1_levels %d x x1_feats %d does not give in_dim %d (XCD8: feats 1 / 2 / 4 / 8, at most 64 features, no x2)", name, levels, feats, in_dim);
    } else {
        PAG_CHECK_ARG(k1 >= 8 && k1 % 8 == 0 && k1 <= K0, "%s: k1 %d is not a multiple of 8 in [8, 64]", name, k1);
        PAG_CHECK_ARG(k1 + k2p <= K0 && in_dim <= k1 + k2p, "%s: in_dim %d / k1 %d + k2p %d (in_dim <= k1 + k2p <= 64)", name, in_dim, k1, k2p);
    }
    f->xcd8 = layout == PAG_LAYOUT_XCD8, f->bf16 = dtype == PAG_BF16, f->k1 = k1, f->levels = levels, f->feats = feats, f->k2p = k2p, f->in_dim = in_dim;
    return PAG_OK;
}

template <int NBO, int ACT>
void launch_fwd_act(const FwdParams &P, hipStream_t st) {
    const int lds = FwdLds(P.n_hidden, NBO).bytes;
    raise_lds_limit<h128_fwd_kernel<NBO, ACT>>(LDS_MAX_BYTES);
    hipLaunchKernelGGL((h128_fwd_kernel<NBO, ACT>), dim3((unsigned)std::min<int64_t>(P.ntile / 8, NUM_CU)), dim3(H128_WG), lds, st, P);
}
template <int NBO>
void launch_fwd(const FwdParams &P, hipStream_t st) {
    switch (P.out_act) {
        case PAG_ACT_SIGMOID: launch_fwd_act<NBO, PAG_ACT_SIGMOID>(P, st); break;
        case PAG_ACT_SOFTMAX: launch_fwd_act<NBO, PAG_ACT_SOFTMAX>(P, st); break;
        default: launch_fwd_act<NBO, PAG_ACT_NONE>(P, st); break;
    }
}
template <int NBO>
void launch_bwd(const BwdParams &P, hipStream_t st) {
    const int lds = BwdLds(P.n_hidden, NBO).bytes;
    raise_lds_limit<h128_bwd_kernel<NBO>>(LDS_MAX_BYTES);
    hipLaunchKernelGGL(h128_bwd_kernel<NBO>, dim3((unsigned)std::min<int64_t>(P.ntile / 8, NUM_CU)), dim3(H128_WG), lds, st, P);
}

}  // namespace

extern "C" int pag_mlp128_supported(int n_hidden, int hidden, int in_dim, int out_dim) {
    return hidden == WH && n_hidden >= 1 && n_hidden <= MAX_HIDDEN && in_dim >= 1 && in_dim <= K0 && out_dim >= 1 && out_dim <= OB_MAX * 32;
}

extern "C" int64_t pag_mlp128_workspace_bytes(int64_t M, int n_hidden, int out_dim, int mode) {
    if (M < 0 || M > PAG_MLP128_MAX_M || mode < 0 || mode > 2 || !pag_mlp128_supported(n_hidden, WH, 1, out_dim)) {
        pag_set_error("pag_mlp128_workspace_bytes: M %lld, n_hidden %d, out_dim %d, mode %d", (long long)M, n_hidden, out_dim, mode);
        return -1;
    }
    if (mode == 0 || M == 0) return 0;
    if (mode == 1) return save_bytes(M, n_hidden);
    const int ob = out_blocks(out_dim);
    return dz_bytes(M, n_hidden, ob) + align256(slab_floats(n_hidden, ob, N_SPLIT) * 4);
}

extern "C" int pag_mlp128_fwd(const pag_mlp128_fwd_args *a, int64_t M, void *stream) {
    PAG_CHECK_ARG(a != nullptr, "pag_mlp128_fwd: NULL args");
    if (int rc = check_shape("pag_mlp128_fwd", a->n_hidden, a->hidden, a->in_dim, a->out_dim, M)) return rc;
    FwdParams P;
    if (int rc = check_form("pag_mlp128_fwd", a->x1_layout, a->x1_dtype, a->k1, a->x1_levels, a->x1_feats, a->x2 ? a->k2p : 0, a->in_dim, &P.in)) return rc;
    PAG_CHECK_ARG(a->out_act >= PAG_ACT_NONE && a->out_act <= PAG_ACT_SOFTMAX, "pag_mlp128_fwd: out_act %d", a->out_act);
    PAG_CHECK_ARG(a->out_dtype == PAG_F32 || a->out_dtype == PAG_BF16, "pag_mlp128_fwd: out_dtype %d", a->out_dtype);
    if (M == 0) return PAG_OK;
    PAG_CHECK_ARG(a->x1 != nullptr, "pag_mlp128_fwd: NULL x1");
    PAG_CHECK_ARG(!a->x2 || a->x2_index != nullptr, "pag_mlp128_fwd: NULL x2_index with x2");
    PAG_CHECK_ARG(a->out != nullptr, "pag_mlp128_fwd: NULL out");
    for (int i = 0; i <= a->n_hidden; ++i) PAG_CHECK_ARG(a->W[i] != nullptr && a->b[i] != nullptr, "pag_mlp128_fwd: NULL W / b %d", i);
    if (a->workspace) {
        const int64_t need = save_bytes(M, a->n_hidden);
        PAG_CHECK_ARG(((uintptr_t)a->workspace & 255) == 0, "pag_mlp128_fwd: unaligned workspace");
        PAG_CHECK_ARG(a->workspace_bytes >= need, "pag_mlp128_fwd: workspace_bytes %lld < %lld", (long long)a->workspace_bytes, (long long)need);
    }
    P.x1 = a->x1, P.x2 = a->x2, P.x2_index = a->x2_index;
    P.n_hidden = a->n_hidden, P.out_dim = a->out_dim, P.out_act = a->out_act, P.out_bf16 = a->out_dtype == PAG_BF16;
    for (int i = 0; i <= a->n_hidden; ++i) P.W[i] = a->W[i], P.b[i] = a->b[i];
    P.out = a->out, P.save = static_cast<bf16_t *>(a->workspace), P.M = M, P.ntile = tiles_padded(M);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (out_blocks(a->out_dim)) {
        case 1: launch_fwd<1>(P, st); break;
        case 4: launch_fwd<4>(P, st); break;
        default: launch_fwd<OB_MAX>(P, st); break;
    }
    PAG_CHECK_LAUNCH("h128_fwd_kernel");
    return PAG_OK;
}

extern "C" int pag_mlp128_bwd(const pag_mlp128_bwd_args *a, int64_t M, void *stream) {
    PAG_CHECK_ARG(a != nullptr, "pag_mlp128_bwd: NULL args");
    if (int rc = check_shape("pag_mlp128_bwd", a->n_hidden, a->hidden, a->in_dim, a->out_dim, M)) return rc;
    BwdParams P;
    if (int rc = check_form("pag_mlp128_bwd", a->x1_layout, a->dx1 ? a->dx1_dtype : PAG_BF16, a->k1, a->x1_levels, a->x1_feats, a->k2p, a->in_dim, &P.in)) return rc;
    PAG_CHECK_ARG(a->out_act >= PAG_ACT_NONE && a->out_act <= PAG_ACT_SOFTMAX, "pag_mlp128_bwd: out_act %d", a->out_act);
    PAG_CHECK_ARG(a->out_dtype == PAG_F32 || a->out_dtype == PAG_BF16, "pag_mlp128_bwd: out_dtype %d", a->out_dtype);
    PAG_CHECK_ARG(!a->dx1_accumulate || (a->dx1 && a->x1_layout == PAG_LAYOUT_XCD8), "pag_mlp128_bwd: dx1_accumulate needs an XCD8 dx1");
    if (M == 0) return PAG_OK;
    PAG_CHECK_ARG(a->grad_out != nullptr, "pag_mlp128_bwd: NULL grad_out");
    PAG_CHECK_ARG(a->out_act == PAG_ACT_NONE || a->out != nullptr, "pag_mlp128_bwd: NULL out (the forward's output, needed for sigmoid / softmax)");
    for (int i = 0; i <= a->n_hidden; ++i)
        PAG_CHECK_ARG(a->W[i] != nullptr && a->dW[i] != nullptr && a->db[i] != nullptr, "pag_mlp128_bwd: NULL W / dW / db %d", i);
    const int ob = out_blocks(a->out_dim);
    const int64_t need_f = save_bytes(M, a->n_hidden), need_b = pag_mlp128_workspace_bytes(M, a->n_hidden, a->out_dim, 2);
    PAG_CHECK_ARG(a->workspace != nullptr && ((uintptr_t)a->workspace & 255) == 0, "pag_mlp128_bwd: NULL or unaligned workspace (the forward's)");
    PAG_CHECK_ARG(a->workspace_bytes >= need_f, "pag_mlp128_bwd: workspace_bytes %lld < %lld", (long long)a->workspace_bytes, (long long)need_f);
    PAG_CHECK_ARG(a->bwd_workspace != nullptr && ((uintptr_t)a->bwd_workspace & 255) == 0, "pag_mlp128_bwd: NULL or unaligned bwd_workspace");
    PAG_CHECK_ARG(a->bwd_workspace_bytes >= need_b, "pag_mlp128_bwd: bwd_workspace_bytes %lld < %lld", (long long)a->bwd_workspace_bytes, (long long)need_b);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ntile_pad = tiles_padded(M), plane = ntile_pad * 32;
    const bf16_t *save = static_cast<const bf16_t *>(a->workspace);
    bf16_t *dz = static_cast<bf16_t *>(a->bwd_workspace);
    P.grad_out = a->grad_out, P.out = a->out;
    P.n_hidden = a->n_hidden, P.out_dim = a->out_dim, P.out_act = a->out_act, P.out_bf16 = a->out_dtype == PAG_BF16, P.accumulate = a->dx1_accumulate;
    for (int i = 0; i <= a->n_hidden; ++i) P.W[i] = a->W[i];
    P.save = save, P.dz = dz, P.dx1 = a->dx1, P.M = M, P.ntile = ntile_pad;
    switch (ob) {
        case 1: launch_bwd<1>(P, st); break;
        case 4: launch_bwd<4>(P, st); break;
        default: launch_bwd<OB_MAX>(P, st); break;
    }
    PAG_CHECK_LAUNCH("h128_bwd_kernel");
    const int n_split = N_SPLIT;
    WgUnits U;
    U.in = P.in;
    float *slab = reinterpret_cast<float *>(static_cast<char *>(a->bwd_workspace) + dz_bytes(M, a->n_hidden, ob));
    int max_rows = 0;
    for (int l = 0; l <= a->n_hidden; ++l) {
        WgUnit &u = U.u[l];
        u.dz = dz + plane * dz_col(l), u.a = save + plane * (l == 0 ? 0 : sv_h(l - 1));
        u.dz_nblk = l == a->n_hidden ? ob : 4, u.a_nblk = l == 0 ? 2 : 4;
        u.n_out = l == a->n_hidden ? a->out_dim : WH, u.ld = l == 0 ? a->in_dim : WH, u.first = l == 0;
        u.slab = slab, u.dW = a->dW[l], u.db = a->db[l];
        slab += (int64_t)n_split * (u.dz_nblk * 32) * 129;
        max_rows = std::max(max_rows, u.dz_nblk * 32);
    }
    hipLaunchKernelGGL(h128_wgrad_kernel, dim3(n_split, a->n_hidden + 1), dim3(H128_WG), WgradLds{}.bytes, st, U, (M + 31) / 32, n_split);
    PAG_CHECK_LAUNCH("h128_wgrad_kernel");
    hipLaunchKernelGGL(h128_wgrad_finish_kernel, dim3(max_rows * 128 / 256, a->n_hidden + 1), dim3(256), 0, st, U, n_split);
    PAG_CHECK_LAUNCH("h128_wgrad_finish_kernel");
    return PAG_OK;
}
