// Supervised-contrastive instance loss (loss/sup_contrastive.py::SupConLoss, pc_nerf/trainer.py:63-65,477-480,499-503) without the [n, n] matrices.
//
// The reference materialises per image about ten fp32 [n, n] tensors (logits, shifted logits, masks, exp, products and autograd's copies) and makes three
// host synchronisations (anchor count, boolean indexing, l.unique()).  Here the logits A_ij = f_i.f_j / T are recomputed tile by tile on the f32-input
// MFMA (exact fp32 products, k-ordered fmaf chains) and never leave registers; per anchor row only (m_i, Sum_{j!=i} exp(A_ij - m_i), cnt_i) are kept.  Nothing is read back to
// the host and no float atomics are used: every sum runs in a fixed order, so two runs are bitwise identical.
//
//   supcon_compact_kernel    one workgroup per image: the anchor rows in order (ballot + prefix), their labels, rank of every row (-1: not an anchor), the
//                            anchor count n and the skip flag (n == 0, or - with an anchor mask - min label == max label)
//   supcon_norm_kernel       one wave per slot q: F[q] = x[idx[q]] / max(||x||, 1e-12) zero-padded to Dp columns (slots q >= n: zeros), ||x|| kept;
//                            the loss of original row q is zeroed when it is not an anchor of a kept image
//   supcon_fwd_kernel        64 anchor rows per workgroup (16 per wave) against every 16*NT-column block of the anchors: S^T tile on
//                            v_mfma_f32_16x16x4_f32, then per row a running max m (j = i included, detached), Sum_{j!=i} exp(A - m), Sum of the
//                            positives' logits and their count; the row's loss goes to its original position
//   supcon_coef_kernel       c_i = g_i * (-T/T_base) / (cnt_i + 1e-16); rows that are not anchors of a kept image get a zero gradient row
//   supcon_bwd_kernel        the same tiles again; W_ij = dA_ij + dA_ji (A is symmetric, both halves from the saved row statistics) and
//                            df_i = (1/T) Sum_j W_ij f_j on the MFMA with W as the B operand straight from the accumulators; then the
//                            normalisation's chain rule dx = (df - f (f.df)) / ||x|| (df / 1e-12 where ||x|| <= 1e-12)
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SC_ROWS = 64;                // anchor rows per workgroup (4 waves x 16)
constexpr int SC_MAX_D = 512;
constexpr int SC_MAX_B = 65535;
constexpr int64_t SC_MAX_P = 1 << 24;

__host__ __device__ inline int sc_dpad(int D) { return (D + 15) / 16 * 16; }
__host__ __device__ inline int64_t sc_align(int64_t x) { return (x + 255) / 256 * 256; }

struct ScWs {
    float *F;                  // [B,P,Dp] normalised anchor rows, compacted
    float *norm, *m, *sum, *cnt, *coef;        // [B,P] per compacted slot (sum = Sum_{j != i} exp(A_ij - m_i))
    int64_t *lab;              // [B,P] compacted labels
    int32_t *idx, *rank;       // [B,P] slot -> original row, original row -> slot (-1: not an anchor)
    int32_t *n, *skip;         // [B]
};

__host__ inline int64_t sc_ws_bytes(int64_t B, int64_t P, int D) {
    return sc_align(B * P * sc_dpad(D) * 4) + 5 * sc_align(B * P * 4) + sc_align(B * P * 8) + 2 * sc_align(B * P * 4) + 2 * sc_align(B * 4);
}

__host__ inline ScWs sc_ws(void *base, int64_t B, int64_t P, int D) {
    unsigned char *p = reinterpret_cast<unsigned char *>(base);
    ScWs w;
    w.F = reinterpret_cast<float *>(p);      p += sc_align(B * P * sc_dpad(D) * 4);
    w.norm = reinterpret_cast<float *>(p);   p += sc_align(B * P * 4);
    w.m = reinterpret_cast<float *>(p);      p += sc_align(B * P * 4);
    w.sum = reinterpret_cast<float *>(p);    p += sc_align(B * P * 4);
    w.cnt = reinterpret_cast<float *>(p);    p += sc_align(B * P * 4);
    w.coef = reinterpret_cast<float *>(p);   p += sc_align(B * P * 4);
    w.lab = reinterpret_cast<int64_t *>(p);  p += sc_align(B * P * 8);
    w.idx = reinterpret_cast<int32_t *>(p);  p += sc_align(B * P * 4);
    w.rank = reinterpret_cast<int32_t *>(p); p += sc_align(B * P * 4);
    w.n = reinterpret_cast<int32_t *>(p);    p += sc_align(B * 4);
    w.skip = reinterpret_cast<int32_t *>(p);
    return w;
}

__device__ __forceinline__ float sc_ld(const void *x, int dtype, int64_t e) {
    return dtype == PAG_BF16 ? (float)reinterpret_cast<const bf16_t *>(x)[e] : reinterpret_cast<const float *>(x)[e];
}

__global__ __launch_bounds__(1024) void supcon_compact_kernel(const int64_t *__restrict__ labels, const uint8_t *__restrict__ mask, int64_t P, ScWs w) {
    __shared__ int32_t s_cnt[16];
    __shared__ long long s_min[16], s_max[16];
    __shared__ int32_t s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    if (tid == 0) s_base = 0;
    long long lo = 0x7fffffffffffffffll, hi = (long long)0x8000000000000000ull;
    __syncthreads();
    for (int64_t p0 = 0; p0 < P; p0 += 1024) {
        const int64_t p = p0 + tid;
        const bool a = p < P && (mask == nullptr || mask[b * P + p] != 0);
        const unsigned long long bal = __ballot(a);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int off = s_base, total = 0;
        for (int v = 0; v < 16; ++v) {
            off += v < wave ? s_cnt[v] : 0;
            total += s_cnt[v];
        }
        if (a) {
            const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
            const long long l = labels[b * P + p];
            w.idx[b * P + pos] = (int32_t)p;
            w.lab[b * P + pos] = l;
            w.rank[b * P + p] = pos;
            lo = l < lo ? l : lo;
            hi = l > hi ? l : hi;
        } else if (p < P) {
            w.rank[b * P + p] = -1;
        }
        __syncthreads();
        if (tid == 0) s_base += total;
        __syncthreads();
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o_lo = __shfl_xor(lo, d), o_hi = __shfl_xor(hi, d);
        lo = o_lo < lo ? o_lo : lo;
        hi = o_hi > hi ? o_hi : hi;
    }
    if (lane == 0) s_min[wave] = lo, s_max[wave] = hi;
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 16; ++v) {
            lo = s_min[v] < lo ? s_min[v] : lo;
            hi = s_max[v] > hi ? s_max[v] : hi;
        }
        const int n = s_base;
        w.n[b] = n;
        w.skip[b] = (n == 0 || (mask != nullptr && lo == hi)) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void supcon_norm_kernel(const void *__restrict__ x, int dtype, int64_t P, int D, int64_t image_stride, int64_t row_stride,
                                                          ScWs w, float *__restrict__ loss) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (q >= P) return;
    const int Dp = sc_dpad(D);
    const int n = w.n[b];
    if (lane == 0 && (w.skip[b] || w.rank[b * P + q] < 0)) loss[b * P + q] = 0.0f;
    float *f = w.F + (b * P + q) * Dp;
    if (q >= n) {
        for (int k = lane; k < Dp; k += 64) f[k] = 0.0f;
        return;
    }
    const int64_t row = b * image_stride + (int64_t)w.idx[b * P + q] * row_stride;
    float ss = 0.0f;
    for (int k = lane; k < D; k += 64) {
        const float v = sc_ld(x, dtype, row + k);
        ss = fmaf(v, v, ss);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) ss += __shfl_xor(ss, d);
    const float nrm = sqrtf(ss);
    const float den = fmaxf(nrm, 1e-12f);
    for (int k = lane; k < Dp; k += 64) f[k] = k < D ? sc_ld(x, dtype, row + k) / den : 0.0f;
    if (lane == 0) w.norm[b * P + q] = nrm;
}

// Column block c0 .. c0 + 16 NT of image b into LDS: F rows (stride Dp + 4 floats) and labels; rows past P are zero.
template <int NT>
__device__ __forceinline__ void sc_stage_cols(const ScWs &w, int64_t b, int64_t P, int Dp, int64_t c0, float *sF, long long *sLab) {
    const int tid = threadIdx.x;
    const int D4 = Dp / 4, stride = Dp + 4;
    for (int e = tid; e < 16 * NT * D4; e += 256) {
        const int r = e / D4, c = e - r * D4;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (c0 + r < P) v = *reinterpret_cast<const f32x4 *>(w.F + (b * P + c0 + r) * Dp + 4 * c);
        *reinterpret_cast<f32x4 *>(sF + r * stride + 4 * c) = v;
    }
    if (tid < 16 * NT) sLab[tid] = c0 + tid < P ? w.lab[b * P + c0 + tid] : 0;
}

// acc[t][r] = S[j][i], j = c0 + 16t + 4(lane>>4) + r, i = this wave's row i0 + (lane&15): A operand = column rows from LDS, B operand = the wave's own rows
// from the workspace.  Lane l feeds dimension 16g + 4(l>>4) + s in k-step s of group g - a permutation of the 16 dimensions of the group, the same for both
// operands.
template <int NT>
__device__ __forceinline__ void sc_scores(const float *__restrict__ fi, const float *sF, int Dp, f32x4 (&acc)[NT]) {
    const int lane = threadIdx.x & 63;
    const int stride = Dp + 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int g = 0; g < Dp / 16; ++g) {
        const int k = 16 * g + 4 * (lane >> 4);
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(fi + k);
        f32x4 av[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) av[t] = *reinterpret_cast<const f32x4 *>(sF + (16 * t + (lane & 15)) * stride + k);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][s], bv[s], acc[t], 0, 0, 0);
    }
}

__device__ __forceinline__ float sc_rescale(float m, float M) { return m == -INFINITY ? 0.0f : expf(m - M); }

template <int NT>
__global__ __launch_bounds__(256) void supcon_fwd_kernel(int64_t P, int D, float T, float Tb, float pw, float nw, ScWs w, float *__restrict__ loss) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.y, r0 = (int64_t)blockIdx.x * SC_ROWS;
    const int n = w.n[b];
    if (w.skip[b] || r0 >= n) return;
    const int Dp = sc_dpad(D);
    float *sF = smem;
    long long *sLab = reinterpret_cast<long long *>(smem + 16 * NT * (Dp + 4));
    const int64_t i = r0 + 16 * wave + (lane & 15);          // < P: P is a multiple of nothing, but r0 < n <= P and rows >= P read a zero row below
    const bool row_ok = i < n;
    const float *fi = w.F + (b * P + (row_ok ? i : 0)) * Dp;
    const long long li = row_ok ? w.lab[b * P + i] : 0;
    const float shift = 1.0f / T;                            // A_ii of a unit row: the positives' logits are summed relative to it (no cancellation)
    float m = -INFINITY, s = 0.0f, q = 0.0f, cnt = 0.0f;
    for (int64_t c0 = 0; c0 < n; c0 += 16 * NT) {
        __syncthreads();
        sc_stage_cols<NT>(w, b, P, Dp, c0, sF, sLab);
        __syncthreads();
        f32x4 acc[NT];
        sc_scores<NT>(fi, sF, Dp, acc);
        float a[NT][4];
        float bm = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t j = c0 + 16 * t + 4 * (lane >> 4) + r;
                a[t][r] = acc[t][r] / T;
                if (j < n) bm = fmaxf(bm, a[t][r]);
            }
        if (bm > m) {
            s *= sc_rescale(m, bm);
            m = bm;
        }
        float bs = 0.0f, bq = 0.0f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * t + 4 * (lane >> 4) + r;
                const int64_t j = c0 + jl;
                if (j < n && j != i) {
                    bs += expf(a[t][r] - m);
                    if (sLab[jl] == li) {
                        bq += a[t][r] - shift;
                        cnt += 1.0f;
                    }
                }
            }
        s += bs;
        q += bq;
    }
    // the four lanes of a row (lane bits 4, 5), in a fixed order
#pragma unroll
    for (int d = 16; d <= 32; d <<= 1) {
        const float om = __shfl_xor(m, d), os = __shfl_xor(s, d), oq = __shfl_xor(q, d), oc = __shfl_xor(cnt, d);
        const float M = fmaxf(m, om);
        const float lo = (lane & d) ? om : m, hi = (lane & d) ? m : om;          // same operand order in both lanes of the pair
        const float slo = (lane & d) ? os : s, shi = (lane & d) ? s : os;
        s = slo * sc_rescale(lo, M) + shi * sc_rescale(hi, M);
        q = (lane & d) ? oq + q : q + oq;
        cnt += oc;
        m = M;
    }
    if (row_ok && lane < 16) {
        const float lse = logf(s);
        // Sum_j M_ij log_prob_ij = pw (Sum_j M_ij A_ij - cnt m) - nw cnt LSE, with Sum_j M_ij A_ij = q + cnt / T
        const float num = pw * (q + cnt * (shift - m)) - (nw * cnt) * lse;
        const float li_loss = -(T / Tb) * (num / (cnt + 1e-16f));
        const int64_t e = b * P + i;
        w.m[e] = m;
        w.sum[e] = s;
        w.cnt[e] = cnt;
        loss[b * P + w.idx[e]] = li_loss;
    }
}

__global__ __launch_bounds__(256) void supcon_coef_kernel(int64_t P, int D, int dtype, float T, float Tb, ScWs w, const float *__restrict__ grad,
                                                          void *__restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (p >= P) return;
    const int q = w.rank[b * P + p];
    if (!w.skip[b] && q >= 0) {
        if (lane == 0) w.coef[b * P + q] = grad[b * P + p] * (-(T / Tb)) / (w.cnt[b * P + q] + 1e-16f);
        return;
    }
    for (int k = lane; k < D; k += 64) {
        if (dtype == PAG_BF16) reinterpret_cast<bf16_t *>(dx)[(b * P + p) * D + k] = (bf16_t)0.0f;
        else reinterpret_cast<float *>(dx)[(b * P + p) * D + k] = 0.0f;
    }
}

template <int NT, int QMAX>
__global__ __launch_bounds__(256) void supcon_bwd_kernel(int64_t P, int D, int dtype, float T, float pw, float nw, ScWs w, void *__restrict__ dx) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.y, r0 = (int64_t)blockIdx.x * SC_ROWS;
    const int n = w.n[b];
    if (w.skip[b] || r0 >= n) return;
    const int Dp = sc_dpad(D), nq = Dp / 16, stride = Dp + 4;
    float *sF = smem;
    long long *sLab = reinterpret_cast<long long *>(smem + 16 * NT * stride);
    float *sStat = reinterpret_cast<float *>(sLab + 16 * NT);                 // [4][16 NT]: m, sum, nw cnt, coef of the column block
    const int64_t i = r0 + 16 * wave + (lane & 15);
    const bool row_ok = i < n;
    const int64_t ei = b * P + (row_ok ? i : 0);
    const float *fi = w.F + ei * Dp;
    const long long li = row_ok ? w.lab[ei] : 0;
    const float mi = w.m[ei], si = w.sum[ei], ci = w.coef[ei], ncnti = nw * w.cnt[ei];
    f32x4 out[QMAX];
#pragma unroll
    for (int qq = 0; qq < QMAX; ++qq) out[qq] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t c0 = 0; c0 < n; c0 += 16 * NT) {
        __syncthreads();
        sc_stage_cols<NT>(w, b, P, Dp, c0, sF, sLab);
        if (threadIdx.x < 16 * NT) {
            const int64_t j = c0 + threadIdx.x, e = b * P + (j < P ? j : 0);
            sStat[threadIdx.x] = w.m[e];
            sStat[16 * NT + threadIdx.x] = w.sum[e];
            sStat[32 * NT + threadIdx.x] = nw * w.cnt[e];
            sStat[48 * NT + threadIdx.x] = j < n ? w.coef[e] : 0.0f;
        }
        __syncthreads();
        f32x4 acc[NT];
        sc_scores<NT>(fi, sF, Dp, acc);
        // W^T[j][i] = dA_ij + dA_ji, dA_ij = c_i (pw M_ij - nw cnt_i p_ij), p_ij = exp(A_ij - m_i) / Sum_{j != i} exp(A_ij - m_i) (the softmax's
        // own rounding: exp(A - m - LSE) would round the exponent at the magnitude of m + LSE)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * t + 4 * (lane >> 4) + r;
                const int64_t j = c0 + jl;
                float v = 0.0f;
                if (row_ok && j < n && j != i) {
                    const float a = acc[t][r] / T;
                    const float pos = sLab[jl] == li ? pw : 0.0f;
                    const float pij = expf(a - mi) / si, pji = expf(a - sStat[jl]) / sStat[16 * NT + jl];
                    v = ci * (pos - ncnti * pij) + sStat[48 * NT + jl] * (pos - sStat[32 * NT + jl] * pji);
                }
                acc[t][r] = v;
            }
        // out^T[kd][i] += Sum_j F[j][kd] W^T[j][i]: for fixed (t, r) lane l holds W^T[16t + 4(l>>4) + r][i], the B operand of k-step index l>>4.
        // Up to D = 256 the block's 16 NT terms are summed on their own and added to the running sum (fmaf chains of 16 NT, not of n)
        constexpr bool split = QMAX <= 16;
        f32x4 blk[split ? QMAX : 1];
#pragma unroll
        for (int qq = 0; qq < (split ? QMAX : 1); ++qq) blk[qq] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *arow = sF + (16 * t + 4 * (lane >> 4) + r) * stride + (lane & 15);
#pragma unroll
                for (int qq = 0; qq < QMAX; ++qq)
                    if (qq < nq) {
                        if constexpr (split) blk[qq] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[16 * qq], acc[t][r], blk[qq], 0, 0, 0);
                        else out[qq] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[16 * qq], acc[t][r], out[qq], 0, 0, 0);
                    }
            }
        if constexpr (split) {
#pragma unroll
            for (int qq = 0; qq < QMAX; ++qq)
                if (qq < nq) out[qq] += blk[qq];
        }
    }
    if (!row_ok) return;
    // lane holds df[i][16 qq + 4 (lane>>4) + rr]
    float dot = 0.0f;
#pragma unroll
    for (int qq = 0; qq < QMAX; ++qq)
        if (qq < nq) {
            const f32x4 f = *reinterpret_cast<const f32x4 *>(fi + 16 * qq + 4 * (lane >> 4));
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                out[qq][rr] = out[qq][rr] / T;
                dot = fmaf(f[rr], out[qq][rr], dot);
            }
        }
    dot += __shfl_xor(dot, 16);
    dot += __shfl_xor(dot, 32);
    const float nrm = w.norm[ei];
    const bool big = nrm > 1e-12f;
    const int64_t drow = (b * P + w.idx[ei]) * D;
#pragma unroll
    for (int qq = 0; qq < QMAX; ++qq)
        if (qq < nq) {
            const f32x4 f = *reinterpret_cast<const f32x4 *>(fi + 16 * qq + 4 * (lane >> 4));
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int k = 16 * qq + 4 * (lane >> 4) + rr;
                if (k < D) {
                    const float g = big ? (out[qq][rr] - f[rr] * dot) / nrm : out[qq][rr] / 1e-12f;
                    if (dtype == PAG_BF16) reinterpret_cast<bf16_t *>(dx)[drow + k] = (bf16_t)g;
                    else reinterpret_cast<float *>(dx)[drow + k] = g;
                }
            }
        }
}

inline int sc_nt(int D) { return sc_dpad(D) <= 256 ? 2 : 1; }
inline size_t sc_lds(int D, bool bwd) {
    const int nt = sc_nt(D);
    return (size_t)16 * nt * (sc_dpad(D) + 4) * 4 + 16 * nt * 8 + (bwd ? 4 * 16 * nt * 4 : 0);
}

}      // namespace

extern "C" int64_t pag_supcon_workspace_bytes(int B, int64_t P, int D) {
    return (B < 1 || P < 1 || D < 1 || D > SC_MAX_D) ? 0 : sc_ws_bytes(B, P, D);
}

extern "C" int pag_supcon_fwd(const void *features, int dtype, int B, int64_t P, int D, int64_t image_stride, int64_t row_stride, const int64_t *labels,
                              const uint8_t *anchor_mask, float temperature, float base_temperature, float pos_weight, float neg_weight, void *workspace,
                              int64_t workspace_bytes, float *loss, void *stream) {
    PAG_CHECK_ARG(B >= 1 && B <= SC_MAX_B && P >= 1 && P <= SC_MAX_P && D >= 1 && D <= SC_MAX_D && row_stride >= D && image_stride >= 0,
                  "pag_supcon_fwd: sizes (B %d, P %lld, D %d, row_stride %lld)", B, (long long)P, D, (long long)row_stride);
    PAG_CHECK_ARG(dtype == PAG_F32 || dtype == PAG_BF16, "pag_supcon_fwd: dtype %d (f32 or bf16)", dtype);
    PAG_CHECK_ARG(temperature > 0.0f && base_temperature > 0.0f, "pag_supcon_fwd: temperatures must be > 0");
    PAG_CHECK_ARG(features && labels && workspace && loss, "pag_supcon_fwd: NULL input/output");
    PAG_CHECK_ARG(workspace_bytes >= sc_ws_bytes(B, P, D), "pag_supcon_fwd: workspace %lld < %lld bytes", (long long)workspace_bytes,
                  (long long)sc_ws_bytes(B, P, D));
    hipStream_t st = (hipStream_t)stream;
    const ScWs w = sc_ws(workspace, B, P, D);
    const dim3 rows((unsigned)((P + 3) / 4), B), tiles((unsigned)((P + SC_ROWS - 1) / SC_ROWS), B);
    hipLaunchKernelGGL(supcon_compact_kernel, dim3(B), dim3(1024), 0, st, labels, anchor_mask, P, w);
    hipLaunchKernelGGL(supcon_norm_kernel, rows, dim3(256), 0, st, features, dtype, P, D, image_stride, row_stride, w, loss);
    if (sc_nt(D) == 2)
        hipLaunchKernelGGL(supcon_fwd_kernel<2>, tiles, dim3(256), sc_lds(D, false), st, P, D, temperature, base_temperature, pos_weight, neg_weight, w, loss);
    else
        hipLaunchKernelGGL(supcon_fwd_kernel<1>, tiles, dim3(256), sc_lds(D, false), st, P, D, temperature, base_temperature, pos_weight, neg_weight, w, loss);
    PAG_CHECK_LAUNCH("pag_supcon_fwd");
    return PAG_OK;
}

extern "C" int pag_supcon_bwd(int dtype, int B, int64_t P, int D, float temperature, float base_temperature, float pos_weight, float neg_weight,
                              void *workspace, int64_t workspace_bytes, const float *grad_loss, void *d_features, void *stream) {
    PAG_CHECK_ARG(B >= 1 && B <= SC_MAX_B && P >= 1 && P <= SC_MAX_P && D >= 1 && D <= SC_MAX_D, "pag_supcon_bwd: sizes (B %d, P %lld, D %d)", B, (long long)P, D);
    PAG_CHECK_ARG(dtype == PAG_F32 || dtype == PAG_BF16, "pag_supcon_bwd: dtype %d (f32 or bf16)", dtype);
    PAG_CHECK_ARG(temperature > 0.0f && base_temperature > 0.0f, "pag_supcon_bwd: temperatures must be > 0");
    PAG_CHECK_ARG(workspace && grad_loss && d_features, "pag_supcon_bwd: NULL input/output");
    PAG_CHECK_ARG(workspace_bytes >= sc_ws_bytes(B, P, D), "pag_supcon_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes,
                  (long long)sc_ws_bytes(B, P, D));
    hipStream_t st = (hipStream_t)stream;
    const ScWs w = sc_ws(workspace, B, P, D);
    const dim3 rows((unsigned)((P + 3) / 4), B), tiles((unsigned)((P + SC_ROWS - 1) / SC_ROWS), B);
    hipLaunchKernelGGL(supcon_coef_kernel, rows, dim3(256), 0, st, P, D, dtype, temperature, base_temperature, w, grad_loss, d_features);
    const int Dp = sc_dpad(D);
    const size_t lds = sc_lds(D, true);
    if (Dp <= 64)
        hipLaunchKernelGGL((supcon_bwd_kernel<2, 4>), tiles, dim3(256), lds, st, P, D, dtype, temperature, pos_weight, neg_weight, w, d_features);
    else if (Dp <= 128)
        hipLaunchKernelGGL((supcon_bwd_kernel<2, 8>), tiles, dim3(256), lds, st, P, D, dtype, temperature, pos_weight, neg_weight, w, d_features);
    else if (Dp <= 256)
        hipLaunchKernelGGL((supcon_bwd_kernel<2, 16>), tiles, dim3(256), lds, st, P, D, dtype, temperature, pos_weight, neg_weight, w, d_features);
    else
        hipLaunchKernelGGL((supcon_bwd_kernel<1, 32>), tiles, dim3(256), lds, st, P, D, dtype, temperature, pos_weight, neg_weight, w, d_features);
    PAG_CHECK_LAUNCH("pag_supcon_bwd");
    return PAG_OK;
}
