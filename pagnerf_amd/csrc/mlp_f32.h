// The FP32 parity path of mlp.hip (only mlp.hip includes this; PAG_MLP_FP32 in the scheme at the top of mlp.hip): mlp_fwd_f32, which
// pag_mlp_fwd launches itself, and mlp_bwd_f32 with its launcher.
#pragma once
#include "mlp_common.h"
#include "mlp_lds.h"
#include "mlp_params.h"

namespace {

// ------------------------------------------------------------------------------------ FP32 parity path
// One lane per sample.  Weights transposed in LDS ([k][j]) so the 64 outputs of a layer are 16
// broadcast ds_read_b128; the per-sample activation column lives in LDS ([k][lane]).

__device__ void stage_f32_t(float *dst, const float *W, int n_out, int n_in, int out_pad) {   // dst[k][out_pad]
    for (int e = threadIdx.x; e < n_in * out_pad; e += blockDim.x) {
        int k = e / out_pad, j = e - k * out_pad;
        dst[e] = j < n_out ? W[(int64_t)j * n_in + k] : 0.0f;
    }
}

template <typename X1T, typename OutT>
__global__ __launch_bounds__(PT) void mlp_fwd_f32(FwdParams p, int n_layers) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr F32Lds L(64);
    float *xs = lds_at<float>(smem, L.cols);              // [64][PT] activation columns
    float *wt = lds_at<float>(smem, L.wt);                // current layer's W^T [k][out_pad]
    const int t = threadIdx.x;
    const int64_t m = (int64_t)blockIdx.x * PT + t;
    const bool live = m < p.M;
    const int64_t mc = live ? m : p.M - 1;
    const X1T *x1 = reinterpret_cast<const X1T *>(p.x1);
    OutT *out = reinterpret_cast<OutT *>(p.out);
    // input column
    const int32_t ray = p.x2 ? p.x2_index[mc] : 0;
    for (int k = 0; k < p.in_dim; ++k)
        xs[k * PT + t] = k < p.k1 ? pag_ld(x1 + mc * p.k1 + k) : p.x2[(int64_t)ray * p.k2p + (k - p.k1)];
    int n_in = p.in_dim;
    for (int l = 0; l < n_layers; ++l) {
        const bool last = l == n_layers - 1;
        const int n_out = last ? p.out_dim : HID;
        const int chunks = (n_out + 63) / 64;
        for (int c = 0; c < chunks; ++c) {
            __syncthreads();
            const int rows = min(64, n_out - 64 * c);
            stage_f32_t(wt, p.W[l] + (int64_t)64 * c * n_in, rows, n_in, 64);
            __syncthreads();
            float acc[64];
#pragma unroll
            for (int j = 0; j < 64; ++j) acc[j] = j < rows ? p.b[l][64 * c + j] : 0.0f;
            for (int k = 0; k < n_in; ++k) {
                const float xk = xs[k * PT + t];
                const f32x4 *wrow = reinterpret_cast<const f32x4 *>(wt + k * 64);
#pragma unroll
                for (int j4 = 0; j4 < 16; ++j4) {
                    f32x4 w = wrow[j4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[4 * j4 + j] = fmaf(w[j], xk, acc[4 * j4 + j]);
                }
            }
            if (!last) {
                __syncthreads();   // everyone finished reading xs of the previous layer
#pragma unroll
                for (int j = 0; j < 64; ++j) {
                    float v = fmaxf(acc[j], 0.0f);
                    xs[j * PT + t] = v;
                    if (p.hsave[l] && live) reinterpret_cast<float *>(p.hsave[l])[m * HID + j] = v;
                }
            } else if (live) {
#pragma unroll
                for (int j = 0; j < 64; ++j)
                    if (j < rows) {
                        float v = acc[j];
                        if (p.act == PAG_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
                        pag_st(out + m * p.out_dim + 64 * c + j, v);
                    }
            }
        }
        n_in = HID;
    }
    if (p.act == PAG_ACT_SOFTMAX && live) {   // second pass over this sample's logits
        OutT *row = out + m * p.out_dim;
        float mx = -INFINITY;
        for (int j = 0; j < p.out_dim; ++j) mx = fmaxf(mx, pag_ld(row + j));
        float sum = 0.0f;
        for (int j = 0; j < p.out_dim; ++j) sum += expf(pag_ld(row + j) - mx);
        for (int j = 0; j < p.out_dim; ++j) pag_st(row + j, expf(pag_ld(row + j) - mx) / sum);
    }
}

__device__ void stage_f32_n(float *dst, const float *W, int row0, int rows, int n_in) {   // dst[j][64] = W[row0+j][0:n_in]
    for (int e = threadIdx.x; e < rows * 64; e += blockDim.x) {
        int j = e / 64, k = e - j * 64;
        dst[e] = k < n_in ? W[(int64_t)(row0 + j) * n_in + k] : 0.0f;
    }
}

template <typename OutT, typename DxT>
__global__ __launch_bounds__(PT) void mlp_bwd_f32(BwdParams p, int n_layers) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr F32Lds L(224);
    float *zs = lds_at<float>(smem, L.cols);              // [224][PT] dz column of the current layer
    float *wt = lds_at<float>(smem, L.wt);                // [64 rows j][64 k]
    const int t = threadIdx.x;
    const int64_t m = (int64_t)blockIdx.x * PT + t;
    const bool live = m < p.M;
    const int64_t mc = live ? m : p.M - 1;
    const OutT *y = reinterpret_cast<const OutT *>(p.out) + mc * p.out_dim;
    const OutT *g = reinterpret_cast<const OutT *>(p.grad_out) + mc * p.out_dim;
    float dot = 0.0f;
    if (p.act == PAG_ACT_SOFTMAX)
        for (int j = 0; j < p.out_dim; ++j) dot += pag_ld(g + j) * pag_ld(y + j);
    for (int j = 0; j < p.out_dim; ++j) {
        float v = pag_ld(g + j);
        if (p.act == PAG_ACT_SIGMOID) {
            float yy = pag_ld(y + j);
            v = v * yy * (1.0f - yy);
        } else if (p.act == PAG_ACT_SOFTMAX) {
            v = pag_ld(y + j) * (v - dot);
        }
        v = live ? v : 0.0f;
        zs[j * PT + t] = v;
        if (live) reinterpret_cast<float *>(p.dz[n_layers - 1])[m * p.out_dim + j] = v;
    }
    int n_out = p.out_dim;
    for (int l = n_layers - 1; l >= 0; --l) {
        const int n_in = l == 0 ? p.in_dim : HID;
        if (l == 0 && !p.dx1) break;
        float acc[64];
#pragma unroll
        for (int k = 0; k < 64; ++k) acc[k] = 0.0f;
        const int chunks = (n_out + 63) / 64;
        for (int c = 0; c < chunks; ++c) {
            __syncthreads();
            const int rows = min(64, n_out - 64 * c);
            stage_f32_n(wt, p.W[l], 64 * c, rows, n_in);
            __syncthreads();
            for (int j = 0; j < rows; ++j) {
                const float zj = zs[(64 * c + j) * PT + t];
                const f32x4 *wrow = reinterpret_cast<const f32x4 *>(wt + j * 64);
#pragma unroll
                for (int k4 = 0; k4 < 16; ++k4) {
                    f32x4 w = wrow[k4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[4 * k4 + k] = fmaf(w[k], zj, acc[4 * k4 + k]);
                }
            }
        }
        __syncthreads();
        if (l > 0) {
            const float *hv = reinterpret_cast<const float *>(p.hsave[l - 1]) + mc * HID;
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                float v = (live && hv[k] > 0.0f) ? acc[k] : 0.0f;
                zs[k * PT + t] = v;
                if (live) reinterpret_cast<float *>(p.dz[l - 1])[m * HID + k] = v;
            }
            n_out = HID;
        } else if (live) {
            DxT *dx = reinterpret_cast<DxT *>(p.dx1) + m * p.k1;
#pragma unroll
            for (int k = 0; k < 64; ++k)
                if (k < p.k1) pag_st(dx + k, acc[k]);
        }
    }
}

template <typename OutT, typename DxT>
void launch_bwd_f32(const BwdParams &p, int n_layers, hipStream_t st) {
    constexpr F32Lds L(224);      // 128 KiB
    raise_lds_limit<mlp_bwd_f32<OutT, DxT>>(L.bytes);
    hipLaunchKernelGGL((mlp_bwd_f32<OutT, DxT>), dim3((unsigned)((p.M + PT - 1) / PT)), dim3(PT), L.bytes, st, p, n_layers);
}

}  // namespace
