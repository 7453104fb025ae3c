// Decoder weight gradients as launches of their own (pag_mlp_wgrad*): mlp_wgrad_kernel forms per-workgroup slabs from the dz tensors mlp_bwd_mfma
// wrote; wgrad_finish_kernel, which sums them, stays in mlp.hip beside the fused backward kernels whose slabs it sums as well, and is reached
// through pagmlp::launch_wgrad_finish.
#include "mlp_common.h"
#include "mlp_lds.h"

namespace {

// ------------------------------------------------------------------------------- weight gradients
// dW[out][in] = sum_m dz[m][out] * a[m][in]  and  db[out] = sum_m dz[m][out]: a GEMM whose reduction
// runs over the M ~ 2e6 samples with both operands K-major in memory, which BLAS libraries handle
// badly (2.5 ms per layer measured).  Here each workgroup walks 64-sample chunks: the [64 x n_out] dz
// tile and the [64 x n_in] input tile are transposed into LDS (lane = sample, so the ds_write_b16
// stores are conflict-free), every wave owns up to 6 of the 32x32 (out-block, in-block) pairs and
// feeds them with ds_read_b128 fragments; an extra in-block whose B fragment is the constant
// "1 in column 0" yields db for free.  Partial sums are written as per-workgroup fp32 slabs
// [blocks][OB*32][96] (cols 0..63 = dW, col 64 = db) and summed by the caller - deterministic, no atomics.
struct WgradParams {
    const bf16_t *dz;
    int dz_cols, n_out;
    const void *a1;
    int k1;
    const float *a2;
    int k2p;
    const int32_t *a2_index;
    int n_in;
    float *slabs;
    int64_t M;
    int a1_grouped;        // a1 is bf16 [8][M][8] (PAG_LAYOUT_XCD8); slab columns are then staged positions
};
struct WgradBatch {
    WgradParams p[WG_MAX_BATCH];
};

template <typename A1T, int APW /* accumulator blocks per wave */, int NWV = 4 /* waves per workgroup */>
// narrow variant (APW 2, 4 waves): asking for 5 waves per SIMD keeps every accumulator in VGPRs (no AGPR copies) under 102
// registers.  Wide layers (up to 224 outputs = 21 block pairs): 8 waves x 3 pairs instead of 4 x 6 - 48 accumulator
// registers per wave leave room for the prefetch and for 4 waves per SIMD (the 4 x 6 form ran 2 waves per SIMD, no prefetch).
__global__ __launch_bounds__(NWV * 64, (APW == 2 ? 5 : (APW == 3 ? 4 : 1))) void mlp_wgrad_kernel(WgradBatch batch) {
    const WgradParams &p = batch.p[blockIdx.y];       // blockIdx.y = layer: the layers of one decoder share a launch
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int OB = (p.n_out + 31) / 32;
    const int IB = (p.n_in + 31) / 32;                 // 1 or 2
    const WgradLds L(OB, IB);
    bf16_t *Zt = lds_at<bf16_t>(smem, L.Zt);            // [OB*32][WG_RS]
    bf16_t *At = lds_at<bf16_t>(smem, L.At);            // [IB*32][WG_RS]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int npairs = OB * (IB + 1);
    f32x16 acc[APW];
#pragma unroll
    for (int i = 0; i < APW; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][q] = 0.0f;
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (bf16_t)(r == 0 ? 1.0f : 0.0f);
    const A1T *a1 = reinterpret_cast<const A1T *>(p.a1);
    const bool dz_vec = (p.dz_cols % 8) == 0 && (p.n_out % 8) == 0;
    const int64_t nchunks = (p.M + 63) / 64;
    // global -> register fetch of one 8-column piece of this lane's sample row (dz tile / input tile)
    auto fetch_z = [&](int64_t chunk, int cg) __attribute__((always_inline)) {
        const int64_t m = chunk * 64 + lane;
        const bool live = m < p.M;
        const int64_t mc = live ? m : p.M - 1;
        const int c0 = 8 * cg;
        bf16x8 v = zero8();
        if (live && c0 < p.n_out) {      // n_out <= dz_cols: dz may point at a band of columns of a wider row
            if (dz_vec) {
                v = load8(p.dz + mc * p.dz_cols + c0);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (c0 + j < p.n_out) v[j] = p.dz[mc * p.dz_cols + c0 + j];
            }
        }
        return v;
    };
    auto fetch_a = [&](int64_t chunk, int cg) __attribute__((always_inline)) {
        const int64_t m = chunk * 64 + lane;
        const bool live = m < p.M;
        const int64_t mc = live ? m : p.M - 1;
        const int c0 = 8 * cg;
        bf16x8 v = zero8();
        if (live && p.a1_grouped)
            v = load8(reinterpret_cast<const bf16_t *>(p.a1) + ((int64_t)cg * p.M + mc) * 8);
        else if (live && c0 < p.k1)
            v = load8(a1 + mc * p.k1 + c0);
        else if (live && p.a2 && c0 < p.k1 + p.k2p)
            v = load8(p.a2 + (int64_t)p.a2_index[mc] * p.k2p + (c0 - p.k1));
        return v;
    };
    // APW == 2 (<= 64 x 64 layers, 76 VGPRs): the next chunk's four 16-byte pieces are fetched into registers while the
    // current chunk goes through LDS and the MFMAs - the kernel sat waiting on memory 77 % of its wave cycles (SQ_WAIT_ANY)
    // with nothing in flight between the two barriers.  The wide variant has no registers to spare for this.
    constexpr bool PF = APW <= 3;
    constexpr int ZG = (NWV == 8) ? 4 : 2, AG = (NWV == 8) ? 1 : 2;      // 16-byte pieces per wave: dz (<= 224 / 64 cols), input (64 cols)
    bf16x8 pz[ZG], pa[AG];
    if constexpr (PF) {
#pragma unroll
        for (int i = 0; i < ZG; ++i) {
            const int cg = wave + NWV * i;
            pz[i] = (blockIdx.x < nchunks && cg < OB * 4) ? fetch_z(blockIdx.x, cg) : zero8();
        }
#pragma unroll
        for (int i = 0; i < AG; ++i) {
            const int cg = wave + NWV * i;
            pa[i] = (blockIdx.x < nchunks && cg < IB * 4) ? fetch_a(blockIdx.x, cg) : zero8();
        }
    }
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        // ---- dz tile, transposed: Zt[col][sample]
        if constexpr (PF) {
#pragma unroll
            for (int i = 0; i < ZG; ++i) {
                const int cg = wave + NWV * i, c0 = 8 * cg;
                if (cg < OB * 4) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) Zt[(c0 + j) * WG_RS + lane] = pz[i][j];
                }
            }
#pragma unroll
            for (int i = 0; i < AG; ++i) {
                const int cg = wave + NWV * i, c0 = 8 * cg;
                if (cg < IB * 4) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) At[(c0 + j) * WG_RS + lane] = (c0 + j < p.n_in) ? pa[i][j] : (bf16_t)0.0f;
                }
            }
        } else {
            for (int cg = wave; cg < OB * 4; cg += NWV) {
                const int c0 = 8 * cg;
                const bf16x8 v = fetch_z(chunk, cg);
#pragma unroll
                for (int j = 0; j < 8; ++j) Zt[(c0 + j) * WG_RS + lane] = v[j];
            }
            // ---- input tile, transposed: At[col][sample]
            for (int cg = wave; cg < IB * 4; cg += NWV) {
                const int c0 = 8 * cg;
                const bf16x8 v = fetch_a(chunk, cg);
#pragma unroll
                for (int j = 0; j < 8; ++j) At[(c0 + j) * WG_RS + lane] = (c0 + j < p.n_in) ? v[j] : (bf16_t)0.0f;
            }
        }
        __syncthreads();
        if constexpr (PF) {
            const int64_t next = chunk + gridDim.x;
            if (next < nchunks) {
#pragma unroll
                for (int i = 0; i < ZG; ++i) {
                    const int cg = wave + NWV * i;
                    if (cg < OB * 4) pz[i] = fetch_z(next, cg);
                }
#pragma unroll
                for (int i = 0; i < AG; ++i) {
                    const int cg = wave + NWV * i;
                    if (cg < IB * 4) pa[i] = fetch_a(next, cg);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            const int pr = wave + NWV * i;
            if (pr < npairs) {
                const int ob = pr / (IB + 1), ib = pr - ob * (IB + 1);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    bf16x8 a = *reinterpret_cast<const bf16x8 *>(Zt + (32 * ob + r) * WG_RS + 16 * ks + 8 * h);
                    bf16x8 b = ones;
                    if (ib < IB) b = *reinterpret_cast<const bf16x8 *>(At + (32 * ib + r) * WG_RS + 16 * ks + 8 * h);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[i], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    float *slab = p.slabs + (int64_t)blockIdx.x * OB * 32 * WG_SLAB_COLS;
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int pr = wave + NWV * i;
        if (pr < npairs) {
            const int ob = pr / (IB + 1), ib = pr - ob * (IB + 1);
#pragma unroll
            for (int q = 0; q < 16; ++q) slab[(32 * ob + rho(q, h)) * WG_SLAB_COLS + (ib < IB ? 32 * ib : 64) + r] = acc[i][q];
        }
    }
}

}  // namespace

static void wgrad_launch(const WgradBatch &b, int count, bool a1_f32, bool small, int n_blocks, size_t lds, hipStream_t st) {
    const dim3 grid(n_blocks, count);
    if (a1_f32) {
        if (small) hipLaunchKernelGGL((mlp_wgrad_kernel<float, 2>), grid, dim3(256), lds, st, b);
        else hipLaunchKernelGGL((mlp_wgrad_kernel<float, 6>), grid, dim3(256), lds, st, b);
    } else {
        if (small) hipLaunchKernelGGL((mlp_wgrad_kernel<bf16_t, 2>), grid, dim3(256), lds, st, b);
        else hipLaunchKernelGGL((mlp_wgrad_kernel<bf16_t, 3, 8>), grid, dim3(512), lds, st, b);
    }
}

extern "C" int pag_mlp_wgrad_blocks(int64_t M) {
    int64_t chunks = (M + 63) / 64;
    return (int)(chunks < 1024 ? (chunks > 0 ? chunks : 1) : 1024);
}

extern "C" int pag_mlp_wgrad(const void *dz, int dz_cols, int n_out, const void *a1, int a1_dtype, int a1_layout, int k1,
                             const float *a2, int k2p, const int32_t *a2_index, int n_in, float *slabs, int n_blocks, int64_t M,
                             void *stream) {
    PAG_CHECK_ARG(M >= 0, "pag_mlp_wgrad: M < 0");
    PAG_CHECK_ARG(n_out >= 1 && n_out <= 224 && dz_cols >= n_out, "pag_mlp_wgrad: n_out %d / dz_cols %d out of range", n_out, dz_cols);
    PAG_CHECK_ARG(k1 > 0 && k1 % 8 == 0, "pag_mlp_wgrad: k1 %d must be a positive multiple of 8", k1);
    PAG_CHECK_ARG(a2 == nullptr || (k2p > 0 && k2p % 8 == 0 && a2_index), "pag_mlp_wgrad: a2 needs k2p %% 8 == 0 and a2_index");
    PAG_CHECK_ARG(n_in >= 1 && n_in <= 64 && n_in <= k1 + (a2 ? k2p : 0), "pag_mlp_wgrad: n_in %d out of range", n_in);
    PAG_CHECK_ARG(a1_dtype == PAG_F32 || a1_dtype == PAG_BF16, "pag_mlp_wgrad: a1 dtype must be F32 or BF16");
    PAG_CHECK_ARG(n_blocks >= 1, "pag_mlp_wgrad: n_blocks < 1");
    if (M == 0) return PAG_OK;
    PAG_CHECK_ARG(dz && a1 && slabs, "pag_mlp_wgrad: NULL dz/a1/slabs");
    PAG_CHECK_ARG(a1_layout == PAG_LAYOUT_STRIDED || (a1_dtype == PAG_BF16 && k1 == 64 && n_in == 64 && a2 == nullptr),
                  "pag_mlp_wgrad: XCD8 a1 needs bf16, k1 = n_in = 64 and no a2");
    WgradParams p{(const bf16_t *)dz, dz_cols, n_out, a1, k1, a2, a2 ? k2p : 0, a2_index, n_in, slabs, M, a1_layout == PAG_LAYOUT_XCD8};
    const int OB = (n_out + 31) / 32, IB = (n_in + 31) / 32;
    const size_t lds = WgradLds(OB, IB).bytes;
    const bool small = OB * (IB + 1) <= 8;      // fewer accumulators -> fewer VGPRs -> more resident workgroups
    WgradBatch b{};
    b.p[0] = p;
    wgrad_launch(b, 1, a1_dtype == PAG_F32, small, n_blocks, lds, (hipStream_t)stream);
    PAG_CHECK_LAUNCH("pag_mlp_wgrad");
    return PAG_OK;
}

extern "C" int pag_mlp_wgrad_finish(const float *slabs, int n_blocks, int n_out, int n_in, int a1_layout, int a1_levels, int a1_feats,
                                    float *dW, float *db, void *stream) {
    PAG_CHECK_ARG(n_blocks >= 1 && n_out >= 1 && n_out <= 224 && n_in >= 1 && n_in <= 64, "pag_mlp_wgrad_finish: size out of range");
    PAG_CHECK_ARG(slabs && dW && db, "pag_mlp_wgrad_finish: NULL slabs/dW/db");
    const int grouped = a1_layout == PAG_LAYOUT_XCD8;
    PAG_CHECK_ARG(!grouped || (a1_levels >= 1 && a1_feats >= 1 && a1_levels * a1_feats == n_in && ((a1_levels + 7) / 8) * a1_feats <= 8),
                  "pag_mlp_wgrad_finish: XCD8 needs n_in = levels*feats");
    FinishBatch fb{};
    fb.p[0] = FinishParams{slabs, n_blocks, n_out, (n_out + 31) / 32 * 32, n_in, grouped ? a1_levels : 0, a1_feats, dW, db};
    launch_wgrad_finish(fb, n_out, 1, (hipStream_t)stream);
    PAG_CHECK_LAUNCH("pag_mlp_wgrad_finish");
    return PAG_OK;
}

// All weight gradients of one decoder: the layers that share a kernel variant (input dtype, narrow / wide) go into ONE slab
// launch (grid.y = layer) and ONE finish launch sums every layer's slabs - 2-3 launches per decoder instead of 2 per layer.
extern "C" int pag_mlp_wgrad_batch(const pag_wgrad_layer *layers, int n_layers, int64_t M, void *stream) {
    PAG_CHECK_ARG(layers && n_layers >= 1 && n_layers <= WG_MAX_BATCH, "pag_mlp_wgrad_batch: n_layers %d not in [1,%d]", n_layers, WG_MAX_BATCH);
    PAG_CHECK_ARG(M >= 1, "pag_mlp_wgrad_batch: M < 1 (callers zero the gradients of an empty batch themselves)");
    hipStream_t st = (hipStream_t)stream;
    bool done[WG_MAX_BATCH] = {};
    FinishBatch fb{};
    int max_out = 0;
    for (int l = 0; l < n_layers; ++l) {
        const pag_wgrad_layer &y = layers[l];
        PAG_CHECK_ARG(y.n_out >= 1 && y.n_out <= 224 && y.dz_cols >= y.n_out, "pag_mlp_wgrad_batch: layer %d n_out %d / dz_cols %d out of range", l, y.n_out, y.dz_cols);
        PAG_CHECK_ARG(y.k1 > 0 && y.k1 % 8 == 0, "pag_mlp_wgrad_batch: layer %d k1 %d must be a positive multiple of 8", l, y.k1);
        PAG_CHECK_ARG(y.a2 == nullptr || (y.k2p > 0 && y.k2p % 8 == 0 && y.a2_index), "pag_mlp_wgrad_batch: layer %d a2 needs k2p %% 8 == 0 and a2_index", l);
        PAG_CHECK_ARG(y.n_in >= 1 && y.n_in <= 64 && y.n_in <= y.k1 + (y.a2 ? y.k2p : 0), "pag_mlp_wgrad_batch: layer %d n_in %d out of range", l, y.n_in);
        PAG_CHECK_ARG(y.a1_dtype == PAG_F32 || y.a1_dtype == PAG_BF16, "pag_mlp_wgrad_batch: layer %d a1 dtype must be F32 or BF16", l);
        PAG_CHECK_ARG(y.n_blocks >= 1 && y.dz && y.a1 && y.slabs && y.dW && y.db, "pag_mlp_wgrad_batch: layer %d NULL pointer or n_blocks < 1", l);
        const bool grouped = y.a1_layout == PAG_LAYOUT_XCD8;
        PAG_CHECK_ARG(!grouped || (y.a1_dtype == PAG_BF16 && y.k1 == 64 && y.n_in == 64 && y.a2 == nullptr && y.a1_levels >= 1 && y.a1_feats >= 1 &&
                                   ((y.a1_levels + 7) / 8) * y.a1_feats <= 8),
                      "pag_mlp_wgrad_batch: layer %d XCD8 a1 needs bf16, k1 = n_in = 64 (staged positions), levels*feats <= 64 and no a2", l);
        // XCD8: the slab columns are the 64 staged positions, dW has levels*feats feature columns
        fb.p[l] = FinishParams{y.slabs, y.n_blocks, y.n_out, (y.n_out + 31) / 32 * 32, grouped ? y.a1_levels * y.a1_feats : y.n_in,
                               grouped ? y.a1_levels : 0, y.a1_feats, y.dW, y.db};
        max_out = std::max(max_out, y.n_out);
    }
    for (int l = 0; l < n_layers; ++l) {
        if (done[l]) continue;
        const pag_wgrad_layer &y = layers[l];
        const bool f32 = y.a1_dtype == PAG_F32;
        const bool small = ((y.n_out + 31) / 32) * ((y.n_in + 31) / 32 + 1) <= 8;
        WgradBatch b{};
        int count = 0;
        size_t lds = 0;
        for (int k = l; k < n_layers; ++k) {
            const pag_wgrad_layer &z = layers[k];
            const int OB = (z.n_out + 31) / 32, IB = (z.n_in + 31) / 32;
            if (done[k] || (z.a1_dtype == PAG_F32) != f32 || (OB * (IB + 1) <= 8) != small || z.n_blocks != y.n_blocks) continue;
            b.p[count++] = WgradParams{(const bf16_t *)z.dz, z.dz_cols, z.n_out, z.a1, z.k1, z.a2, z.a2 ? z.k2p : 0, z.a2_index, z.n_in, z.slabs, M,
                                       z.a1_layout == PAG_LAYOUT_XCD8};
            lds = std::max<size_t>(lds, WgradLds(OB, IB).bytes);      // the launch's layers share a workgroup size: the largest layout
            done[k] = true;
        }
        wgrad_launch(b, count, f32, small, y.n_blocks, lds, st);
        PAG_CHECK_LAUNCH("pag_mlp_wgrad_batch (slabs)");
    }
    launch_wgrad_finish(fb, max_out, n_layers, st);
    PAG_CHECK_LAUNCH("pag_mlp_wgrad_batch (finish)");
    return PAG_OK;
}
