// TensoRF vector-matrix grid (grids/tensorf.py::VMSplitFeatureVolume): fused gather + product + basis projection, and its backward.
//
// Tables are channel-last (plane [R][R][C], line [R][C]): one bilinear tap of the 16 density and 48 appearance components is a 64-B and a 192-B row,
// and the 64 lanes of a wave are the 64 components of ONE sample (lanes 0..15 density, 16..63 appearance).  The sample index is wave-uniform, so
// the pixel coordinates, weights and bounds tests are scalar work and a table gradient leaves the wave as contiguous rows.
//
//   forward   phase 1: wave per sample, 18 taps per lane, the three plane x line products go to an LDS tile [64 samples][48 + 144]
//             phase 2: lane per sample, wave per 7 of the 27 basis rows (wave-uniform basis reads); the fourth wave also sums the density products
//   backward  phase 1: wave per sample; samples whose upstream gradients are all zero are skipped (a wave-uniform test); g_prod = g_app . basis from
//             81 basis values per lane kept in registers; the taps are recomputed; tap gradients are summed in registers while consecutive samples
//             stay in the same cell (the samples of a ray are consecutive) and leave as one atomic row per cell visit
//             phase 2: the basis gradient g_app^T . prod from the LDS tiles, 18 accumulators per thread over the whole launch, written as
//             per-workgroup partial sums; vm_basis_finish_kernel adds them in workgroup order (no atomics: fixed bits)
// Arithmetic follows grid_sample's op order (pixel = ((c + 1) / 2) * (R - 1); nw, ne, sw, se); built without FMA contraction.
#include "common.h"
#include <limits.h>

namespace {

constexpr int DC = 16, AC = 48, AD = 27, KP = 3 * AC;        // density / appearance components, appearance width, basis columns
constexpr int TILE = 64;                                     // samples per LDS tile (16 per wave)
constexpr int CHUNK = 256;                                   // consecutive samples per workgroup visit (64 per wave: the span tap sums are merged over)
constexpr int FROW = 3 * DC + KP + 1;                        // forward tile row: 48 density + 144 appearance products, odd stride
constexpr int BROW = KP + 1;                                 // backward tile row
constexpr int GROW = 32;                                     // backward g_app row (27, zero padded)
constexpr int MAX_BWD_BLOCKS = 1024;

struct VmTables {
    const float *dp[3], *dl[3], *ap[3], *al[3], *basis;
    int R;
};
struct VmGrads {
    float *dp[3], *dl[3], *ap[3], *al[3];
};

// grid_sample's unnormalize (align_corners) with the result kept inside [-2, R + 1]: beyond that every tap is outside the table anyway, and the
// integer conversion below stays defined for any input (NaN becomes -2: all taps outside)
__device__ __forceinline__ float vm_pixel(float c, float rm1) {
    const float p = ((c + 1.0f) / 2.0f) * rm1;
    return fminf(fmaxf(p, -2.0f), rm1 + 2.0f);
}

struct Axis {
    int i0;          // floor(pixel)
    float w0, w1;    // weights of taps i0 and i0 + 1
};
__device__ __forceinline__ Axis vm_axis(float c, float rm1) {
    const float p = vm_pixel(c, rm1);
    const float f = floorf(p);
    Axis a;
    a.i0 = (int)f;
    a.w0 = (f + 1.0f) - p;
    a.w1 = p - f;
    return a;
}
__device__ __forceinline__ bool vm_in(int i, int R) { return i >= 0 && i < R; }

// plane i reads (a, b) = matMode[i] = {xy, xz, yz}: a indexes the columns, b the rows; line i runs along vecMode[i] = {z, y, x}
__device__ __forceinline__ void vm_coords(const float *__restrict__ xyz, int64_t s, int i, float &a, float &b, float &l) {
    const float x = xyz[s * 3], y = xyz[s * 3 + 1], z = xyz[s * 3 + 2];
    a = i == 2 ? y : x;
    b = i == 0 ? y : z;
    l = i == 0 ? z : (i == 1 ? y : x);
}

__device__ __forceinline__ float vm_plane(const float *__restrict__ p, int R, int C, int c, const Axis &ax, const Axis &ay) {
    if (!p) return 0.0f;               // a set that is not part of this call
    const float *q = p + ((int64_t)ay.i0 * R + ax.i0) * C + c;
    const bool x0 = vm_in(ax.i0, R), x1 = vm_in(ax.i0 + 1, R), y0 = vm_in(ay.i0, R), y1 = vm_in(ay.i0 + 1, R);
    float v = 0.0f;
    if (y0 && x0) v += q[0] * (ax.w0 * ay.w0);
    if (y0 && x1) v += q[C] * (ax.w1 * ay.w0);
    if (y1 && x0) v += q[(int64_t)R * C] * (ax.w0 * ay.w1);
    if (y1 && x1) v += q[(int64_t)R * C + C] * (ax.w1 * ay.w1);
    return v;
}
__device__ __forceinline__ float vm_line(const float *__restrict__ p, int R, int C, int c, const Axis &al) {
    if (!p) return 0.0f;
    const float *q = p + (int64_t)al.i0 * C + c;
    float v = 0.0f;
    if (vm_in(al.i0, R)) v += q[0] * al.w0;
    if (vm_in(al.i0 + 1, R)) v += q[C] * al.w1;
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(256) void vm_fwd_kernel(VmTables t, const float *__restrict__ xyz, int64_t M, float *__restrict__ sigma, float *__restrict__ app) {
    __shared__ float tile[TILE * FROW];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const bool dens = lane < DC;
    const int C = dens ? DC : AC, c = dens ? lane : lane - DC, R = t.R;
    const float rm1 = (float)(R - 1);
    const float *pl[3], *ln[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pl[i] = dens ? t.dp[i] : t.ap[i];
        ln[i] = dens ? t.dl[i] : t.al[i];
    }
    const int col = dens ? c : 3 * DC + c;
    const int cstep = dens ? DC : AC;
    const int64_t chunk0 = (int64_t)blockIdx.x * CHUNK;
    for (int64_t tile0 = chunk0; tile0 < chunk0 + CHUNK && tile0 < M; tile0 += TILE) {
#pragma unroll 2
        for (int k = 0; k < TILE / 4; ++k) {
            const int ls = wave * (TILE / 4) + k;
            const int64_t s = tile0 + ls;
            if (s >= M) break;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                float a, b, l;
                vm_coords(xyz, s, i, a, b, l);
                const Axis ax = vm_axis(a, rm1), ay = vm_axis(b, rm1), al = vm_axis(l, rm1);
                tile[ls * FROW + col + i * cstep] = vm_plane(pl[i], R, C, c, ax, ay) * vm_line(ln[i], R, C, c, al);
            }
        }
        __syncthreads();
        const int64_t s = tile0 + lane;
        if (s < M) {
            const float *row = tile + lane * FROW;
            if (app) {
                const int j0 = wave * 7;
                float acc[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                const float *B[7];
#pragma unroll
                for (int jj = 0; jj < 7; ++jj) B[jj] = t.basis + (int64_t)min(j0 + jj, AD - 1) * KP;       // row 27 does not exist: read 26, never stored
                for (int k = 0; k < KP; ++k) {
                    const float p = row[3 * DC + k];
#pragma unroll
                    for (int jj = 0; jj < 7; ++jj) acc[jj] += B[jj][k] * p;
                }
#pragma unroll
                for (int jj = 0; jj < 7; ++jj)
                    if (j0 + jj < AD) app[s * AD + j0 + jj] = acc[jj];
            }
            if (sigma && wave == 3) {
                float sg = 0.0f;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    float si = 0.0f;
#pragma unroll
                    for (int cc = 0; cc < DC; ++cc) si += row[i * DC + cc];
                    sg = sg + si;
                }
                sigma[s] = sg;
            }
        }
        __syncthreads();
    }
}

// density only (prune: one sample per dense cell, no appearance): 16 lanes per sample, four samples per wave
__global__ __launch_bounds__(256) void vm_density_kernel(VmTables t, const float *__restrict__ xyz, int64_t M, float *__restrict__ sigma) {
    const int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int c = threadIdx.x & 15, R = t.R;
    const float rm1 = (float)(R - 1);
    if (s >= M) return;                 // whole 16-lane groups leave together
    float sg = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float a, b, l;
        vm_coords(xyz, s, i, a, b, l);
        const Axis ax = vm_axis(a, rm1), ay = vm_axis(b, rm1), al = vm_axis(l, rm1);
        float v = vm_plane(t.dp[i], R, DC, c, ax, ay) * vm_line(t.dl[i], R, DC, c, al);
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d, 16);
        sg = sg + v;
    }
    if (c == 0) sigma[s] = sg;
}

// --------------------------------------------------------------------------------------------------------------------------------- backward
struct CellSums {
    int x0, y0;          // the cell the plane sums belong to (floor of the pixel pair); y0 = INT_MIN: empty
    int l0;              // the line cell; INT_MIN: empty
    float p[4], l[2];
};

__device__ __forceinline__ void vm_add(float *p, float v) {
    if (v != 0.0f) atomicAdd(p, v);
}
__device__ __forceinline__ void vm_flush_plane(CellSums &cs, float *__restrict__ g, int R, int C, int c) {
    if (cs.y0 != INT_MIN && g) {
        float *q = g + ((int64_t)cs.y0 * R + cs.x0) * C + c;
        const bool x0 = vm_in(cs.x0, R), x1 = vm_in(cs.x0 + 1, R), y0 = vm_in(cs.y0, R), y1 = vm_in(cs.y0 + 1, R);
        if (y0 && x0) vm_add(q, cs.p[0]);
        if (y0 && x1) vm_add(q + C, cs.p[1]);
        if (y1 && x0) vm_add(q + (int64_t)R * C, cs.p[2]);
        if (y1 && x1) vm_add(q + (int64_t)R * C + C, cs.p[3]);
    }
    cs.p[0] = cs.p[1] = cs.p[2] = cs.p[3] = 0.0f;
}
__device__ __forceinline__ void vm_flush_line(CellSums &cs, float *__restrict__ g, int R, int C, int c) {
    if (cs.l0 != INT_MIN && g) {
        float *q = g + (int64_t)cs.l0 * C + c;
        if (vm_in(cs.l0, R)) vm_add(q, cs.l[0]);
        if (vm_in(cs.l0 + 1, R)) vm_add(q + C, cs.l[1]);
    }
    cs.l[0] = cs.l[1] = 0.0f;
}

__global__ __launch_bounds__(256) void vm_bwd_kernel(VmTables t, VmGrads g, const float *__restrict__ xyz, int64_t M, const float *__restrict__ g_sigma,
                                                     const float *__restrict__ g_app, float *__restrict__ partials, int64_t n_chunks) {
    __shared__ float tile[TILE * BROW];
    __shared__ float gt[TILE * GROW];
    __shared__ int flag[TILE];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const bool dens = lane < DC;
    const int C = dens ? DC : AC, c = dens ? lane : lane - DC, R = t.R;
    const float rm1 = (float)(R - 1);
    const float *pl[3], *ln[3];
    float *gpl[3], *gln[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pl[i] = dens ? t.dp[i] : t.ap[i];
        ln[i] = dens ? t.dl[i] : t.al[i];
        gpl[i] = dens ? g.dp[i] : g.ap[i];
        gln[i] = dens ? g.dl[i] : g.al[i];
    }
    // the lane's three basis columns (density lanes read column c too and never use it)
    float Bc[3][AD];
    if (g_app) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < AD; ++j) Bc[i][j] = t.basis[j * KP + i * AC + c];
    }
    CellSums cs[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        cs[i].x0 = 0;
        cs[i].y0 = INT_MIN;
        cs[i].l0 = INT_MIN;
        cs[i].p[0] = cs[i].p[1] = cs[i].p[2] = cs[i].p[3] = cs[i].l[0] = cs[i].l[1] = 0.0f;
    }
    // basis gradient: thread -> rows {jj, jj + 16}, columns kk + 16 m
    const int kk = threadIdx.x & 15, jj = threadIdx.x >> 4;
    float acc0[9], acc1[9];
#pragma unroll
    for (int m = 0; m < 9; ++m) acc0[m] = acc1[m] = 0.0f;

    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        for (int sub = 0; sub < CHUNK / TILE; ++sub) {
            // wave w owns the 64 consecutive samples chunk * 256 + 64 w ..: 16 of them per tile
            int any_app = 0;
            for (int k = 0; k < TILE / 4; ++k) {
                const int ls = wave * (TILE / 4) + k;
                const int64_t s = chunk * CHUNK + wave * (CHUNK / 4) + sub * (TILE / 4) + k;
                float gs = 0.0f, ga = 0.0f;
                if (s < M) {
                    if (g_sigma) gs = g_sigma[s];
                    if (g_app && lane < AD) ga = g_app[s * AD + lane];
                }
                const bool app_on = __ballot(ga != 0.0f) != 0ull;
                if (lane == 0) flag[ls] = app_on ? 1 : 0;
                if (!app_on && gs == 0.0f) continue;          // wave-uniform: nothing to add for this sample
                float gp[3] = {dens ? gs : 0.0f, dens ? gs : 0.0f, dens ? gs : 0.0f};
                if (app_on) {
                    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
                    for (int j = 0; j < AD; ++j) {
                        const float gj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ga), j));
                        a0 += gj * Bc[0][j];
                        a1 += gj * Bc[1][j];
                        a2 += gj * Bc[2][j];
                    }
                    if (!dens) gp[0] = a0, gp[1] = a1, gp[2] = a2;
                    if (lane < GROW) gt[ls * GROW + lane] = ga;
                    any_app = 1;
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    float a, b, l;
                    vm_coords(xyz, s, i, a, b, l);
                    const Axis ax = vm_axis(a, rm1), ay = vm_axis(b, rm1), al = vm_axis(l, rm1);
                    const float pv = vm_plane(pl[i], R, C, c, ax, ay), lv = vm_line(ln[i], R, C, c, al);
                    if (app_on && !dens) tile[ls * BROW + i * AC + c] = pv * lv;
                    if (cs[i].y0 != ay.i0 || cs[i].x0 != ax.i0) {
                        vm_flush_plane(cs[i], gpl[i], R, C, c);
                        cs[i].x0 = ax.i0;
                        cs[i].y0 = ay.i0;
                    }
                    if (cs[i].l0 != al.i0) {
                        vm_flush_line(cs[i], gln[i], R, C, c);
                        cs[i].l0 = al.i0;
                    }
                    const float dpv = gp[i] * lv, dlv = gp[i] * pv;
                    cs[i].p[0] += dpv * (ax.w0 * ay.w0);
                    cs[i].p[1] += dpv * (ax.w1 * ay.w0);
                    cs[i].p[2] += dpv * (ax.w0 * ay.w1);
                    cs[i].p[3] += dpv * (ax.w1 * ay.w1);
                    cs[i].l[0] += dlv * al.w0;
                    cs[i].l[1] += dlv * al.w1;
                }
            }
            if (!g_app) continue;                             // kernel-uniform: no basis gradient, no barriers
            const int some = __syncthreads_or(any_app);
            if (some) {
                for (int ls = 0; ls < TILE; ++ls) {
                    if (!flag[ls]) continue;
                    const float g0 = gt[ls * GROW + jj], g1 = gt[ls * GROW + jj + 16];
#pragma unroll
                    for (int m = 0; m < 9; ++m) {
                        const float p = tile[ls * BROW + kk + 16 * m];
                        acc0[m] += g0 * p;
                        acc1[m] += g1 * p;
                    }
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        vm_flush_plane(cs[i], gpl[i], R, C, c);
        vm_flush_line(cs[i], gln[i], R, C, c);
    }
    if (g_app) {
        float *out = partials + (int64_t)blockIdx.x * (AD * KP);
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            out[jj * KP + kk + 16 * m] = acc0[m];
            if (jj + 16 < AD) out[(jj + 16) * KP + kk + 16 * m] = acc1[m];
        }
    }
}

__global__ __launch_bounds__(256) void vm_basis_finish_kernel(const float *__restrict__ partials, int nb, float *__restrict__ g_basis) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= AD * KP) return;
    float s = 0.0f;
    for (int b = 0; b < nb; ++b) s += partials[(int64_t)b * (AD * KP) + e];
    g_basis[e] = s;
}

int64_t vm_bwd_blocks(int64_t M) {
    const int64_t chunks = (M + CHUNK - 1) / CHUNK;
    return chunks < MAX_BWD_BLOCKS ? chunks : MAX_BWD_BLOCKS;
}

int vm_check(const char *name, const pag_vm_args *a, int64_t M) {
    PAG_CHECK_ARG(a, "%s: NULL args", name);
    PAG_CHECK_ARG(M >= 0 && M <= ((int64_t)1 << 31), "%s: M %lld not in [0,2^31]", name, (long long)M);
    PAG_CHECK_ARG(pag_vm_supported(a->density_n_comp, a->app_n_comp, a->app_dim, a->res),
                  "%s: unsupported shape: density_n_comp %d (16), app_n_comp %d (48), app_dim %d (27), res %d ([2,2048])", name, a->density_n_comp,
                  a->app_n_comp, a->app_dim, a->res);
    return PAG_OK;
}

void vm_tables(const pag_vm_args *a, VmTables &t) {
    for (int i = 0; i < 3; ++i) {
        t.dp[i] = a->density_plane[i];
        t.dl[i] = a->density_line[i];
        t.ap[i] = a->app_plane[i];
        t.al[i] = a->app_line[i];
    }
    t.basis = a->basis;
    t.R = a->res;
}

}  // namespace

extern "C" int pag_vm_supported(int density_n_comp, int app_n_comp, int app_dim, int res) {
    return density_n_comp == DC && app_n_comp == AC && app_dim == AD && res >= 2 && res <= 2048 ? 1 : 0;
}

extern "C" int64_t pag_vm_bwd_workspace_bytes(int64_t M) {
    if (M < 0 || M > ((int64_t)1 << 31)) {
        pag_set_error("pag_vm_bwd_workspace_bytes: M %lld not in [0,2^31]", (long long)M);
        return -1;
    }
    return vm_bwd_blocks(M) * (int64_t)(AD * KP) * (int64_t)sizeof(float);
}

extern "C" int pag_vm_fwd(const pag_vm_args *a, int64_t M, void *stream) {
    int rc = vm_check("pag_vm_fwd", a, M);
    if (rc != PAG_OK) return rc;
    if (M == 0) return PAG_OK;
    PAG_CHECK_ARG(a->xyz, "pag_vm_fwd: NULL xyz");
    PAG_CHECK_ARG(a->sigma || a->app, "pag_vm_fwd: NULL sigma and app (at least one output is needed)");
    for (int i = 0; i < 3; ++i) {
        PAG_CHECK_ARG(!a->sigma || (a->density_plane[i] && a->density_line[i]), "pag_vm_fwd: NULL density table %d", i);
        PAG_CHECK_ARG(!a->app || (a->app_plane[i] && a->app_line[i]), "pag_vm_fwd: NULL appearance table %d", i);
    }
    PAG_CHECK_ARG(!a->app || a->basis, "pag_vm_fwd: NULL basis");
    VmTables t;
    vm_tables(a, t);
    if (!a->app) {
        hipLaunchKernelGGL(vm_density_kernel, dim3((unsigned)((M * 16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, a->xyz, M, a->sigma);
    } else {
        if (!a->sigma)                     // appearance only: the density lanes gather nothing
            for (int i = 0; i < 3; ++i) t.dp[i] = t.dl[i] = nullptr;
        hipLaunchKernelGGL(vm_fwd_kernel, dim3((unsigned)((M + CHUNK - 1) / CHUNK)), dim3(256), 0, (hipStream_t)stream, t, a->xyz, M, a->sigma, a->app);
    }
    PAG_CHECK_LAUNCH("pag_vm_fwd");
    return PAG_OK;
}

extern "C" int pag_vm_bwd(const pag_vm_args *a, int64_t M, void *stream) {
    int rc = vm_check("pag_vm_bwd", a, M);
    if (rc != PAG_OK) return rc;
    if (M == 0) return PAG_OK;
    PAG_CHECK_ARG(a->xyz, "pag_vm_bwd: NULL xyz");
    PAG_CHECK_ARG(a->g_sigma || a->g_app, "pag_vm_bwd: NULL g_sigma and g_app (at least one upstream gradient is needed)");
    for (int i = 0; i < 3; ++i) {
        PAG_CHECK_ARG(!a->g_sigma || (a->density_plane[i] && a->density_line[i] && a->g_density_plane[i] && a->g_density_line[i]),
                      "pag_vm_bwd: NULL density table / gradient table %d", i);
        PAG_CHECK_ARG(!a->g_app || (a->app_plane[i] && a->app_line[i] && a->g_app_plane[i] && a->g_app_line[i]),
                      "pag_vm_bwd: NULL appearance table / gradient table %d", i);
    }
    const int64_t nb = vm_bwd_blocks(M);
    if (a->g_app) {
        PAG_CHECK_ARG(a->basis && a->g_basis, "pag_vm_bwd: NULL basis / g_basis");
        PAG_CHECK_ARG(a->workspace && a->workspace_bytes >= nb * (int64_t)(AD * KP) * (int64_t)sizeof(float),
                      "pag_vm_bwd: workspace NULL or %lld bytes < pag_vm_bwd_workspace_bytes", (long long)a->workspace_bytes);
    }
    VmTables t;
    vm_tables(a, t);
    VmGrads g;
    for (int i = 0; i < 3; ++i) {
        g.dp[i] = a->g_density_plane[i];
        g.dl[i] = a->g_density_line[i];
        g.ap[i] = a->g_app_plane[i];
        g.al[i] = a->g_app_line[i];
    }
    for (int i = 0; i < 3; ++i) {          // a set without an upstream gradient: its lanes gather nothing and add nothing
        if (!a->g_sigma) t.dp[i] = t.dl[i] = nullptr, g.dp[i] = g.dl[i] = nullptr;
        if (!a->g_app) t.ap[i] = t.al[i] = nullptr, g.ap[i] = g.al[i] = nullptr;
    }
    const int64_t n_chunks = (M + CHUNK - 1) / CHUNK;
    hipLaunchKernelGGL(vm_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, t, g, a->xyz, M, a->g_sigma, a->g_app, (float *)a->workspace, n_chunks);
    PAG_CHECK_LAUNCH("pag_vm_bwd");
    if (a->g_app) {
        hipLaunchKernelGGL(vm_basis_finish_kernel, dim3((AD * KP + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float *)a->workspace, (int)nb, a->g_basis);
        PAG_CHECK_LAUNCH("pag_vm_bwd (finish)");
    }
    return PAG_OK;
}
