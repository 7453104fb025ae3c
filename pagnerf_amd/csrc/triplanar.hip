// Tri-plane feature grid (wisp TriplanarGrid; the spec of record is DESIGN.md 4.18): L levels, three planes fmx / fmy / fmz of [R_l][R_l][F] per level,
//   feat_l(c) = gs(fmx_l, (y, z)) + gs(fmy_l, (x, z)) + gs(fmz_l, (x, y)),   gs = grid_sample bilinear, reflection padding, align_corners
// One flat fp32 buffer holds every level, per level [3][R][R][F] channel-last: a bilinear tap is one row of F floats (16 B at F = 4).
//
//   forward          lane per (sample, level): 12 row gathers of F floats per lane, the three planes summed in the order x, y, z, the level's F
//                    columns leave as one vector store (the lanes of a wave write consecutive 4 F-byte pieces of the output)
//   table gradient   wave per sample, lanes over (level, plane, f) as in vm.hip: the sample index is wave-uniform, a wave walks 64 consecutive samples
//                    (the samples of a ray are consecutive), every lane sums its four tap gradients in registers while its cell stays the same and
//                    emits one atomic per tap and cell visit; samples whose upstream gradient is exactly zero are skipped (a wave-uniform test)
//   position grad    lane per sample, levels and planes in a loop: no atomics, fixed order
// Arithmetic follows grid_sample's op order (unnormalize, reflect with fmod / floor, clip, nw ne sw se); built without FMA contraction.
#include "common.h"
#include <limits.h>

namespace {

constexpr int MAX_L = 8;
constexpr int WALK = 64;                   // consecutive samples per wave of the table gradient: the span tap sums are merged over
constexpr int BLOCK = 256;

struct TriLevels {
    int64_t off[MAX_L];                    // float offset of the level inside the flat buffer
    int R[MAX_L];
    int L;
};
struct TriScale {
    float v[MAX_L * 8];                    // feat_scale per output column (1 when the caller gave none)
};

struct Axis {
    int i0;            // floor(pixel) in [0, R - 1]
    float w0, w1;      // weights of taps i0 and i0 + 1
    float d;           // d pixel / d coordinate: +-(R - 1) / 2, 0 where the clip is active
};

// grid_sample's compute_coordinates for align_corners + reflection: unnormalize, reflect about [0, R - 1], clip.  The pixel is clamped into
// [0, R - 1] BEFORE the integer conversion: a non-finite or huge coordinate indexes row / column 0 or R - 1, never outside the table.
__device__ __forceinline__ Axis tri_axis(float c, float rm1) {
    const float p = ((c + 1.0f) / 2.0f) * rm1;
    const float a = fabsf(p);
    float sign = p < 0.0f ? -1.0f : 1.0f;
    float e = a, q;
    if (a < rm1) {                         // no flip: fmod(a, span) == a, floor(a / span) == 0
        q = e;
    } else {
        e = fmodf(a, rm1);
        const float k = floorf(a / rm1);
        if (fmodf(k, 2.0f) == 0.0f) {
            q = e;
        } else {
            q = rm1 - e;
            sign = -sign;
        }
    }
    float clip = 1.0f;
    if (!(q > 0.0f)) q = 0.0f, clip = 0.0f;            // NaN lands here
    if (q >= rm1) q = rm1, clip = 0.0f;
    const float f = floorf(q);
    Axis ax;
    ax.i0 = (int)f;
    ax.w0 = (f + 1.0f) - q;
    ax.w1 = q - f;
    ax.d = clip * sign * (rm1 / 2.0f);
    return ax;
}

// plane 0 = fmx reads (y, z), 1 = fmy (x, z), 2 = fmz (x, y): the first coordinate indexes the columns, the second the rows
__device__ __forceinline__ void tri_pair(float x, float y, float z, int plane, float &a, float &b) {
    a = plane == 0 ? y : x;
    b = plane == 2 ? y : z;
}

template <int F>
struct Row {
    float v[F];
};
template <int F>
__device__ __forceinline__ Row<F> tri_row(const float *__restrict__ p) {
    Row<F> r;
    if constexpr (F == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        r.v[0] = t.x, r.v[1] = t.y;
    } else {
#pragma unroll
        for (int i = 0; i < F; i += 4) {
            const float4 t = *reinterpret_cast<const float4 *>(p + i);
            r.v[i] = t.x, r.v[i + 1] = t.y, r.v[i + 2] = t.z, r.v[i + 3] = t.w;
        }
    }
    return r;
}

// one plane of one level at (a, b): out = 0; out += row * (wx * wy) for nw, ne, sw, se; the tap at index R does not exist and is skipped
template <int F>
__device__ __forceinline__ Row<F> tri_plane(const float *__restrict__ plane, int R, const Axis &ax, const Axis &ay) {
    const float *q = plane + ((int64_t)ay.i0 * R + ax.i0) * F;
    const bool x1 = ax.i0 + 1 < R, y1 = ay.i0 + 1 < R;
    Row<F> o;
#pragma unroll
    for (int f = 0; f < F; ++f) o.v[f] = 0.0f;
    {
        const Row<F> t = tri_row<F>(q);
        const float w = ax.w0 * ay.w0;
#pragma unroll
        for (int f = 0; f < F; ++f) o.v[f] += t.v[f] * w;
    }
    if (x1) {
        const Row<F> t = tri_row<F>(q + F);
        const float w = ax.w1 * ay.w0;
#pragma unroll
        for (int f = 0; f < F; ++f) o.v[f] += t.v[f] * w;
    }
    if (y1) {
        const Row<F> t = tri_row<F>(q + (int64_t)R * F);
        const float w = ax.w0 * ay.w1;
#pragma unroll
        for (int f = 0; f < F; ++f) o.v[f] += t.v[f] * w;
    }
    if (x1 && y1) {
        const Row<F> t = tri_row<F>(q + (int64_t)R * F + F);
        const float w = ax.w1 * ay.w1;
#pragma unroll
        for (int f = 0; f < F; ++f) o.v[f] += t.v[f] * w;
    }
    return o;
}

// ---------------------------------------------------------------------------------------------------------------------------------- forward
// thread = (sample, level), level fastest: block b owns the BLOCK / L samples from b * (BLOCK / L); threads past (BLOCK / L) * L idle
template <int F, typename OutT>
__global__ __launch_bounds__(BLOCK) void tri_fwd_kernel(TriLevels lv, TriScale sc, const float *__restrict__ tables, const float *__restrict__ xyz, int64_t M,
                                                        OutT *__restrict__ out, int64_t stride_m, int64_t stride_c, int vec) {
    const int L = lv.L, spb = BLOCK / L;
    const int ls = (int)threadIdx.x / L, l = (int)threadIdx.x - ls * L;
    const int64_t s = (int64_t)blockIdx.x * spb + ls;
    if (ls >= spb || s >= M) return;
    const float x = xyz[s * 3], y = xyz[s * 3 + 1], z = xyz[s * 3 + 2];
    const int R = lv.R[l];
    const float rm1 = (float)(R - 1);
    const float *base = tables + lv.off[l];
    const Axis axx = tri_axis(x, rm1), axy = tri_axis(y, rm1), axz = tri_axis(z, rm1);
    const Row<F> px = tri_plane<F>(base, R, axy, axz);
    const Row<F> py = tri_plane<F>(base + (int64_t)R * R * F, R, axx, axz);
    const Row<F> pz = tri_plane<F>(base + (int64_t)2 * R * R * F, R, axx, axy);
    float o[F];
#pragma unroll
    for (int f = 0; f < F; ++f) o[f] = ((px.v[f] + py.v[f]) + pz.v[f]) * sc.v[l * F + f];
    if (vec) {                                             // contiguous rows: the level's F columns as one store
        OutT *p = out + s * stride_m + l * F;
        if constexpr (sizeof(OutT) == 4) {
            if constexpr (F == 2) {
                *reinterpret_cast<float2 *>(p) = make_float2(o[0], o[1]);
            } else {
#pragma unroll
                for (int f = 0; f < F; f += 4) *reinterpret_cast<float4 *>(p + f) = make_float4(o[f], o[f + 1], o[f + 2], o[f + 3]);
            }
        } else {
            union {
                bf16_t h[F];
                uint32_t u[F / 2];
            } pk;
#pragma unroll
            for (int f = 0; f < F; ++f) pk.h[f] = (bf16_t)o[f];
            uint32_t *d = reinterpret_cast<uint32_t *>(p);
#pragma unroll
            for (int f = 0; f < F / 2; ++f) d[f] = pk.u[f];
        }
    } else {
#pragma unroll
        for (int f = 0; f < F; ++f) pag_st(out + s * stride_m + (int64_t)(l * F + f) * stride_c, o[f]);
    }
}

// --------------------------------------------------------------------------------------------------------------------------- table gradient
// lane = ((level - l0) * 3 + plane) * F + f for the levels l0 .. l0 + lpw - 1 of this workgroup row (blockIdx.y); lpw = 64 / (3 F)
template <int F, typename GT>
__global__ __launch_bounds__(BLOCK) void tri_bwd_tables_kernel(TriLevels lv, TriScale sc, const float *__restrict__ xyz, int64_t M, const GT *__restrict__ g,
                                                               int64_t stride_m, int64_t stride_c, float *__restrict__ gt) {
    constexpr int LPW = 64 / (3 * F);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int f = lane % F, plane = (lane / F) % 3, l = (int)blockIdx.y * LPW + lane / (3 * F);
    const bool on = lane < LPW * 3 * F && l < lv.L;
    const int R = on ? lv.R[l] : 2;
    const float rm1 = (float)(R - 1);
    const int col = on ? l * F + f : 0;
    const float scale = on ? sc.v[col] : 0.0f;
    float *gp = on ? gt + lv.off[l] + (int64_t)plane * R * R * F + f : nullptr;
    int cx = 0, cy = INT_MIN;                      // the cell the sums belong to; cy = INT_MIN: empty
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int64_t s0 = ((int64_t)blockIdx.x * (BLOCK / 64) + wave) * WALK;
    for (int k = 0; k < WALK; ++k) {
        const int64_t s = s0 + k;
        if (s >= M) break;                          // wave-uniform
        const float gv = on ? pag_ld(g + s * stride_m + (int64_t)col * stride_c) * scale : 0.0f;
        if (__ballot(gv != 0.0f) == 0ull) continue; // nothing to add for this sample
        const float x = xyz[s * 3], y = xyz[s * 3 + 1], z = xyz[s * 3 + 2];
        float a, b;
        tri_pair(x, y, z, plane, a, b);
        const Axis ax = tri_axis(a, rm1), ay = tri_axis(b, rm1);
        if (cy != ay.i0 || cx != ax.i0) {
            if (cy != INT_MIN && on) {
                float *q = gp + ((int64_t)cy * R + cx) * F;
                const bool x1 = cx + 1 < R, y1 = cy + 1 < R;
                if (sum[0] != 0.0f) atomicAdd(q, sum[0]);
                if (x1 && sum[1] != 0.0f) atomicAdd(q + F, sum[1]);
                if (y1 && sum[2] != 0.0f) atomicAdd(q + (int64_t)R * F, sum[2]);
                if (x1 && y1 && sum[3] != 0.0f) atomicAdd(q + (int64_t)R * F + F, sum[3]);
            }
            sum[0] = sum[1] = sum[2] = sum[3] = 0.0f;
            cx = ax.i0;
            cy = ay.i0;
        }
        sum[0] += gv * (ax.w0 * ay.w0);
        sum[1] += gv * (ax.w1 * ay.w0);
        sum[2] += gv * (ax.w0 * ay.w1);
        sum[3] += gv * (ax.w1 * ay.w1);
    }
    if (cy != INT_MIN && on) {
        float *q = gp + ((int64_t)cy * R + cx) * F;
        const bool x1 = cx + 1 < R, y1 = cy + 1 < R;
        if (sum[0] != 0.0f) atomicAdd(q, sum[0]);
        if (x1 && sum[1] != 0.0f) atomicAdd(q + F, sum[1]);
        if (y1 && sum[2] != 0.0f) atomicAdd(q + (int64_t)R * F, sum[2]);
        if (x1 && y1 && sum[3] != 0.0f) atomicAdd(q + (int64_t)R * F + F, sum[3]);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ position gradient
// d value / d pixel of one plane, dotted with the upstream row gr: (d / d a, d / d b) in pixels (grid_sample's backward: taps outside are skipped)
template <int F>
__device__ __forceinline__ void tri_plane_dpix(const float *__restrict__ plane, int R, const Axis &ax, const Axis &ay, const float *gr, float &da, float &db) {
    const float *q = plane + ((int64_t)ay.i0 * R + ax.i0) * F;
    const bool x1 = ax.i0 + 1 < R, y1 = ay.i0 + 1 < R;
    float t00 = 0.0f, t01 = 0.0f, t10 = 0.0f, t11 = 0.0f;
    {
        const Row<F> t = tri_row<F>(q);
#pragma unroll
        for (int f = 0; f < F; ++f) t00 += t.v[f] * gr[f];
    }
    if (x1) {
        const Row<F> t = tri_row<F>(q + F);
#pragma unroll
        for (int f = 0; f < F; ++f) t01 += t.v[f] * gr[f];
    }
    if (y1) {
        const Row<F> t = tri_row<F>(q + (int64_t)R * F);
#pragma unroll
        for (int f = 0; f < F; ++f) t10 += t.v[f] * gr[f];
    }
    if (x1 && y1) {
        const Row<F> t = tri_row<F>(q + (int64_t)R * F + F);
#pragma unroll
        for (int f = 0; f < F; ++f) t11 += t.v[f] * gr[f];
    }
    da = (t01 - t00) * ay.w0 + (t11 - t10) * ay.w1;
    db = (t10 - t00) * ax.w0 + (t11 - t01) * ax.w1;
}

template <int F, typename GT>
__global__ __launch_bounds__(BLOCK) void tri_bwd_xyz_kernel(TriLevels lv, TriScale sc, const float *__restrict__ tables, const float *__restrict__ xyz, int64_t M,
                                                            const GT *__restrict__ g, int64_t stride_m, int64_t stride_c, float *__restrict__ d_xyz) {
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= M) return;
    const float x = xyz[s * 3], y = xyz[s * 3 + 1], z = xyz[s * 3 + 2];
    float dx = 0.0f, dy = 0.0f, dz = 0.0f;
    for (int l = 0; l < lv.L; ++l) {
        float gr[F];
#pragma unroll
        for (int f = 0; f < F; ++f) gr[f] = pag_ld(g + s * stride_m + (int64_t)(l * F + f) * stride_c) * sc.v[l * F + f];
        const int R = lv.R[l];
        const float rm1 = (float)(R - 1);
        const float *base = tables + lv.off[l];
        const Axis axx = tri_axis(x, rm1), axy = tri_axis(y, rm1), axz = tri_axis(z, rm1);
        float da, db;
        tri_plane_dpix<F>(base, R, axy, axz, gr, da, db);                                   // fmx (y, z)
        dy += da * axy.d;
        dz += db * axz.d;
        tri_plane_dpix<F>(base + (int64_t)R * R * F, R, axx, axz, gr, da, db);              // fmy (x, z)
        dx += da * axx.d;
        dz += db * axz.d;
        tri_plane_dpix<F>(base + (int64_t)2 * R * R * F, R, axx, axy, gr, da, db);          // fmz (x, y)
        dx += da * axx.d;
        dy += db * axy.d;
    }
    d_xyz[s * 3] = dx;
    d_xyz[s * 3 + 1] = dy;
    d_xyz[s * 3 + 2] = dz;
}

// ------------------------------------------------------------------------------------------------------------------------------------ host
int tri_setup(const char *name, int64_t M, int n_levels, int n_feat, const int *res_host, const float *feat_scale_host, TriLevels &lv, TriScale &sc) {
    PAG_CHECK_ARG(M >= 0 && M <= ((int64_t)1 << 31), "%s: M %lld not in [0,2^31]", name, (long long)M);
    PAG_CHECK_ARG(n_levels >= 1 && n_levels <= MAX_L, "%s: n_levels %d not in [1,%d]", name, n_levels, MAX_L);
    PAG_CHECK_ARG(n_feat == 2 || n_feat == 4 || n_feat == 8, "%s: n_feat %d not in {2,4,8}", name, n_feat);
    PAG_CHECK_ARG(res_host, "%s: NULL res", name);
    int64_t off = 0;
    for (int l = 0; l < MAX_L; ++l) {
        lv.off[l] = 0;
        lv.R[l] = 2;
    }
    for (int l = 0; l < n_levels; ++l) {
        PAG_CHECK_ARG(res_host[l] >= 2 && res_host[l] <= 8193, "%s: res[%d] = %d not in [2,8193]", name, l, res_host[l]);
        lv.off[l] = off;
        lv.R[l] = res_host[l];
        off += (int64_t)3 * res_host[l] * res_host[l] * n_feat;
    }
    lv.L = n_levels;
    for (int i = 0; i < MAX_L * 8; ++i) sc.v[i] = (feat_scale_host && i < n_levels * n_feat) ? feat_scale_host[i] : 1.0f;
    return PAG_OK;
}

#define TRI_DISPATCH_F(n_feat, CALL) \
    do {                             \
        if ((n_feat) == 2) {         \
            CALL(2);                 \
        } else if ((n_feat) == 4) {  \
            CALL(4);                 \
        } else {                     \
            CALL(8);                 \
        }                            \
    } while (0)

}  // namespace

extern "C" int pag_triplanar_fwd(const float *xyz, int64_t M, const float *tables, int n_levels, int n_feat, const int *res_host, const float *feat_scale_host,
                                 void *out, int out_dtype, int64_t stride_m, int64_t stride_c, void *stream) {
    TriLevels lv;
    TriScale sc;
    int rc = tri_setup("pag_triplanar_fwd", M, n_levels, n_feat, res_host, feat_scale_host, lv, sc);
    if (rc != PAG_OK) return rc;
    PAG_CHECK_ARG(out_dtype == PAG_F32 || out_dtype == PAG_BF16, "pag_triplanar_fwd: out_dtype %d (f32 or bf16)", out_dtype);
    if (M == 0) return PAG_OK;
    PAG_CHECK_ARG(xyz && tables && out, "pag_triplanar_fwd: NULL xyz / tables / out");
    PAG_CHECK_ARG(((uintptr_t)tables) % 16 == 0, "pag_triplanar_fwd: tables must be 16-byte aligned");
    const int C = n_levels * n_feat;
    PAG_CHECK_ARG(stride_c >= 1 && stride_m >= 1, "pag_triplanar_fwd: strides %lld, %lld must be positive", (long long)stride_m, (long long)stride_c);
    const int esz = out_dtype == PAG_F32 ? 4 : 2;
    const int piece = n_feat * esz > 16 ? 16 : n_feat * esz;          // the widest store of the vector form
    const int vec = stride_c == 1 && stride_m >= C && (stride_m * esz) % piece == 0 && ((uintptr_t)out) % piece == 0 ? 1 : 0;
    const unsigned blocks = (unsigned)((M + (BLOCK / n_levels) - 1) / (BLOCK / n_levels));
#define CALL(F)                                                                                                                                             \
    if (out_dtype == PAG_F32)                                                                                                                               \
        hipLaunchKernelGGL((tri_fwd_kernel<F, float>), dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, lv, sc, tables, xyz, M, (float *)out, stride_m,   \
                           stride_c, vec);                                                                                                                  \
    else                                                                                                                                                    \
        hipLaunchKernelGGL((tri_fwd_kernel<F, bf16_t>), dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, lv, sc, tables, xyz, M, (bf16_t *)out, stride_m, \
                           stride_c, vec)
    TRI_DISPATCH_F(n_feat, CALL);
#undef CALL
    PAG_CHECK_LAUNCH("pag_triplanar_fwd");
    return PAG_OK;
}

extern "C" int pag_triplanar_bwd_tables(const float *xyz, int64_t M, const void *grad_out, int grad_dtype, int64_t stride_m, int64_t stride_c, int n_levels,
                                        int n_feat, const int *res_host, const float *feat_scale_host, float *grad_tables, void *stream) {
    TriLevels lv;
    TriScale sc;
    int rc = tri_setup("pag_triplanar_bwd_tables", M, n_levels, n_feat, res_host, feat_scale_host, lv, sc);
    if (rc != PAG_OK) return rc;
    PAG_CHECK_ARG(grad_dtype == PAG_F32 || grad_dtype == PAG_BF16, "pag_triplanar_bwd_tables: grad_dtype %d (f32 or bf16)", grad_dtype);
    if (M == 0) return PAG_OK;
    PAG_CHECK_ARG(xyz && grad_out && grad_tables, "pag_triplanar_bwd_tables: NULL xyz / grad_out / grad_tables");
    PAG_CHECK_ARG(stride_c >= 1 && stride_m >= 1, "pag_triplanar_bwd_tables: strides %lld, %lld must be positive", (long long)stride_m, (long long)stride_c);
    const int lpw = 64 / (3 * n_feat);
    const dim3 grid((unsigned)((M + BLOCK / 64 * WALK - 1) / (BLOCK / 64 * WALK)), (unsigned)((n_levels + lpw - 1) / lpw));
#define CALL(F)                                                                                                                                              \
    if (grad_dtype == PAG_F32)                                                                                                                               \
        hipLaunchKernelGGL((tri_bwd_tables_kernel<F, float>), grid, dim3(BLOCK), 0, (hipStream_t)stream, lv, sc, xyz, M, (const float *)grad_out, stride_m,  \
                           stride_c, grad_tables);                                                                                                           \
    else                                                                                                                                                     \
        hipLaunchKernelGGL((tri_bwd_tables_kernel<F, bf16_t>), grid, dim3(BLOCK), 0, (hipStream_t)stream, lv, sc, xyz, M, (const bf16_t *)grad_out, stride_m, \
                           stride_c, grad_tables)
    TRI_DISPATCH_F(n_feat, CALL);
#undef CALL
    PAG_CHECK_LAUNCH("pag_triplanar_bwd_tables");
    return PAG_OK;
}

extern "C" int pag_triplanar_bwd_xyz(const float *xyz, int64_t M, const float *tables, const void *grad_out, int grad_dtype, int64_t stride_m, int64_t stride_c,
                                     int n_levels, int n_feat, const int *res_host, const float *feat_scale_host, float *d_xyz, void *stream) {
    TriLevels lv;
    TriScale sc;
    int rc = tri_setup("pag_triplanar_bwd_xyz", M, n_levels, n_feat, res_host, feat_scale_host, lv, sc);
    if (rc != PAG_OK) return rc;
    PAG_CHECK_ARG(grad_dtype == PAG_F32 || grad_dtype == PAG_BF16, "pag_triplanar_bwd_xyz: grad_dtype %d (f32 or bf16)", grad_dtype);
    if (M == 0) return PAG_OK;
    PAG_CHECK_ARG(xyz && tables && grad_out && d_xyz, "pag_triplanar_bwd_xyz: NULL xyz / tables / grad_out / d_xyz");
    PAG_CHECK_ARG(((uintptr_t)tables) % 16 == 0, "pag_triplanar_bwd_xyz: tables must be 16-byte aligned");
    PAG_CHECK_ARG(stride_c >= 1 && stride_m >= 1, "pag_triplanar_bwd_xyz: strides %lld, %lld must be positive", (long long)stride_m, (long long)stride_c);
    const unsigned blocks = (unsigned)((M + BLOCK - 1) / BLOCK);
#define CALL(F)                                                                                                                                                  \
    if (grad_dtype == PAG_F32)                                                                                                                                   \
        hipLaunchKernelGGL((tri_bwd_xyz_kernel<F, float>), dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, lv, sc, tables, xyz, M, (const float *)grad_out,   \
                           stride_m, stride_c, d_xyz);                                                                                                           \
    else                                                                                                                                                         \
        hipLaunchKernelGGL((tri_bwd_xyz_kernel<F, bf16_t>), dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, lv, sc, tables, xyz, M, (const bf16_t *)grad_out, \
                           stride_m, stride_c, d_xyz)
    TRI_DISPATCH_F(n_feat, CALL);
#undef CALL
    PAG_CHECK_LAUNCH("pag_triplanar_bwd_xyz");
    return PAG_OK;
}
