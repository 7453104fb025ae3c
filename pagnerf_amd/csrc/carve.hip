// Occupancy carving from depth images for gfx950 (pagnerf_amd/carve.py is the definition: carve_reference, carve_finish_reference).
//
//   pag_carve_rays    every valid depth pixel's ray is walked through the 2^level lattice; the cells in front of the measured surface are OR-ed into
//                     `free_bits`, the cells within `margin` of it into `surface_bits`.
//   pag_carve_finish  surface dilated by the 26-neighbourhood, combined with the free set -> the occupancy bitfield the marches read.
//
// Memory behaviour of the walk.  A lane owns a ray, as in render.hip's voxel_walk_kernel, whose DDA is restated here operation for operation (the
// candidates (t_in, t_out, cell) are the same bits; render.hip itself is untouched, so its kernels compile to what they were).  What differs is what a
// step does with its candidate: it sets one bit of one of two bitfields (256 KB each at level 7: both stay in L2).  Neighbouring pixels cross almost
// the same cells, and after the first views nearly every bit a ray would set is set already, so a step first LOADS the word and issues the vector
// atomic OR only when its bit is still clear (the load bypasses L1, see carve_set; an XCD's L2 may still hold a word that another XCD has since
// added to).  Bits are only ever set, so a stale word costs a redundant atomic and never a lost bit: the result is a
// set, independent of the order of rays, lanes and launches - the same input gives the same bits.  The load is not on the loop-carried path (the DDA
// state does not depend on it), and a ray leaves the walk at the first candidate that starts behind t_hit + margin, so a wave ends with its last
// surface, not at the far side of the cube.
#include "common.h"

namespace {

struct CarveArgs {
    const float *origins, *dirs, *t_hit;
    int64_t N;
    int level;
    float dmin, dmax, margin;
    uint32_t *free_bits, *surface_bits;
};

__device__ __forceinline__ void carve_set(uint32_t *bits, int32_t cell) {
    uint32_t *w = bits + (cell >> 5);
    const uint32_t b = 1u << (cell & 31);
    // the test reads past the CU's L1 (a device-scope load): the atomics execute at the memory side and do not update an L1 line, which would go on
    // answering "clear" to every later wave of the CU until it is evicted
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & b)) atomicOr(w, b);
}

__global__ __launch_bounds__(256) void carve_rays_kernel(CarveArgs a) {
    const int R = 1 << a.level;
    const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= a.N) return;
    const float th = a.t_hit[ray];
    if (!(th > 0.0f) || !(th < INFINITY)) return;                  // invalid pixel: t_hit <= 0, NaN or infinite
    const float lo = __fsub_rn(th, a.margin), hi = __fadd_rn(th, a.margin);
    const float cs = __fdiv_rn(2.0f, (float)R);
    const float o[3] = {a.origins[ray * 3], a.origins[ray * 3 + 1], a.origins[ray * 3 + 2]};
    const float d[3] = {a.dirs[ray * 3], a.dirs[ray * 3 + 1], a.dirs[ray * 3 + 2]};
    float t0 = a.dmin, t1 = a.dmax;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (d[ax] != 0.0f) {
            const float ta = __fdiv_rn(__fsub_rn(-1.0f, o[ax]), d[ax]), tb = __fdiv_rn(__fsub_rn(1.0f, o[ax]), d[ax]);
            const float l = ta < tb ? ta : tb, h = ta < tb ? tb : ta;
            t0 = t0 >= l ? t0 : l;
            t1 = t1 <= h ? t1 : h;
        } else if (o[ax] < -1.0f || o[ax] > 1.0f) {
            t1 = -1.0f;
        }
    }
    if (!(t0 < t1)) return;
    const float tm = __fadd_rn(t0, __fmul_rn(__fsub_rn(t1, t0), 1e-6f));
    int c0, c1, c2, s0 = 0, s1 = 0, s2 = 0;
    float n0 = INFINITY, n1 = INFINITY, n2 = INFINITY, e0 = INFINITY, e1 = INFINITY, e2 = INFINITY;
    auto setup = [&](int ax, int &c, int &st, float &tn, float &td) {
        const float pa = __fadd_rn(__fmul_rn(d[ax], tm), o[ax]);
        int ci = (int)floorf(__fdiv_rn(__fadd_rn(pa, 1.0f), cs));
        c = min(max(ci, 0), R - 1);
        if (d[ax] > 0.0f) {
            st = 1;
            tn = __fdiv_rn(__fsub_rn(__fadd_rn(-1.0f, __fmul_rn((float)(c + 1), cs)), o[ax]), d[ax]);
            td = __fdiv_rn(cs, d[ax]);
        } else if (d[ax] < 0.0f) {
            st = -1;
            tn = __fdiv_rn(__fsub_rn(__fadd_rn(-1.0f, __fmul_rn((float)c, cs)), o[ax]), d[ax]);
            td = __fdiv_rn(cs, -d[ax]);
        }
    };
    setup(0, c0, s0, n0, e0);
    setup(1, c1, s1, n1, e1);
    setup(2, c2, s2, n2, e2);
    float t = t0;
    bool active = true;
    for (int it = 0; it < 3 * R + 3; ++it) {
        const bool a0 = n0 <= n1 && n0 <= n2, a1 = !a0 && n1 <= n2, a2 = !a0 && !a1;
        const float tn = a0 ? n0 : (a1 ? n1 : n2);
        const float tout = tn <= t1 ? tn : t1;
        if (active && tout > t) {                                   // the candidate (t, tout, cell); the cell index is inside the lattice while active
            const int32_t cell = (c0 * R + c1) * R + c2;
            if (t <= hi && tout >= lo)
                carve_set(a.surface_bits, cell);
            else if (tout <= lo)
                carve_set(a.free_bits, cell);
            active = !(t > hi);                                     // everything from here on lies behind the surface
        }
        const bool last = tout >= t1;
        t = tout;
        c0 += a0 ? s0 : 0;
        c1 += a1 ? s1 : 0;
        c2 += a2 ? s2 : 0;
        const float m0 = __fadd_rn(n0, e0), m1 = __fadd_rn(n1, e1), m2 = __fadd_rn(n2, e2);
        n0 = a0 ? m0 : n0;
        n1 = a1 ? m1 : n1;
        n2 = a2 ? m2 : n2;
        const int cm = a0 ? c0 : (a1 ? c1 : c2);
        active = active && !last && (unsigned)cm < (unsigned)R;
        if (!active) break;                                         // the lane leaves; its wave goes on with the lanes that remain
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- finish
// D = surface dilated `r` times by the 26-neighbourhood = the cells within Chebyshev distance r of a surface cell (no wrap-around: a neighbour outside
// the cube does not exist); out = ~free | D (hull) or D (band).
// R >= 32: a word is 32 consecutive z of one (x, y) column, so the dilation is done on WORDS - a thread per output word ORs the (2r+1)^2 columns around
// it (its own word and the two beside it along z), then spreads the result by r bits each way with shifts: 3 (2r+1)^2 word loads for 32 cells.
__global__ __launch_bounds__(256) void carve_finish_words_kernel(const uint32_t *__restrict__ free_bits, const uint32_t *__restrict__ surface_bits,
                                                                 int level, int r, int band, uint32_t *__restrict__ out) {
    const int R = 1 << level, W = R >> 5;
    const int64_t words = (int64_t)R * R * W;
    const int64_t wi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi >= words) return;
    const int zw = (int)(wi % W), y = (int)((wi / W) % R), x = (int)(wi / ((int64_t)W * R));
    uint32_t c = 0, l = 0, h = 0;
    for (int xx = max(x - r, 0); xx <= min(x + r, R - 1); ++xx)
        for (int yy = max(y - r, 0); yy <= min(y + r, R - 1); ++yy) {
            const uint32_t *col = surface_bits + ((int64_t)xx * R + yy) * W;
            c |= col[zw];
            if (zw > 0) l |= col[zw - 1];
            if (zw + 1 < W) h |= col[zw + 1];
        }
    uint32_t acc = c;
    for (int k = 1; k <= r; ++k) acc |= (c << k) | (c >> k) | (l >> (32 - k)) | (h << (32 - k));
    out[wi] = band ? acc : (~free_bits[wi] | acc);
}

// R < 32 (at most 4096 cells): a thread per cell tests its neighbourhood bit by bit, a wave's ballot is two words of the result; the bits past R^3 of
// the last word (levels 0 and 1) are 0.
__global__ __launch_bounds__(256) void carve_finish_cells_kernel(const uint32_t *__restrict__ free_bits, const uint32_t *__restrict__ surface_bits,
                                                                 int level, int r, int band, uint32_t *__restrict__ out) {
    const int R = 1 << level, cells = R * R * R, words = max(1, cells >> 5);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    if (i < cells) {
        const int z = i % R, y = (i / R) % R, x = i / (R * R);
        bool near = false;
        for (int xx = max(x - r, 0); xx <= min(x + r, R - 1); ++xx)
            for (int yy = max(y - r, 0); yy <= min(y + r, R - 1); ++yy)
                for (int zz = max(z - r, 0); zz <= min(z + r, R - 1); ++zz) {
                    const int j = (xx * R + yy) * R + zz;
                    near = near || ((surface_bits[j >> 5] >> (j & 31)) & 1u);
                }
        keep = near || (!band && !((free_bits[i >> 5] >> (i & 31)) & 1u));
    }
    const uint64_t m = __ballot(keep);
    const int lane = threadIdx.x & 63, word = (i - lane) >> 5;
    if (lane == 0 && word < words) out[word] = (uint32_t)m;
    if (lane == 32 && word + 1 < words) out[word + 1] = (uint32_t)(m >> 32);
}

int carve_level_check(const char *name, int blas_level) {
    PAG_CHECK_ARG(blas_level >= 0 && blas_level <= 10, "%s: blas_level %d not in [0,10]", name, blas_level);
    return PAG_OK;
}

}  // namespace

extern "C" int pag_carve_rays(const float *origins, const float *dirs, const float *t_hit, int64_t N, float dist_min, float dist_max, float margin,
                              int blas_level, uint32_t *free_bits, uint32_t *surface_bits, void *stream) {
    PAG_CHECK_ARG(N >= 0, "pag_carve_rays: N < 0");
    int rc = carve_level_check("pag_carve_rays", blas_level);
    if (rc) return rc;
    PAG_CHECK_ARG(margin >= 0.0f, "pag_carve_rays: margin is negative or NaN");
    if (N == 0) return PAG_OK;
    PAG_CHECK_ARG(origins && dirs && t_hit && free_bits && surface_bits, "pag_carve_rays: NULL input/output");
    PAG_CHECK_ARG(N <= ((int64_t)1 << 31) * 256 - 256, "pag_carve_rays: N too large for one launch");
    CarveArgs a{origins, dirs, t_hit, N, blas_level, dist_min, dist_max, margin, free_bits, surface_bits};
    hipLaunchKernelGGL(carve_rays_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PAG_CHECK_LAUNCH("pag_carve_rays");
    return PAG_OK;
}

extern "C" int pag_carve_finish(const uint32_t *free_bits, const uint32_t *surface_bits, int blas_level, int dilate, int mode, uint32_t *out_bits,
                                void *stream) {
    int rc = carve_level_check("pag_carve_finish", blas_level);
    if (rc) return rc;
    PAG_CHECK_ARG(dilate >= 0 && dilate <= PAG_CARVE_MAX_DILATE, "pag_carve_finish: dilate %d not in [0,%d]", dilate, PAG_CARVE_MAX_DILATE);
    PAG_CHECK_ARG(mode == PAG_CARVE_HULL || mode == PAG_CARVE_BAND, "pag_carve_finish: unknown mode %d", mode);
    PAG_CHECK_ARG(free_bits && surface_bits && out_bits, "pag_carve_finish: NULL input/output");
    const int band = mode == PAG_CARVE_BAND;
    if (blas_level >= 5) {
        const int64_t words = ((int64_t)1 << (3 * blas_level)) >> 5;
        hipLaunchKernelGGL(carve_finish_words_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, free_bits, surface_bits,
                           blas_level, dilate, band, out_bits);
    } else {
        const int cells = 1 << (3 * blas_level);
        hipLaunchKernelGGL(carve_finish_cells_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, free_bits, surface_bits,
                           blas_level, dilate, band, out_bits);
    }
    PAG_CHECK_LAUNCH("pag_carve_finish");
    return PAG_OK;
}
