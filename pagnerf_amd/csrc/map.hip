// Panoptic point-cloud map export (utils/render_map.py): the reduction of rendered rays / dense lattice rows to the kept map points.
//
// render_points_at_depth (:107-120) as tensor ops is an argmax over [n, 200] probabilities, five masks, the unprojection of every ray and three
// boolean-index gathers (one host synchronisation each) per rendered chunk; get_dense_occupied_points / generate_pc_map (:46-79, :143-169) are the
// same select without the camera.  Here a call is an ORDERED APPEND behind a running device counter (ordered_append.h: count, scan and write pass,
// three launches, no host synchronisation) with MapPred as the predicate and map_write_kernel as the write pass: ray order is kept whatever the
// chunking; rows at or past the capacity are counted and not written.  Only KEPT rays are unprojected, copy their colour and have their instance
// row read: the [n, I] rows are 800 of the ~850 bytes a ray owns at I = 200, and 50 - 95 % of the rays are dropped.
// The instance id is torch.argmax's: the first index of the maximum, a NaN counting as the maximum (the first NaN wins).  A row is read by a
// 16-lane group (four kept rows per wave pass, float4 loads where the row length and stride allow, scalar loads otherwise) and reduced with xor
// shuffles under a total order on (value, index), so the result does not depend on how the elements were spread over the lanes.
// The point is pose_points_kernel's: sum_k (o_c - t + d_c depth)[k] R[k], same op order; compiled with -ffp-contract=off.
#include "ordered_append.h"
#include "pose_common.h"

namespace {

constexpr int MAP_EMPTY = 0x7fffffff;      // index of "no element yet": loses every tie

enum { MAP_PRED_VIEWS = 0, MAP_PRED_VALUE = 1, MAP_PRED_IDS64 = 2, MAP_PRED_IDS32 = 3 };

struct MapPred {
    int mode;
    int64_t n;
    // MAP_PRED_VIEWS: density > min_density && alpha > min_alpha && hit && depth < depth_max && depth > depth_min
    const float *depth, *alpha, *density;
    const uint8_t *hit;
    float min_density, min_alpha, depth_min, depth_max;
    // MAP_PRED_VALUE: value > threshold;  MAP_PRED_IDS64 / _IDS32: id != 0
    const float *value;
    float threshold;
    const int64_t *ids64;
    const int32_t *ids32;
    __device__ __forceinline__ bool operator()(int64_t i) const {
        if (i >= n) return false;
        switch (mode) {
        case MAP_PRED_VIEWS: {
            const float d = depth[i];
            return density[i] > min_density && alpha[i] > min_alpha && hit[i] != 0 && d < depth_max && d > depth_min;
        }
        case MAP_PRED_VALUE: return value[i] > threshold;
        case MAP_PRED_IDS64: return ids64[i] != 0;
        default: return ids32[i] != 0;
        }
    }
};

// torch.argmax's order: a beats b when a is NaN and b is not, when a > b, or on equal rank (both NaN, or a == b) when its index is lower
__device__ __forceinline__ bool map_better(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

// argmax of row `row` (I elements at inst + row * stride) by the 16-lane group the calling lane belongs to; every lane of the WAVE must call it
// (the shuffles are wave-wide), groups without a row pass active = false.  -> the index, in every lane of the group.
__device__ __forceinline__ int map_group_argmax(const float *__restrict__ inst, int64_t row, int I, int64_t stride, bool vec4, bool active, int l) {
    float best = -INFINITY;
    int bi = MAP_EMPTY;
    if (active) {
        const float *r = inst + row * stride;
        if (vec4) {
            const float4 *r4 = (const float4 *)r;
            for (int j = l; j < (I >> 2); j += 16) {
                const float4 v = r4[j];
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (map_better(e[c], 4 * j + c, best, bi)) {
                        best = e[c];
                        bi = 4 * j + c;
                    }
            }
        } else {
            for (int j = l; j < I; j += 16) {
                const float v = r[j];
                if (map_better(v, j, best, bi)) {
                    best = v;
                    bi = j;
                }
            }
        }
    }
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1) {
        const float ov = __shfl_xor(best, s);
        const int oi = __shfl_xor(bi, s);
        if (map_better(ov, oi, best, bi)) {
            best = ov;
            bi = oi;
        }
    }
    return bi;
}

// ids32[row] = argmax of every row (the dense export's `argmax != 0` predicate needs all of them): 16 rows per workgroup
__global__ __launch_bounds__(OA_BLOCK) void map_argmax_kernel(const float *__restrict__ inst, int64_t n, int I, int64_t stride, int vec4,
                                                               int32_t *__restrict__ ids32) {
    const int l = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * (OA_BLOCK / 16) + (threadIdx.x >> 4);
    const bool active = row < n;
    const int bi = map_group_argmax(inst, row, I, stride, vec4 != 0, active, l);
    if (active && l == 0) ids32[row] = bi;
}

struct MapWrite {
    // views: the unprojection (params f32 [C,9], cam i32 [n_cam], base rays f32 [rays_per_camera,3]) and the colour; NULL params = plain select
    const float *params;
    int64_t C;
    const int32_t *cam;
    int64_t rays_per_camera, ray0;
    const float *oc, *dc, *rgb;
    // select: the rows to copy
    const float *points_in;
    // ids: one of inst (argmax per kept row) / ids64 / ids32, or none
    const float *inst;
    int I;
    int64_t inst_stride;
    int vec4;
    const int64_t *ids64;
    const int32_t *ids32;
    // outputs
    float *points, *color;
    int64_t *ids_out;
    int64_t cap;
};

__global__ __launch_bounds__(OA_BLOCK) void map_write_kernel(MapPred p, MapWrite w, const int64_t *__restrict__ block_offset) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    const bool keep = p(i);
    __shared__ int wc[OA_WAVES];
    __shared__ uint8_t kept_lane[OA_WAVES][PAG_WAVE];
    const OaVote vote = oa_vote(keep);
    const int rank = vote.rank, wcount = vote.wcount;
    if (lane == 0) wc[wave] = wcount;
    if (keep) kept_lane[wave][rank] = (uint8_t)lane;
    __syncthreads();
    const int64_t wbase = oa_wave_base(block_offset, wc);
    const int64_t dst = wbase + rank;
    if (keep && dst < w.cap) {
        if (w.params) {
            const int64_t g = w.ray0 + i;
            int64_t c = w.cam[g / w.rays_per_camera];
            c = c < 0 ? 0 : (c >= w.C ? w.C - 1 : c);
            const int64_t b = g % w.rays_per_camera;
            const float *prm = w.params + c * 9;
            const Rot r = rotation(prm);
            const float t = p.depth[i];
            float v[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = (w.oc[b * 3 + k] - prm[6 + k]) + w.dc[b * 3 + k] * t;
#pragma unroll
            for (int j = 0; j < 3; ++j) w.points[dst * 3 + j] = (v[0] * r.b[0][j] + v[1] * r.b[1][j]) + v[2] * r.b[2][j];
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) w.points[dst * 3 + j] = w.points_in[i * 3 + j];
        }
        if (w.color)
#pragma unroll
            for (int j = 0; j < 3; ++j) w.color[dst * 3 + j] = w.rgb[i * 3 + j];
        if (w.ids_out) {
            if (w.ids64) w.ids_out[dst] = w.ids64[i];
            else if (w.ids32) w.ids_out[dst] = w.ids32[i];
        }
    }
    if (w.inst && w.ids_out) {
        // the wave's kept rows, four per pass: group g of 16 lanes takes kept row k0 + g, whose destination is wbase + k0 + g
        const int g = lane >> 4, l = lane & 15;
        const int64_t row0 = (int64_t)blockIdx.x * OA_BLOCK + wave * PAG_WAVE;
        for (int k0 = 0; k0 < wcount; k0 += 4) {          // wcount is uniform over the wave
            const int k = k0 + g;
            const bool active = k < wcount && wbase + k < w.cap;
            const int64_t row = active ? row0 + kept_lane[wave][k] : 0;
            const int bi = map_group_argmax(w.inst, row, w.I, w.inst_stride, w.vec4 != 0, active, l);
            if (active && l == 0) w.ids_out[wbase + k] = bi;
        }
    }
}

constexpr int64_t MAP_MAX_ROWS = (int64_t)1 << 31;

int map_check_inst(const char *name, const float *inst, int I, int64_t stride) {
    if (!inst) return PAG_OK;
    PAG_CHECK_ARG(I >= 1 && I <= 1024 && stride >= I, "%s: instance rows of %d elements (1..1024) at stride %lld (>= the row length)", name, I, (long long)stride);
    return PAG_OK;
}

bool map_vec4(const float *inst, int I, int64_t stride) { return inst && I % 4 == 0 && stride % 4 == 0 && ((uintptr_t)inst & 15) == 0; }

// an append, after the all-rows argmax of the `argmax != 0` predicate into the workspace's ids32 plane (behind the append's block tables; it writes
// the workspace before oa_append has checked it, hence the check of its own)
int map_append(const char *name, MapPred p, MapWrite w, bool argmax_all, int64_t *count, void *workspace, int64_t workspace_bytes, hipStream_t st) {
    const int64_t n = p.n, nb = oa_blocks(n), need = pag_map_workspace_bytes(n);
    if (argmax_all) {
        PAG_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace smaller than pag_map_workspace_bytes(n)", name);
        int32_t *ids32 = (int32_t *)((char *)workspace + oa_align(nb * 8) + oa_align(nb * 4));
        hipLaunchKernelGGL(map_argmax_kernel, dim3((unsigned)((n + 15) / 16)), dim3(OA_BLOCK), 0, st, w.inst, n, w.I, w.inst_stride, w.vec4, ids32);
        p.ids32 = ids32;
        w.ids32 = ids32;
        w.inst = nullptr;
    }
    return oa_append(name, "pag_map_workspace_bytes(n)", need, p, count, workspace, workspace_bytes, st, [&](dim3 grid, dim3 block, const int64_t *block_offset) {
        hipLaunchKernelGGL(map_write_kernel, grid, block, 0, st, p, w, block_offset);
    });
}
}  // namespace

extern "C" int64_t pag_map_workspace_bytes(int64_t n) {
    if (n <= 0 || n > MAP_MAX_ROWS) return 0;
    const int64_t nb = oa_blocks(n);
    return oa_align(nb * 8) + oa_align(nb * 4) + oa_align(n * 4);
}

extern "C" int pag_map_points(const float *params, int64_t C, const int32_t *cam, int64_t n_cam, int64_t rays_per_camera, const float *origins_c,
                              const float *dirs_c, int64_t ray0, int64_t n, const float *depth, const float *alpha, const uint8_t *hit,
                              const float *density, const float *rgb, const float *inst, int I, int64_t inst_stride, const int64_t *ids_in,
                              float min_density, float min_alpha, float depth_min, float depth_max, float *points, float *color, int64_t *ids_out,
                              int64_t cap, int64_t *count, void *workspace, int64_t workspace_bytes, void *stream) {
    PAG_CHECK_ARG(n >= 0 && n <= MAP_MAX_ROWS && C >= 1 && C <= 65535 && n_cam >= 1 && rays_per_camera >= 1 && ray0 >= 0 && cap >= 0,
                  "pag_map_points: n %lld not in [0, 2^31], cameras %lld not in [1,65535], n_cam %lld < 1, rays_per_camera %lld < 1, ray0 %lld < 0 or cap %lld < 0",
                  (long long)n, (long long)C, (long long)n_cam, (long long)rays_per_camera, (long long)ray0, (long long)cap);
    PAG_CHECK_ARG(rays_per_camera <= MAP_MAX_ROWS && n_cam <= 65535 && ray0 + n <= n_cam * rays_per_camera,
                  "pag_map_points: rays [%lld, %lld) outside the %lld x %lld rays of the cameras", (long long)ray0, (long long)(ray0 + n), (long long)n_cam,
                  (long long)rays_per_camera);
    PAG_CHECK_ARG(!(inst && ids_in), "pag_map_points: give either inst or ids_in");
    int rc = map_check_inst("pag_map_points", inst, I, inst_stride);
    if (rc) return rc;
    if (n == 0) return PAG_OK;
    PAG_CHECK_ARG(params && cam && origins_c && dirs_c && depth && alpha && hit && density && rgb, "pag_map_points: NULL input");
    PAG_CHECK_ARG(inst || ids_in, "pag_map_points: NULL inst and ids_in");
    PAG_CHECK_ARG(count && (cap == 0 || (points && color && ids_out)), "pag_map_points: NULL counter / output");
    MapPred p = {};
    p.mode = MAP_PRED_VIEWS;
    p.n = n;
    p.depth = depth, p.alpha = alpha, p.density = density, p.hit = hit;
    p.min_density = min_density, p.min_alpha = min_alpha, p.depth_min = depth_min, p.depth_max = depth_max;
    MapWrite w = {};
    w.params = params, w.C = C, w.cam = cam, w.rays_per_camera = rays_per_camera, w.ray0 = ray0, w.oc = origins_c, w.dc = dirs_c, w.rgb = rgb;
    w.inst = inst, w.I = I, w.inst_stride = inst_stride, w.vec4 = map_vec4(inst, I, inst_stride), w.ids64 = ids_in;
    w.points = points, w.color = color, w.ids_out = ids_out, w.cap = cap;
    return map_append("pag_map_points", p, w, false, count, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int pag_map_select(const float *points_in, int64_t n, const float *value, float threshold, const float *inst, int I, int64_t inst_stride,
                              const int64_t *ids_in, float *points, int64_t *ids_out, int64_t cap, int64_t *count, void *workspace,
                              int64_t workspace_bytes, void *stream) {
    PAG_CHECK_ARG(n >= 0 && n <= MAP_MAX_ROWS && cap >= 0, "pag_map_select: n %lld not in [0, 2^31] or cap %lld < 0", (long long)n, (long long)cap);
    PAG_CHECK_ARG(!(inst && ids_in), "pag_map_select: give either inst or ids_in");
    int rc = map_check_inst("pag_map_select", inst, I, inst_stride);
    if (rc) return rc;
    if (n == 0) return PAG_OK;
    PAG_CHECK_ARG(points_in && (value || inst || ids_in), "pag_map_select: NULL points / no predicate input (value, inst or ids_in)");
    PAG_CHECK_ARG(count && (cap == 0 || points), "pag_map_select: NULL counter / output");
    MapPred p = {};
    p.n = n;
    p.mode = value ? MAP_PRED_VALUE : (ids_in ? MAP_PRED_IDS64 : MAP_PRED_IDS32);
    p.value = value, p.threshold = threshold, p.ids64 = ids_in;
    MapWrite w = {};
    w.points_in = points_in;
    w.inst = inst, w.I = I, w.inst_stride = inst_stride, w.vec4 = map_vec4(inst, I, inst_stride), w.ids64 = ids_in;
    w.points = points, w.ids_out = ids_out, w.cap = cap;
    // with a value predicate the ids (if any) are wanted for the kept rows only: map_write_kernel's per-row argmax; with the id predicate every row's
    return map_append("pag_map_select", p, w, !value && inst, count, workspace, workspace_bytes, (hipStream_t)stream);
}
