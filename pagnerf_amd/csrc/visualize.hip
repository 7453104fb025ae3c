// Validation pictures (pagnerf_amd/visualize.py; pc_nerf/trainer.py:710-829, :855-896: the per-image .cpu() / numpy chain of imgviz label_colormap,
// label2rgb, depth2rgb, torchvision masks_to_boxes / draw_bounding_boxes and the 0.7 blend as two launches).
//
// vis_stats_kernel   a workgroup covers 256 * STATS_PER_THREAD consecutive pixels.  Depth: every thread keeps the smallest / largest monotone key of
//                    its finite values, the workgroup combines them with two LDS atomics per thread, thread 0 sends the pair on with two global
//                    atomics.  Boxes: four LDS min / max atomics per labelled pixel into the workgroup's copy of the table, then the present ids of
//                    that copy go to the global table with integer atomics.  Integer min / max commute: the result does not depend on the order.
// vis_paint_kernel   a thread paints 4 consecutive pixels of every requested picture: 12 bytes per picture, stored as three dwords when the plane is
//                    4-byte aligned and all 4 pixels exist, as bytes otherwise (the tail, and planes of an image whose pixel count is no multiple
//                    of 4).  Neighbouring threads write neighbouring 12-byte pieces.  The box tables are staged in LDS with the highest present id,
//                    so that the outline search of a pixel runs from that id down and stops at the first box whose outline holds the pixel (boxes
//                    are drawn in ascending id order: the highest id is on top); every lane reads the same LDS word (a broadcast).  Workgroup 0
//                    re-initialises the other half of the workspace for the next image.
// Bytes at 720 x 1280, all inputs, int64 labels: the paint pass reads 77 MB (rgb and gt 11 MB each, depth and two confidences 3.7 MB each, six label
// images 7.4 MB each) and writes 15 * 2.76 MB; the statistics pass reads 18 MB.  Every float operation is in the written order of the tensor-op forms (no
// contraction: -ffp-contract=off), so the pictures are bit-equal to them.
#include <limits.h>
#include "common.h"

namespace {

constexpr int VIS_THREADS = 256;
constexpr int STATS_PER_THREAD = 8;
constexpr int WS_HEAD = 4;                                   // {min key, max key, 0, 0}

__host__ __device__ __forceinline__ int ws_half_words(int max_id) { return WS_HEAD + 8 * (max_id + 1); }

__device__ __forceinline__ uint32_t float_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ int64_t load_label(const void *p, int bytes, int64_t i) {
    if (bytes == 8) return static_cast<const int64_t *>(p)[i];
    if (bytes == 4) return static_cast<const int32_t *>(p)[i];
    return static_cast<const unsigned char *>(p)[i];
}

// 0x00BBGGRR of a label id: the PASCAL-VOC bit procedure on the low 24 bits, black for a negative id
__device__ __forceinline__ uint32_t label_colour(int64_t id) {
    if (id < 0) return 0u;
    uint32_t v = (uint32_t)id, r = 0, g = 0, b = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        r |= (v & 1u) << (7 - j);
        g |= ((v >> 1) & 1u) << (7 - j);
        b |= ((v >> 2) & 1u) << (7 - j);
        v >>= 3;
    }
    return r | (g << 8) | (b << 16);
}

__device__ __forceinline__ uint32_t unit_to_u8(float x) {
    const float c = fminf(fmaxf(x, 0.0f), 1.0f);             // fmaxf(NaN, 0) = 0
    return (uint32_t)(c * 255.0f);
}

__device__ __forceinline__ uint32_t table_colour(const unsigned char *__restrict__ table, int idx) {
    return (uint32_t)table[3 * idx] | ((uint32_t)table[3 * idx + 1] << 8) | ((uint32_t)table[3 * idx + 2] << 16);
}

// t clamped to [0, 1]; index min(255, floor(t * 256)); non-finite black; hi == lo index 0
__device__ __forceinline__ uint32_t ramp_colour(const unsigned char *__restrict__ table, float d, float lo, float hi) {
    if (!finite_f(d)) return 0u;
    int idx = 0;
    if (hi != lo) {
        float t = (d - lo) / (hi - lo);
        t = fminf(fmaxf(t, 0.0f), 1.0f);
        idx = (int)floorf(t * 256.0f);
        idx = idx > 255 ? 255 : idx;
    }
    return table_colour(table, idx);
}

// rint(keep * grey + alpha * colour) per channel, grey = rint(0.299 R + 0.587 G + 0.114 B) of the base picture
__device__ __forceinline__ uint32_t blend_grey(uint32_t base, uint32_t colour, float keep, float alpha) {
    const float R = (float)(base & 255u), G = (float)((base >> 8) & 255u), B = (float)((base >> 16) & 255u);
    const float grey = rintf(0.299f * R + 0.587f * G + 0.114f * B);
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = rintf(keep * grey + alpha * (float)((colour >> (8 * c)) & 255u));
        out |= ((uint32_t)v & 255u) << (8 * c);
    }
    return out;
}

// per channel where the label colour's channel is non-zero: trunc(keep * base + alpha * colour)
__device__ __forceinline__ uint32_t overlay(uint32_t base, uint32_t colour, float keep, float alpha) {
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t b = (base >> (8 * c)) & 255u, l = (colour >> (8 * c)) & 255u;
        const uint32_t v = l ? (uint32_t)(keep * (float)b + alpha * (float)l) : b;
        out |= (v & 255u) << (8 * c);
    }
    return out;
}

// the id in [1, hi] whose box outline holds (x, y), the highest one; 0 when none does.  boxes: LDS, (x0, y0, x1, y1) per id
__device__ __forceinline__ int outline_id(const int *boxes, int hi, int x, int y, int width) {
    for (int id = hi; id >= 1; --id) {
        const int4 b = reinterpret_cast<const int4 *>(boxes)[id];          // both tables start on a 16-byte boundary of the LDS block
        const int x0 = b.x, y0 = b.y, x1 = b.z, y1 = b.w;
        if (x >= x0 && x <= x1 && y >= y0 && y <= y1 && (x - x0 < width || x1 - x < width || y - y0 < width || y1 - y < width)) return id;
    }
    return 0;
}

__device__ __forceinline__ void store4(unsigned char *__restrict__ plane, int64_t i0, int n, const uint32_t c[4]) {
    unsigned char *p = plane + 3 * i0;
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
        uint32_t *w = reinterpret_cast<uint32_t *>(p);
        w[0] = (c[0] & 0xffffffu) | (c[1] << 24);
        w[1] = ((c[1] >> 8) & 0xffffu) | (c[2] << 16);
        w[2] = ((c[2] >> 16) & 0xffu) | (c[3] << 8);
        return;
    }
    for (int k = 0; k < n; ++k) {
        p[3 * k] = (unsigned char)(c[k] & 255u);
        p[3 * k + 1] = (unsigned char)((c[k] >> 8) & 255u);
        p[3 * k + 2] = (unsigned char)((c[k] >> 16) & 255u);
    }
}

struct StatsArgs {
    const float *depth;
    const void *labels[2];
    int label_bytes[2];
    int W, max_id;
    int64_t HW;
    int32_t *ws;                                             // the half to reduce into
};

__global__ __launch_bounds__(VIS_THREADS) void vis_stats_kernel(StatsArgs a) {
    extern __shared__ __attribute__((aligned(16))) int lds[];          // {min key, max key, 0, 0}, box table 0, box table 1
    const int ids = a.max_id + 1, words = ws_half_words(a.max_id);
    for (int i = threadIdx.x; i < words; i += VIS_THREADS) lds[i] = i == 0 ? -1 : i < WS_HEAD ? 0 : ((i - WS_HEAD) & 2) ? -1 : INT_MAX;
    __syncthreads();
    uint32_t kmin = 0xffffffffu, kmax = 0u;
    const int64_t begin = (int64_t)blockIdx.x * (VIS_THREADS * STATS_PER_THREAD);
    for (int j = 0; j < STATS_PER_THREAD; ++j) {
        const int64_t i = begin + (int64_t)j * VIS_THREADS + threadIdx.x;
        if (i >= a.HW) break;
        if (a.depth) {
            const float d = a.depth[i];
            if (finite_f(d)) {
                const uint32_t k = float_key(d);
                kmin = k < kmin ? k : kmin;
                kmax = k > kmax ? k : kmax;
            }
        }
        const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
        for (int t = 0; t < 2; ++t) {
            if (!a.labels[t]) continue;
            const int64_t id = load_label(a.labels[t], a.label_bytes[t], i);
            if (id < 1 || id > a.max_id) continue;
            int *box = lds + WS_HEAD + 4 * (t * ids + (int)id);          // id <= max_id: inside the table
            atomicMin(box, x);
            atomicMin(box + 1, y);
            atomicMax(box + 2, x);
            atomicMax(box + 3, y);
        }
    }
    if (a.depth && kmin <= kmax) {
        atomicMin(reinterpret_cast<unsigned int *>(lds), kmin);
        atomicMax(reinterpret_cast<unsigned int *>(lds) + 1, kmax);
    }
    __syncthreads();
    if (threadIdx.x == 0 && a.depth && (uint32_t)lds[0] <= (uint32_t)lds[1]) {
        atomicMin(reinterpret_cast<unsigned int *>(a.ws), (uint32_t)lds[0]);
        atomicMax(reinterpret_cast<unsigned int *>(a.ws) + 1, (uint32_t)lds[1]);
    }
    for (int b = threadIdx.x; b < 2 * ids; b += VIS_THREADS) {
        const int *box = lds + WS_HEAD + 4 * b;
        if (box[0] > box[2]) continue;                                  // the id has no pixel in this workgroup
        int32_t *g = a.ws + WS_HEAD + 4 * b;
        atomicMin(g, box[0]);
        atomicMin(g + 1, box[1]);
        atomicMax(g + 2, box[2]);
        atomicMax(g + 3, box[3]);
    }
}

struct PaintArgs {
    pag_vis_args v;
    int64_t HW;
    const int32_t *ws;                                       // the half the statistics pass filled
    int32_t *ws_next;                                        // the half to re-initialise
};

__global__ __launch_bounds__(VIS_THREADS) void vis_paint_kernel(PaintArgs a) {
    extern __shared__ __attribute__((aligned(16))) int lds[];          // box table 0, box table 1, then the highest present id of each
    const pag_vis_args &v = a.v;
    const int ids = v.max_id + 1;
    const bool boxes0 = v.out[PAG_VIS_INST_RGB] != nullptr, boxes1 = v.out[PAG_VIS_INST_PRED_RGB] != nullptr;
    int *top = lds + 8 * ids;
    if (boxes0 || boxes1) {
        if (threadIdx.x < 2) top[threadIdx.x] = 0;
        __syncthreads();
        for (int b = threadIdx.x; b < 2 * ids; b += VIS_THREADS) {
            if (!(b < ids ? boxes0 : boxes1)) continue;
            const int32_t *g = a.ws + WS_HEAD + 4 * b;
            const int x0 = g[0], x1 = g[2];
            lds[4 * b] = x0;
            lds[4 * b + 1] = g[1];
            lds[4 * b + 2] = x1;
            lds[4 * b + 3] = g[3];
            const int id = b < ids ? b : b - ids;
            if (x0 <= x1 && id >= 1) atomicMax(top + (b < ids ? 0 : 1), id);
        }
        __syncthreads();
    }
    if (blockIdx.x == 0) {
        const int words = ws_half_words(v.max_id);
        for (int i = threadIdx.x; i < words; i += VIS_THREADS) a.ws_next[i] = i == 0 ? -1 : i < WS_HEAD ? 0 : ((i - WS_HEAD) & 2) ? -1 : INT_MAX;
    }
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * VIS_THREADS + threadIdx.x);
    if (i0 >= a.HW) return;
    const int n = a.HW - i0 < 4 ? (int)(a.HW - i0) : 4;
    uint32_t base[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0};

    if (v.rgb) {
        for (int k = 0; k < n; ++k) {
            const int64_t e = (i0 + k) * v.rgb_stride;
            if (v.rgb_is_u8) {
                const unsigned char *p = static_cast<const unsigned char *>(v.rgb) + e;
                base[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
            } else {
                const float *p = static_cast<const float *>(v.rgb) + e;
                base[k] = unit_to_u8(p[0]) | (unit_to_u8(p[1]) << 8) | (unit_to_u8(p[2]) << 16);
            }
        }
        if (v.out[PAG_VIS_RGB]) store4(v.out[PAG_VIS_RGB], i0, n, base);
    }
    if (v.out[PAG_VIS_GT]) {
        for (int k = 0; k < n; ++k) {
            const float *p = v.gt + (i0 + k) * v.gt_stride;
            c[k] = unit_to_u8(p[0]) | (unit_to_u8(p[1]) << 8) | (unit_to_u8(p[2]) << 16);
        }
        store4(v.out[PAG_VIS_GT], i0, n, c);
    }
    if (v.out[PAG_VIS_DEPTH]) {
        const uint32_t klo = (uint32_t)a.ws[0], khi = (uint32_t)a.ws[1];
        const float lo = klo <= khi ? key_float(klo) : 0.0f, hi = klo <= khi ? key_float(khi) : 0.0f;     // no finite value: every pixel is black
        for (int k = 0; k < n; ++k) c[k] = ramp_colour(v.table, v.depth[i0 + k], lo, hi);
        store4(v.out[PAG_VIS_DEPTH], i0, n, c);
    }
    for (int t = 0; t < 2; ++t) {
        const int pic = t ? PAG_VIS_INST_CONF_PRED : PAG_VIS_INST_CONF;
        if (!v.out[pic]) continue;
        for (int k = 0; k < n; ++k) c[k] = ramp_colour(v.table, v.conf[t][i0 + k], v.conf_min, v.conf_max);
        store4(v.out[pic], i0, n, c);
    }
    // the label pictures: colour, and for the semantic images the grey blend
    const int colour_pic[PAG_VIS_LABELS] = {PAG_VIS_SEM, PAG_VIS_INST, PAG_VIS_SEM_GT, PAG_VIS_INST_GT, PAG_VIS_SEM_PRED, PAG_VIS_INST_PRED};
    const int second_pic[PAG_VIS_LABELS] = {PAG_VIS_SEM_RGB, PAG_VIS_INST_RGB, -1, -1, PAG_VIS_SEM_PRED_RGB, PAG_VIS_INST_PRED_RGB};
#pragma unroll
    for (int l = 0; l < PAG_VIS_LABELS; ++l) {
        unsigned char *first = v.out[colour_pic[l]];
        unsigned char *second = second_pic[l] >= 0 ? v.out[second_pic[l]] : nullptr;
        if (!first && !second) continue;
        for (int k = 0; k < n; ++k) c[k] = label_colour(load_label(v.labels[l], v.label_bytes[l], i0 + k));
        if (first) store4(first, i0, n, c);
        if (!second) continue;
        if (l == PAG_VIS_L_SEM || l == PAG_VIS_L_SEM_PRED) {
            for (int k = 0; k < n; ++k) c[k] = blend_grey(base[k], c[k], v.blend_keep, v.blend_alpha);
        } else {
            const int t = l == PAG_VIS_L_INST ? 0 : 1;
            const int *boxes = lds + 4 * t * ids;
            const int hi = top[t];
            for (int k = 0; k < n; ++k) {
                const int64_t i = i0 + k;
                const int y = (int)(i / v.W), x = (int)(i - (int64_t)y * v.W);
                const int id = outline_id(boxes, hi, x, y, v.box_width);
                c[k] = overlay(id ? label_colour(id) : base[k], c[k], v.overlay_keep, v.overlay_alpha);
            }
        }
        store4(second, i0, n, c);
    }
}

int check_common(const pag_vis_args *a, const char *who) {
    PAG_CHECK_ARG(a, "%s: NULL args", who);
    PAG_CHECK_ARG(a->H >= 1 && a->W >= 1 && (int64_t)a->H * a->W * 3 < ((int64_t)1 << 31), "%s: image %d x %d outside [1, 2^31 / 3 pixels)", who, a->H, a->W);
    PAG_CHECK_ARG(a->max_id >= 1 && a->max_id <= PAG_VIS_MAX_ID, "%s: max_id %d not in [1,%d]", who, a->max_id, PAG_VIS_MAX_ID);
    PAG_CHECK_ARG(a->phase == 0 || a->phase == 1, "%s: phase %d not 0 / 1", who, a->phase);
    PAG_CHECK_ARG(a->workspace && a->workspace_bytes >= pag_vis_workspace_bytes(a->max_id), "%s: workspace NULL or shorter than %lld bytes", who,
                  (long long)pag_vis_workspace_bytes(a->max_id));
    for (int l = 0; l < PAG_VIS_LABELS; ++l)
        PAG_CHECK_ARG(!a->labels[l] || a->label_bytes[l] == 8 || a->label_bytes[l] == 4 || a->label_bytes[l] == 1, "%s: label image %d: %d bytes per label (8, 4 or 1)",
                      who, l, a->label_bytes[l]);
    return PAG_OK;
}

}  // namespace

extern "C" int64_t pag_vis_workspace_bytes(int max_id) {
    if (max_id < 1 || max_id > PAG_VIS_MAX_ID) return 0;
    return (int64_t)2 * ws_half_words(max_id) * (int64_t)sizeof(int32_t);
}

extern "C" int pag_vis_stats(const pag_vis_args *a, void *stream) {
    const int rc = check_common(a, "pag_vis_stats");
    if (rc != PAG_OK) return rc;
    if (!a->depth && !a->labels[PAG_VIS_L_INST] && !a->labels[PAG_VIS_L_INST_PRED]) return PAG_OK;
    StatsArgs s = {};
    s.depth = a->depth;
    s.labels[0] = a->labels[PAG_VIS_L_INST];
    s.labels[1] = a->labels[PAG_VIS_L_INST_PRED];
    s.label_bytes[0] = a->label_bytes[PAG_VIS_L_INST];
    s.label_bytes[1] = a->label_bytes[PAG_VIS_L_INST_PRED];
    s.W = a->W;
    s.max_id = a->max_id;
    s.HW = (int64_t)a->H * a->W;
    s.ws = a->workspace + (int64_t)a->phase * ws_half_words(a->max_id);
    const int64_t per_block = VIS_THREADS * STATS_PER_THREAD;
    const unsigned blocks = (unsigned)((s.HW + per_block - 1) / per_block);
    hipLaunchKernelGGL(vis_stats_kernel, dim3(blocks), dim3(VIS_THREADS), (size_t)ws_half_words(a->max_id) * sizeof(int), (hipStream_t)stream, s);
    PAG_CHECK_LAUNCH("pag_vis_stats");
    return PAG_OK;
}

extern "C" int pag_vis_paint(const pag_vis_args *a, void *stream) {
    const int rc = check_common(a, "pag_vis_paint");
    if (rc != PAG_OK) return rc;
    unsigned char *const *o = a->out;
    const bool needs_rgb = o[PAG_VIS_RGB] || o[PAG_VIS_SEM_RGB] || o[PAG_VIS_SEM_PRED_RGB] || o[PAG_VIS_INST_RGB] || o[PAG_VIS_INST_PRED_RGB];
    PAG_CHECK_ARG(!needs_rgb || (a->rgb && a->rgb_stride >= 3), "pag_vis_paint: a picture needs rgb (NULL, or rgb_stride %d < 3)", a->rgb_stride);
    PAG_CHECK_ARG(!o[PAG_VIS_GT] || (a->gt && a->gt_stride >= 3), "pag_vis_paint: the gt picture needs gt (NULL, or gt_stride %d < 3)", a->gt_stride);
    PAG_CHECK_ARG(!o[PAG_VIS_DEPTH] || a->depth, "pag_vis_paint: the depth picture needs depth");
    PAG_CHECK_ARG(!(o[PAG_VIS_DEPTH] || o[PAG_VIS_INST_CONF] || o[PAG_VIS_INST_CONF_PRED]) || a->table, "pag_vis_paint: NULL colour table");
    PAG_CHECK_ARG((!o[PAG_VIS_INST_CONF] || a->conf[0]) && (!o[PAG_VIS_INST_CONF_PRED] || a->conf[1]), "pag_vis_paint: a confidence picture without its confidence");
    PAG_CHECK_ARG((!o[PAG_VIS_SEM] && !o[PAG_VIS_SEM_RGB]) || a->labels[PAG_VIS_L_SEM], "pag_vis_paint: sem / sem_rgb need the semantics");
    PAG_CHECK_ARG((!o[PAG_VIS_INST] && !o[PAG_VIS_INST_RGB]) || a->labels[PAG_VIS_L_INST], "pag_vis_paint: inst / inst_rgb need the instances");
    PAG_CHECK_ARG(!o[PAG_VIS_SEM_GT] || a->labels[PAG_VIS_L_SEM_GT], "pag_vis_paint: sem_gt needs its labels");
    PAG_CHECK_ARG(!o[PAG_VIS_INST_GT] || a->labels[PAG_VIS_L_INST_GT], "pag_vis_paint: inst_gt needs its labels");
    PAG_CHECK_ARG((!o[PAG_VIS_SEM_PRED] && !o[PAG_VIS_SEM_PRED_RGB]) || a->labels[PAG_VIS_L_SEM_PRED], "pag_vis_paint: sem_pred / sem_pred_rgb need their labels");
    PAG_CHECK_ARG((!o[PAG_VIS_INST_PRED] && !o[PAG_VIS_INST_PRED_RGB]) || a->labels[PAG_VIS_L_INST_PRED], "pag_vis_paint: inst_pred / inst_pred_rgb need their labels");
    PAG_CHECK_ARG(a->box_width >= 1 || (!o[PAG_VIS_INST_RGB] && !o[PAG_VIS_INST_PRED_RGB]), "pag_vis_paint: box_width %d < 1", a->box_width);
    PaintArgs p = {};
    p.v = *a;
    p.HW = (int64_t)a->H * a->W;
    const int half = ws_half_words(a->max_id);
    p.ws = a->workspace + (int64_t)a->phase * half;
    p.ws_next = a->workspace + (int64_t)(a->phase ^ 1) * half;
    const int64_t per_block = VIS_THREADS * 4;
    const unsigned blocks = (unsigned)((p.HW + per_block - 1) / per_block);
    hipLaunchKernelGGL(vis_paint_kernel, dim3(blocks), dim3(VIS_THREADS), (size_t)(8 * (a->max_id + 1) + 2) * sizeof(int), (hipStream_t)stream, p);
    PAG_CHECK_LAUNCH("pag_vis_paint");
    return PAG_OK;
}
