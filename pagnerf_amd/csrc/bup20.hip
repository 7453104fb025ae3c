// The BUP20 loader's device work (pagnerf_amd/bup20.py; datasets/formats/bup20.py:189-234 on agrobot_base.py:442-461 and :524-547): ground-truth label
// planes from COCO annotations, the depth filter of the detector's instance masks, and the shrink of a chunk's frames into the dataset's final tensors.
// pagnerf_amd.bup20 holds the tensor-op / NumPy forms that define every result; the kernels give the same bits.
//
//   coco_keys     one workgroup per polygon part.  A lane owns a consecutive pair of boundary points: each point comes from the closed form of its edge
//                 (the edge by binary search in the per-edge point-count prefix sums; u or v = trunc(start + s t + 0.5) in fp64, s one fp64 division, the
//                 file is built without contraction), a kept pair becomes the key X h + Y, the workgroup's keys are compacted into LDS (an LDS counter:
//                 the order is irrelevant, they are sorted next) and bitonic-sorted there, then written with their count.
//   coco_count    optional: per candidate annotation the number of covered full-resolution pixels (a ballot per wave, one integer atomic per wave).
//   coco_labels   a thread per OUTPUT pixel (y, x) reads source pixel (y f, x f): per annotation the OR over its parts of the parity of a binary search in
//                 the part's sorted keys.  semantics = min(max_label, sum of labels, restarted at an annotation whose count is H0 W0), instance = 1 + the
//                 index of the last covering annotation.  Integers only.  A frame without labels is -1.
//   pred_stats    per view and instance id (pixels, pixels with valid depth): a workgroup histogram in LDS when the ids fit, integer atomics to memory.
//   prepare       a thread per output pixel: inst' / sem' at (y f, x f), and the bilinear shrink - the four source pixels at offsets f/2 - 1 and f/2,
//                 ((0.25 a + 0.25 b) + 0.25 c) + 0.25 d in fp32 - of the image (u8 / 255f), the depth (u16 * 0.001f) and the confidences (1 where
//                 the filter removed the pixel's instance).  Every destination may be NULL; writes go to view view_offset + b.
#include "common.h"

namespace {

constexpr int COCO_SCALE = 5;

struct Point {
    int u, v;
};

// boundary point g (an index into the chunk's global point sequence) of the part whose vertices are [vb, ve)
__device__ __forceinline__ Point boundary_point(const int32_t *__restrict__ verts, const int32_t *__restrict__ point_begin, int vb, int ve, int g) {
    int lo = vb, hi = ve - 1;                                   // the last edge e in [vb, ve) with point_begin[e] <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (point_begin[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int e = lo, d = g - point_begin[e], nx = e + 1 < ve ? e + 1 : vb;
    int xs = verts[2 * e], ys = verts[2 * e + 1], xe = verts[2 * nx], ye = verts[2 * nx + 1];
    const int dx = abs(xe - xs), dy = abs(ye - ys);
    const bool xmajor = dx >= dy;
    const int len = xmajor ? dx : dy;
    if (len == 0) return Point{xs, ys};
    const bool flip = xmajor ? xs > xe : ys > ye;
    if (flip) {
        int t = xs; xs = xe; xe = t;
        t = ys; ys = ye; ye = t;
    }
    const int t = flip ? len - d : d;
    if (xmajor) {
        const double s = (double)(ye - ys) / (double)dx;
        return Point{xs + t, (int)(((double)ys + s * (double)t) + 0.5)};
    }
    const double s = (double)(xe - xs) / (double)dy;
    return Point{(int)(((double)xs + s * (double)t) + 0.5), ys + t};
}

__global__ __launch_bounds__(256) void coco_keys_kernel(pag_coco_tables t, int H, int W) {
    __shared__ int32_t sk[PAG_COCO_MAX_PART_KEYS];
    __shared__ int count;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int vb = t.part_vert_begin[p], ve = t.part_vert_begin[p + 1];
    if (ve <= vb) return;                                       // an RLE part: its keys came from the host.  Uniform for the workgroup
    const int kb = t.part_key_begin[p];
    const int cap = min(t.part_key_begin[p + 1] - kb, PAG_COCO_MAX_PART_KEYS);
    const int pb = t.point_begin[vb], npts = t.point_begin[ve] - pb;
    if (tid == 0) count = 0;
    __syncthreads();
    for (int j = 1 + tid; j < npts; j += 256) {
        const Point a = boundary_point(t.verts, t.point_begin, vb, ve, pb + j - 1), b = boundary_point(t.verts, t.point_begin, vb, ve, pb + j);
        if (a.u == b.u) continue;
        const int xd = b.u < a.u ? b.u : b.u - 1;
        if (xd < 2 || (xd - 2) % COCO_SCALE != 0) continue;
        const int X = (xd - 2) / COCO_SCALE;
        if (X > W - 1) continue;
        const int vm = min(a.v, b.v) + 2;
        const int Y = vm < 0 ? 0 : min(vm / COCO_SCALE, H);
        const int slot = atomicAdd(&count, 1);
        if (slot < cap) sk[slot] = X * H + Y;
    }
    __syncthreads();
    const int n = min(count, cap);
    int m = 1;
    while (m < n) m <<= 1;
    for (int i = n + tid; i < m; i += 256) sk[i] = INT32_MAX;
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const int32_t x = sk[i], y = sk[l];
                    if (((i & k) == 0) == (x > y)) sk[i] = y, sk[l] = x;
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < n; i += 256) t.keys[kb + i] = sk[i];
    if (tid == 0) t.part_key_count[p] = n;
}

// whether annotation a covers the pixel with column-major index q
__device__ __forceinline__ bool ann_covers(const pag_coco_tables &t, int a, int q) {
    bool cov = false;
    for (int p = t.ann_part_begin[a]; p < t.ann_part_begin[a + 1]; ++p) {
        const int32_t *k = t.keys + t.part_key_begin[p];
        int lo = 0, hi = t.part_key_count[p];                   // the number of keys <= q
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (k[mid] <= q) lo = mid + 1;
            else hi = mid;
        }
        cov |= (lo & 1) != 0;
    }
    return cov;
}

__global__ __launch_bounds__(256) void coco_count_kernel(pag_coco_tables t, int n_pixels) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int a = t.cand[blockIdx.y];
    const bool cov = q < n_pixels && ann_covers(t, a, q);
    const int c = __popcll(__ballot(cov));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&t.ann_cover[a], c);
}

__global__ __launch_bounds__(256) void coco_labels_kernel(pag_coco_tables t, int H0, int W0, int h, int w, int f, int max_label, int64_t view_offset,
                                                          int64_t *__restrict__ semantics, int64_t *__restrict__ instance) {
    const int n = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int b = blockIdx.y;
    const int64_t out = (view_offset + b) * n + p;
    int64_t sem = -1, inst = -1;
    if (t.frame_labelled[b]) {
        const int y = p / w, x = p - y * w;
        const int q = x * f * H0 + y * f;
        const int a0 = t.frame_ann_begin[b], a1 = t.frame_ann_begin[b + 1];
        int sum = 0, last = 0;
        for (int a = a0; a < a1; ++a) {
            if (t.ann_cover[a] == H0 * W0) sum = 0;
            if (ann_covers(t, a, q)) {
                sum = min(sum + t.ann_label[a], max_label);
                last = a - a0 + 1;
            }
        }
        sem = sum, inst = last;
    }
    if (semantics) semantics[out] = sem;
    if (instance) instance[out] = inst;
}

__device__ __forceinline__ bool depth_valid(uint16_t raw, float max_depth) {
    const float d = (float)raw * 0.001f;
    return d > 0.0f && d <= max_depth;
}

constexpr int STATS_LDS_IDS = 2048;        // 16 KB of (total, valid) pairs
constexpr int STATS_PER_THREAD = 8;

template <bool LDS>
__global__ __launch_bounds__(256) void pred_stats_kernel(const int32_t *__restrict__ inst, const uint16_t *__restrict__ depth, int n_pixels, float max_depth,
                                                         int n_ids, int32_t *__restrict__ counts) {
    __shared__ int32_t hist[LDS ? 2 * STATS_LDS_IDS : 1];
    const int b = blockIdx.y;
    int32_t *dst = counts + (int64_t)b * n_ids * 2;
    if (LDS) {
        for (int i = threadIdx.x; i < 2 * n_ids; i += 256) hist[i] = 0;
        __syncthreads();
    }
    const int base = blockIdx.x * (256 * STATS_PER_THREAD) + threadIdx.x;
    for (int i = 0; i < STATS_PER_THREAD; ++i) {
        const int p = base + i * 256;
        if (p >= n_pixels) break;
        const int64_t src = (int64_t)b * n_pixels + p;
        const uint32_t id = (uint32_t)inst[src];
        if (id >= (uint32_t)n_ids) continue;                    // the host sized n_ids from the ids it decoded: never taken, never out of bounds
        int32_t *c = (LDS ? hist : dst) + 2 * id;
        atomicAdd(c, 1);
        if (depth_valid(depth[src], max_depth)) atomicAdd(c + 1, 1);
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * n_ids; i += 256)
            if (hist[i]) atomicAdd(dst + i, hist[i]);
    }
}

struct Corner {
    int64_t a, b, c, d;             // source pixel indices (within the chunk) of the four taps
};

__device__ __forceinline__ float blend(float a, float b, float c, float d) { return ((0.25f * a + 0.25f * b) + 0.25f * c) + 0.25f * d; }

__device__ __forceinline__ bool id_kept(const pag_bup20_prepare_args &a, int b, int32_t id) {
    if (!a.counts || (uint32_t)id >= (uint32_t)a.n_ids) return true;
    const int32_t *c = a.counts + ((int64_t)b * a.n_ids + id) * 2;
    return 2 * (int64_t)c[1] > (int64_t)c[0];
}

// the confidence of source pixel s after the depth filter
__device__ __forceinline__ float conf_at(const pag_bup20_prepare_args &a, const float *__restrict__ conf, int b, int64_t s) {
    if (a.counts && a.inst) {
        const int32_t id = a.inst[s];
        if (id != 0 && !id_kept(a, b, id)) return 1.0f;
    }
    return conf[s];
}

template <int C0>
__global__ __launch_bounds__(256) void bup20_prepare_kernel(pag_bup20_prepare_args a, int h, int w, int f) {
    const int64_t n = (int64_t)h * w;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int b = blockIdx.y;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    const int64_t out = (a.view_offset + b) * n + p;
    const int64_t view = (int64_t)b * a.H0 * a.W0;
    const int o0 = f == 1 ? 0 : f / 2 - 1, o1 = f == 1 ? 0 : f / 2;
    Corner k;
    k.a = view + (int64_t)(y * f + o0) * a.W0 + (x * f + o0);
    k.b = view + (int64_t)(y * f + o0) * a.W0 + (x * f + o1);
    k.c = view + (int64_t)(y * f + o1) * a.W0 + (x * f + o0);
    k.d = view + (int64_t)(y * f + o1) * a.W0 + (x * f + o1);
    const int64_t near = view + (int64_t)(y * f) * a.W0 + x * f;

    if (a.imgs || a.masks) {
        float v[C0];
#pragma unroll
        for (int c = 0; c < C0; ++c) {
            const float va = (float)a.img[k.a * C0 + c] / 255.0f;
            v[c] = va;
            if (f > 1) v[c] = blend(va, (float)a.img[k.b * C0 + c] / 255.0f, (float)a.img[k.c * C0 + c] / 255.0f, (float)a.img[k.d * C0 + c] / 255.0f);
        }
        bool mask = true;
        if (C0 == 4) {
            const float al = v[3], rest = 1.0f - al;
            mask = al > 0.5f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float r = a.bg == PAG_BG_WHITE ? v[c] * al + rest : v[c] - rest;
                v[c] = fminf(fmaxf(r, 0.0f), 1.0f);
            }
        }
        if (a.imgs) {
            float *o = a.imgs + out * 3;
            o[0] = v[0], o[1] = v[1], o[2] = v[2];
        }
        if (a.masks) a.masks[out] = mask ? 1 : 0;
    }
    if (a.depths) {
        const float da = (float)a.depth[k.a] * 0.001f;
        a.depths[out] = f == 1 ? da : blend(da, (float)a.depth[k.b] * 0.001f, (float)a.depth[k.c] * 0.001f, (float)a.depth[k.d] * 0.001f);
    }
    if (a.instance_pred || a.semantics_pred) {
        int32_t id = a.inst ? a.inst[near] : 0;
        if (a.inst && id != 0 && !id_kept(a, b, id)) id = 0;
        if (a.instance_pred) a.instance_pred[out] = (int64_t)id;
        if (a.semantics_pred) a.semantics_pred[out] = (a.counts && a.inst && id == 0) ? (int64_t)0 : (int64_t)a.sem[near];
    }
    if (a.sem_conf_out) {
        const float ca = conf_at(a, a.sem_conf, b, k.a);
        a.sem_conf_out[out] = f == 1 ? ca : blend(ca, conf_at(a, a.sem_conf, b, k.b), conf_at(a, a.sem_conf, b, k.c), conf_at(a, a.sem_conf, b, k.d));
    }
    if (a.inst_conf_out) {
        const float ca = conf_at(a, a.inst_conf, b, k.a);
        a.inst_conf_out[out] = f == 1 ? ca : blend(ca, conf_at(a, a.inst_conf, b, k.b), conf_at(a, a.inst_conf, b, k.c), conf_at(a, a.inst_conf, b, k.d));
    }
}

int coco_check(const char *who, const pag_coco_tables *t, int H0, int W0) {
    PAG_CHECK_ARG(t, "%s: NULL tables", who);
    PAG_CHECK_ARG(H0 >= 1 && W0 >= 1 && ((int64_t)W0 + 1) * H0 < ((int64_t)1 << 31), "%s: image size %d x %d does not fit 32-bit keys", who, H0, W0);
    PAG_CHECK_ARG(t->B >= 0 && t->B <= 65535 && t->n_parts >= 0 && t->n_anns >= 0 && t->n_cand >= 0 && t->n_cand <= 65535,
                  "%s: B %d, n_parts %d, n_anns %d, n_cand %d", who, t->B, t->n_parts, t->n_anns, t->n_cand);
    PAG_CHECK_ARG(t->max_part_keys >= 0 && t->max_part_keys <= PAG_COCO_MAX_PART_KEYS,
                  "%s: a polygon part with up to %d keys, more than the %d the sort holds (take the tensor-op form for that image)", who, t->max_part_keys,
                  PAG_COCO_MAX_PART_KEYS);
    PAG_CHECK_ARG(t->n_parts == 0 || (t->part_vert_begin && t->point_begin && t->part_key_begin && t->part_key_count && t->keys),
                  "%s: NULL part tables", who);
    PAG_CHECK_ARG(t->n_parts == 0 || t->verts || t->n_verts == 0, "%s: NULL verts", who);
    PAG_CHECK_ARG(t->n_anns == 0 || (t->ann_part_begin && t->ann_label && t->ann_cover), "%s: NULL annotation tables", who);
    PAG_CHECK_ARG(t->n_cand == 0 || t->cand, "%s: NULL cand", who);
    return PAG_OK;
}

}  // namespace

extern "C" int pag_coco_keys(const pag_coco_tables *t, int H0, int W0, void *stream) {
    const int rc = coco_check("pag_coco_keys", t, H0, W0);
    if (rc != PAG_OK) return rc;
    if (t->n_parts == 0 || t->n_verts == 0) return PAG_OK;
    hipLaunchKernelGGL(coco_keys_kernel, dim3((unsigned)t->n_parts), dim3(256), 0, (hipStream_t)stream, *t, H0, W0);
    PAG_CHECK_LAUNCH("pag_coco_keys");
    return PAG_OK;
}

extern "C" int pag_coco_labels(const pag_coco_tables *t, int H0, int W0, int mip, int max_label, int64_t view_offset, int64_t V, int64_t *semantics,
                               int64_t *instance, void *stream) {
    const int rc = coco_check("pag_coco_labels", t, H0, W0);
    if (rc != PAG_OK) return rc;
    PAG_CHECK_ARG(mip >= 0 && mip <= 8, "pag_coco_labels: mip %d not in [0,8]", mip);
    const int f = 1 << mip;
    PAG_CHECK_ARG(H0 % f == 0 && W0 % f == 0, "pag_coco_labels: source size %d x %d is not divisible by 2^mip = %d", H0, W0, f);
    PAG_CHECK_ARG(max_label >= 0, "pag_coco_labels: max_label %d < 0", max_label);
    PAG_CHECK_ARG(view_offset >= 0 && V >= 1 && view_offset + t->B <= V, "pag_coco_labels: views [%lld, %lld) outside the destination's [0, %lld)",
                  (long long)view_offset, (long long)(view_offset + t->B), (long long)V);
    if (t->B == 0 || !(semantics || instance)) return PAG_OK;
    PAG_CHECK_ARG(t->frame_ann_begin && t->frame_labelled, "pag_coco_labels: NULL frame tables");
    const int h = H0 / f, w = W0 / f;
    hipStream_t s = (hipStream_t)stream;
    if (t->n_cand > 0) {
        hipLaunchKernelGGL(coco_count_kernel, dim3((unsigned)(((int64_t)H0 * W0 + 255) / 256), (unsigned)t->n_cand), dim3(256), 0, s, *t, H0 * W0);
        PAG_CHECK_LAUNCH("pag_coco_labels (count)");
    }
    hipLaunchKernelGGL(coco_labels_kernel, dim3((unsigned)((h * w + 255) / 256), (unsigned)t->B), dim3(256), 0, s, *t, H0, W0, h, w, f, max_label, view_offset,
                       semantics, instance);
    PAG_CHECK_LAUNCH("pag_coco_labels");
    return PAG_OK;
}

extern "C" int pag_bup20_pred_stats(const int32_t *inst, const void *depth_u16, int B, int H0, int W0, float max_depth, int n_ids, int32_t *counts,
                                    void *stream) {
    PAG_CHECK_ARG(B >= 0 && B <= 65535, "pag_bup20_pred_stats: B %d not in [0,65535]", B);
    PAG_CHECK_ARG(H0 >= 1 && W0 >= 1 && (int64_t)H0 * W0 < ((int64_t)1 << 24), "pag_bup20_pred_stats: %d x %d pixels not in [1, 2^24)", H0, W0);
    PAG_CHECK_ARG(n_ids >= 1 && n_ids <= (1 << 24), "pag_bup20_pred_stats: n_ids %d not in [1, 2^24]", n_ids);
    PAG_CHECK_ARG(max_depth > 0.0f, "pag_bup20_pred_stats: max_depth %g is not positive", (double)max_depth);
    if (B == 0) return PAG_OK;
    PAG_CHECK_ARG(inst && depth_u16 && counts, "pag_bup20_pred_stats: NULL inst / depth / counts");
    const int n = H0 * W0;
    const dim3 grid((unsigned)((n + 256 * STATS_PER_THREAD - 1) / (256 * STATS_PER_THREAD)), (unsigned)B);
    if (n_ids <= STATS_LDS_IDS)
        hipLaunchKernelGGL(pred_stats_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, inst, static_cast<const uint16_t *>(depth_u16), n, max_depth, n_ids,
                           counts);
    else
        hipLaunchKernelGGL(pred_stats_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, inst, static_cast<const uint16_t *>(depth_u16), n, max_depth,
                           n_ids, counts);
    PAG_CHECK_LAUNCH("pag_bup20_pred_stats");
    return PAG_OK;
}

extern "C" int pag_bup20_prepare(const pag_bup20_prepare_args *a, void *stream) {
    PAG_CHECK_ARG(a, "pag_bup20_prepare: NULL args");
    PAG_CHECK_ARG(a->mip >= 0 && a->mip <= 8, "pag_bup20_prepare: mip %d not in [0,8]", a->mip);
    PAG_CHECK_ARG(a->B >= 0 && a->B <= 65535, "pag_bup20_prepare: B %d not in [0,65535]", a->B);
    PAG_CHECK_ARG(a->H0 >= 1 && a->W0 >= 1, "pag_bup20_prepare: source size %d x %d < 1", a->H0, a->W0);
    const int f = 1 << a->mip;
    PAG_CHECK_ARG(a->H0 % f == 0 && a->W0 % f == 0, "pag_bup20_prepare: source size %d x %d is not divisible by 2^mip = %d", a->H0, a->W0, f);
    const int h = a->H0 / f, w = a->W0 / f;
    PAG_CHECK_ARG((int64_t)a->H0 * a->W0 <= ((int64_t)1 << 30), "pag_bup20_prepare: %lld source pixels per view, more than 2^30", (long long)a->H0 * a->W0);
    PAG_CHECK_ARG(a->view_offset >= 0 && a->V >= 1 && a->view_offset + a->B <= a->V, "pag_bup20_prepare: views [%lld, %lld) outside the destination's [0, %lld)",
                  (long long)a->view_offset, (long long)(a->view_offset + a->B), (long long)a->V);
    PAG_CHECK_ARG(a->C0 == 3 || a->C0 == 4, "pag_bup20_prepare: C0 %d is neither 3 nor 4", a->C0);
    PAG_CHECK_ARG(a->bg == PAG_BG_BLACK || a->bg == PAG_BG_WHITE, "pag_bup20_prepare: background code %d", a->bg);
    const bool any = a->imgs || a->masks || a->depths || a->semantics_pred || a->instance_pred || a->sem_conf_out || a->inst_conf_out;
    if (a->B == 0 || !any) return PAG_OK;
    PAG_CHECK_ARG(!(a->imgs || a->masks) || a->img, "pag_bup20_prepare: NULL img");
    PAG_CHECK_ARG(!a->depths || a->depth, "pag_bup20_prepare: depths without depth");
    PAG_CHECK_ARG(!a->semantics_pred || a->sem, "pag_bup20_prepare: semantics_pred without sem");
    PAG_CHECK_ARG(!a->instance_pred || a->inst, "pag_bup20_prepare: instance_pred without inst");
    PAG_CHECK_ARG(!a->sem_conf_out || a->sem_conf, "pag_bup20_prepare: sem_conf_out without sem_conf");
    PAG_CHECK_ARG(!a->inst_conf_out || a->inst_conf, "pag_bup20_prepare: inst_conf_out without inst_conf");
    PAG_CHECK_ARG(!a->counts || (a->inst && a->n_ids >= 1), "pag_bup20_prepare: counts without inst, or n_ids %d < 1", a->n_ids);
    PAG_CHECK_ARG(!a->counts || (int64_t)a->H0 * a->W0 < ((int64_t)1 << 24),
                  "pag_bup20_prepare: the keep rule 2 valid > total equals the float32 quotient rule below 2^24 pixels only, got %d x %d", a->H0, a->W0);
    const dim3 grid((unsigned)(((int64_t)h * w + 255) / 256), (unsigned)a->B), block(256);
    if (a->C0 == 3)
        hipLaunchKernelGGL(bup20_prepare_kernel<3>, grid, block, 0, (hipStream_t)stream, *a, h, w, f);
    else
        hipLaunchKernelGGL(bup20_prepare_kernel<4>, grid, block, 0, (hipStream_t)stream, *a, h, w, f);
    PAG_CHECK_LAUNCH("pag_bup20_prepare");
    return PAG_OK;
}
