// Panoptic evaluation of a validation image on the device: the instance cleanup of pc_nerf/trainer.py:750-772, the panoptic quality update of
// utils/metrics/panoptic_quality{,_func}.py and the confusion matrix behind the semantic IoU (trainer.py:670-671, :720).
//
// The reference builds one [K, H, W] mask per instance id for the cleanup and loops in Python over every (pred, target) segment pair for PQ, with a
// host round trip per pair.  Here every pass is a pixel pass or a pass over a hash table sized from the pixel count; nothing is read back, no float
// atomics are used, and every sum is an integer sum, so two runs are bitwise identical and the calls can be captured in a graph.
//
// Hash tables: open addressing with linear probing over u64 keys (PN_EMPTY = all ones), capacity N + N/4 + 64 for N pixels, so one segment per pixel
// still fits.  Pixel passes aggregate per wave first: the lanes that share a key elect a leader, which inserts once and adds the lane count (labels are
// spatially coherent, so a wave of 64 pixels of one row usually holds one to three keys).
//
//   pq_max_kernel       per-image maximum of the raw instance channel (B > 1 only: the cumulative batch offsets of _make_instance_ids_batch_unique)
//   pq_seg_kernel       per pixel: the preprocessed (category, instance) colour of pred and target (_prepocess_image), inserted into the pred and the
//                       target segment table (area counts); the two slots are kept per pixel
//   pq_pair_kernel      per pixel: the (pred slot, target slot) pair inserted into the pair table (intersection counts)
//   pq_match_kernel     per pair: non-void target, same category, IoU = f32(inter) / f32(union) > 0.5 -> tp, the IoU as an exact integer multiple of
//                       2^-24, and the matched bits of both segments
//   pq_unmatched_kernel per segment: unmatched, non-void and not mostly void -> fn (target table) / fp (pred table)
//   pq_commit_kernel    the call's sums added to the metric state (skipped when an unknown pred category is found and not allowed)
//
//   cl_min_kernel       background id = the smallest id of the image
//   cl_open_kernel      flat 3x3 opening of every non-background id as one 5x5 stencil on an LDS tile with a 2-pixel halo; the surviving pixels'
//                       exact integer moments (n, sum y, sum x, sum y^2, sum x^2) per id
//   cl_centre_kernel    per id: centre of mass and mean squared distance in fp64
//   cl_dist_kernel      per pixel: the distance to its centre, summed per id in 2^-20 fixed point
//   cl_thresh_kernel    per id: mean + std_threshold * std of the distances
//   cl_keep_kernel      per pixel: kept if its distance <= the threshold; survivors counted per id
//   cl_out_kernel       id where the pixel survived and its id keeps >= min_area pixels, else the background id
//
//   cm_kernel           confusion matrix [target, pred] of the semantic labels: LDS histogram per workgroup for C <= 64, wave-aggregated global
//                       atomics above
#include "common.h"

namespace {

constexpr unsigned long long PN_EMPTY = ~0ull;
constexpr int PN_MAX_CATS = 1024;
constexpr int64_t PN_MAX_PIXELS = 1ll << 28;
constexpr int64_t PN_MAX_SIDE = 1ll << 15;
constexpr uint32_t PN_MATCHED = 0x80000000u;
constexpr uint32_t PN_COUNT = 0x7fffffffu;
constexpr int PN_FLAG_UNKNOWN_PRED = 1;
constexpr int PN_FLAG_INST_RANGE = 2;
constexpr int CL_TW = 64, CL_TH = 4;          // cleanup tile: one wave per tile row
constexpr double CL_FIX = 1048576.0;          // 2^20: fixed-point scale of the distance sums

__host__ __device__ inline int64_t pn_align(int64_t x) { return (x + 255) / 256 * 256; }
__host__ __device__ inline int64_t pn_cap(int64_t n) { return n + n / 4 + 64; }

__device__ __forceinline__ uint32_t pn_slot(unsigned long long key, uint32_t cap) {
    unsigned long long h = key;                                  // splitmix64 finaliser, then a multiply-shift onto [0, cap)
    h ^= h >> 30; h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27; h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    return (uint32_t)__umul64hi(h, (unsigned long long)cap);
}

// Keys only ever go from PN_EMPTY to their final value, so a stale read of PN_EMPTY just costs a failed CAS.  The tables hold more slots than there
// are pixels, so a probe always ends; the bound on the probe count only guards against a workspace that was not initialised.
__device__ uint32_t pn_insert(unsigned long long *keys, uint32_t cap, unsigned long long key) {
    uint32_t s = pn_slot(key, cap);
    for (uint32_t probes = 0; probes < cap; ++probes) {
        unsigned long long k = __atomic_load_n(&keys[s], __ATOMIC_RELAXED);
        if (k == key) return s;
        if (k == PN_EMPTY) {
            k = atomicCAS(&keys[s], PN_EMPTY, key);
            if (k == PN_EMPTY || k == key) return s;
        }
        s = s + 1 == cap ? 0 : s + 1;
    }
    return 0;
}

// Lookup after every insertion has finished (a later launch): the slot, or -1.
__device__ int64_t pn_find(const unsigned long long *keys, uint32_t cap, unsigned long long key) {
    uint32_t s = pn_slot(key, cap);
    for (uint32_t probes = 0; probes < cap; ++probes) {
        const unsigned long long k = keys[s];
        if (k == key) return s;
        if (k == PN_EMPTY) return -1;
        s = s + 1 == cap ? 0 : s + 1;
    }
    return -1;
}

__device__ __forceinline__ int64_t pn_ld(const void *p, int dtype, int64_t e) {
    return dtype == PAG_I64 ? reinterpret_cast<const int64_t *>(p)[e] : (int64_t)reinterpret_cast<const int32_t *>(p)[e];
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Insert `key` for every active lane (one insert per distinct key of the wave), add the lane count to counts[slot] and return the lane's slot.  Must
// be called by all 64 lanes.
__device__ uint32_t pn_wave_insert_count(unsigned long long *keys, uint32_t *counts, uint32_t cap, unsigned long long key, bool active) {
    const int lane = __lane_id();
    unsigned long long pending = __ballot(active);
    uint32_t mine = 0;
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const unsigned long long lk = __shfl(key, leader);
        const bool match = active && key == lk;
        const unsigned long long m = __ballot(match);
        uint32_t slot = 0;
        if (lane == leader) {
            slot = pn_insert(keys, cap, lk);
            atomicAdd(&counts[slot], (uint32_t)__popcll(m));
        }
        slot = __shfl(slot, leader);
        if (match) mine = slot;
        pending &= ~m;
    }
    return mine;
}

// ================================================================================================ panoptic quality
struct PqWs {
    int32_t *flags;                  // [1] this call's flags (the first bytes of the workspace: the host reads them when unknown preds raise)
    long long *maxp, *maxt;          // [B] raw per-image instance maxima
    uint32_t *tp, *fp, *fn;          // [n_cat] this call's counts
    unsigned long long *iou;         // [n_cat] this call's IoU sums in units of 2^-24
    unsigned long long *kp, *kt, *kx;   // [cap] keys: pred segments, target segments, pairs
    uint32_t *cp, *ct, *cx;          // [cap] counts (bit 31 of cp / ct: matched)
    int32_t *sp, *st;                // [N] per-pixel slots
};

__host__ inline int64_t pq_ws_bytes(int B, int64_t N, int n_cat) {
    const int64_t cap = pn_cap(N);
    return pn_align(16 + 16 * (int64_t)B + 3 * 4 * n_cat + 8 * n_cat) + pn_align(3 * 8 * cap) + pn_align(3 * 4 * cap) + 2 * pn_align(4 * N);
}

__host__ inline PqWs pq_ws(void *base, int B, int64_t N, int n_cat, int64_t *head_bytes, int64_t *key_bytes, int64_t *count_bytes) {
    const int64_t cap = pn_cap(N);
    unsigned char *p = reinterpret_cast<unsigned char *>(base);
    PqWs w;
    w.flags = reinterpret_cast<int32_t *>(p);
    w.maxp = reinterpret_cast<long long *>(p + 16);
    w.maxt = w.maxp + B;
    w.iou = reinterpret_cast<unsigned long long *>(w.maxt + B);
    w.tp = reinterpret_cast<uint32_t *>(w.iou + n_cat);
    w.fp = w.tp + n_cat;
    w.fn = w.fp + n_cat;
    *head_bytes = pn_align(16 + 16 * (int64_t)B + 3 * 4 * n_cat + 8 * n_cat);
    p += *head_bytes;
    w.kp = reinterpret_cast<unsigned long long *>(p);
    w.kt = w.kp + cap;
    w.kx = w.kt + cap;
    *key_bytes = pn_align(3 * 8 * cap);
    p += *key_bytes;
    w.cp = reinterpret_cast<uint32_t *>(p);
    w.ct = w.cp + cap;
    w.cx = w.ct + cap;
    *count_bytes = pn_align(3 * 4 * cap);
    p += *count_bytes;
    w.sp = reinterpret_cast<int32_t *>(p);
    p += pn_align(4 * N);
    w.st = reinterpret_cast<int32_t *>(p);
    return w;
}

struct PqImg {
    const void *ptr;
    int dtype;
    int64_t s[4];                    // element strides of [B, 2, H, W]
};

__global__ void pq_init_kernel(PqWs w, int B) {
    for (int i = threadIdx.x; i < B; i += blockDim.x) w.maxp[i] = w.maxt[i] = INT64_MIN;
}

__global__ __launch_bounds__(256) void pq_max_kernel(PqImg P, PqImg T, int64_t H, int64_t W, PqWs w) {
    const int b = blockIdx.y;
    const int64_t HW = H * W;
    long long mp = INT64_MIN, mt = INT64_MIN;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / W, x = i - y * W;
        const long long vp = pn_ld(P.ptr, P.dtype, b * P.s[0] + P.s[1] + y * P.s[2] + x * P.s[3]);
        const long long vt = pn_ld(T.ptr, T.dtype, b * T.s[0] + T.s[1] + y * T.s[2] + x * T.s[3]);
        mp = vp > mp ? vp : mp;
        mt = vt > mt ? vt : mt;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const long long a = __shfl_xor(mp, o), c = __shfl_xor(mt, o);
        mp = a > mp ? a : mp;
        mt = c > mt ? c : mt;
    }
    if (__lane_id() == 0) {
        atomicMax(&w.maxp[b], mp);
        atomicMax(&w.maxt[b], mt);
    }
}

// Category rank of a raw id in the sorted table (binary search), -1 when it is neither a thing nor a stuff.
__device__ __forceinline__ int pq_rank(const long long *cats, int n_cat, long long c) {
    int lo = 0, hi = n_cat;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cats[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_cat && cats[lo] == c ? lo : -1;
}

// _prepocess_image for one pixel -> segment key (rank << 32 | instance as u32); void = (n_cat << 32 | 0).
__device__ __forceinline__ unsigned long long pq_key(const long long *cats, const uint8_t *stuff, int n_cat, long long c, long long inst, long long off,
                                                     int *flags, bool is_pred) {
    const int r = pq_rank(cats, n_cat, c);
    if (r < 0) {
        if (is_pred) *flags |= PN_FLAG_UNKNOWN_PRED;
        return (unsigned long long)n_cat << 32;
    }
    if (stuff[r]) return (unsigned long long)r << 32;
    const long long v = inst + off;
    if (v < INT32_MIN || v > INT32_MAX) {
        *flags |= PN_FLAG_INST_RANGE;
        return (unsigned long long)r << 32;
    }
    return ((unsigned long long)r << 32) | (uint32_t)(int32_t)v;
}

__global__ __launch_bounds__(256) void pq_seg_kernel(PqImg P, PqImg T, int B, int64_t H, int64_t W, const long long *cats, const int32_t *cont, int n_cat,
                                                     int n_things, PqWs w, uint32_t cap) {
    __shared__ long long s_cat[PN_MAX_CATS];
    __shared__ uint8_t s_stuff[PN_MAX_CATS];
    __shared__ int s_flags;
    for (int i = threadIdx.x; i < n_cat; i += blockDim.x) {
        s_cat[i] = cats[i];
        s_stuff[i] = cont[i] >= n_things;
    }
    if (threadIdx.x == 0) s_flags = 0;
    __syncthreads();
    const int64_t HW = H * W, N = (int64_t)B * HW;
    int flags = 0;
    const int lane = __lane_id();
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < N; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        const bool on = i < N;
        unsigned long long kp = 0, kt = 0;
        if (on) {
            const int64_t b = i / HW, r = i - b * HW, y = r / W, x = r - y * W;
            long long op = 0, ot = 0;
            for (int j = 0; j < b; ++j) {                      // cumulative offsets: arr[b+1,1] += arr[b,1].max() over the raw instance channel
                op += w.maxp[j];
                ot += w.maxt[j];
            }
            const int64_t ep = b * P.s[0] + y * P.s[2] + x * P.s[3], et = b * T.s[0] + y * T.s[2] + x * T.s[3];
            kp = pq_key(s_cat, s_stuff, n_cat, pn_ld(P.ptr, P.dtype, ep), pn_ld(P.ptr, P.dtype, ep + P.s[1]), op, &flags, true);
            kt = pq_key(s_cat, s_stuff, n_cat, pn_ld(T.ptr, T.dtype, et), pn_ld(T.ptr, T.dtype, et + T.s[1]), ot, &flags, false);
        }
        const uint32_t sp = pn_wave_insert_count(w.kp, w.cp, cap, kp, on);
        const uint32_t st = pn_wave_insert_count(w.kt, w.ct, cap, kt, on);
        if (on) {
            w.sp[i] = (int32_t)sp;
            w.st[i] = (int32_t)st;
        }
    }
    if (flags) atomicOr(&s_flags, flags);
    __syncthreads();
    if (threadIdx.x == 0 && s_flags) atomicOr(w.flags, s_flags);
}

__global__ __launch_bounds__(256) void pq_pair_kernel(int64_t N, PqWs w, uint32_t cap) {
    const int lane = __lane_id();
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < N; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        const bool on = i < N;
        const unsigned long long k = on ? ((unsigned long long)(uint32_t)w.sp[i] << 32) | (uint32_t)w.st[i] : 0;
        pn_wave_insert_count(w.kx, w.cx, cap, k, on);
    }
}

__device__ __forceinline__ uint32_t pq_inter(const PqWs &w, uint32_t cap, int64_t sp, int64_t st) {
    if (sp < 0 || st < 0) return 0;
    const int64_t s = pn_find(w.kx, cap, ((unsigned long long)sp << 32) | (unsigned long long)st);
    return s < 0 ? 0 : w.cx[s];
}

// The reference's int64 tensor divisions yield float32: both operands are converted to f32, then divided (correctly rounded; no fast math here).
__device__ __forceinline__ float pq_div(long long a, long long b) { return (float)a / (float)b; }

__global__ __launch_bounds__(256) void pq_match_kernel(PqWs w, uint32_t cap, const int32_t *cont, int n_cat) {
    const unsigned long long void_key = (unsigned long long)n_cat << 32;
    const int64_t void_p = pn_find(w.kp, cap, void_key), void_t = pn_find(w.kt, cap, void_key);
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = w.kx[s];
        if (k == PN_EMPTY) continue;
        const uint32_t sp = (uint32_t)(k >> 32), st = (uint32_t)k;
        const unsigned long long tkey = w.kt[st], pkey = w.kp[sp];
        if ((tkey >> 32) == (unsigned long long)n_cat || (pkey >> 32) != (tkey >> 32)) continue;   // void target, or another category
        const long long inter = w.cx[s];
        const long long pred_area = w.cp[sp] & PN_COUNT, target_area = w.ct[st] & PN_COUNT;
        const long long pred_void = pq_inter(w, cap, sp, void_t), void_target = pq_inter(w, cap, void_p, st);
        const long long uni = pred_area - pred_void + target_area - void_target - inter;
        const float iou = pq_div(inter, uni);
        if (iou > 0.5f) {
            const int c = cont[(int)(tkey >> 32)];
            atomicOr(&w.cp[sp], PN_MATCHED);
            atomicOr(&w.ct[st], PN_MATCHED);
            atomicAdd(&w.tp[c], 1u);
            atomicAdd(&w.iou[c], (unsigned long long)(iou * 16777216.0f));      // iou in (0.5, 1] is a multiple of 2^-24: exact
        }
    }
}

__global__ __launch_bounds__(256) void pq_unmatched_kernel(PqWs w, uint32_t cap, const int32_t *cont, int n_cat) {
    const unsigned long long void_key = (unsigned long long)n_cat << 32;
    const int64_t void_p = pn_find(w.kp, cap, void_key), void_t = pn_find(w.kt, cap, void_key);
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long kt = w.kt[s];
        if (kt != PN_EMPTY && (kt >> 32) != (unsigned long long)n_cat && !(w.ct[s] & PN_MATCHED)) {
            const long long void_target = pq_inter(w, cap, void_p, s);
            if (!(pq_div(void_target, w.ct[s] & PN_COUNT) > 0.5f)) atomicAdd(&w.fn[cont[(int)(kt >> 32)]], 1u);
        }
        const unsigned long long kp = w.kp[s];
        if (kp != PN_EMPTY && (kp >> 32) != (unsigned long long)n_cat && !(w.cp[s] & PN_MATCHED)) {
            const long long pred_void = pq_inter(w, cap, s, void_t);
            if (!(pq_div(pred_void, w.cp[s] & PN_COUNT) > 0.5f)) atomicAdd(&w.fp[cont[(int)(kp >> 32)]], 1u);
        }
    }
}

__global__ void pq_commit_kernel(PqWs w, int n_cat, int allow_unknown, double *iou_sum, int32_t *tp, int32_t *fp, int32_t *fn, int32_t *state_flags) {
    const int f = *w.flags;
    if ((f & PN_FLAG_UNKNOWN_PRED) && !allow_unknown) return;         // the reference raises before touching its state
    for (int c = threadIdx.x; c < n_cat; c += blockDim.x) {
        iou_sum[c] += (double)w.iou[c] * 0x1p-24;
        tp[c] = (int32_t)((uint32_t)tp[c] + w.tp[c]);
        fp[c] = (int32_t)((uint32_t)fp[c] + w.fp[c]);
        fn[c] = (int32_t)((uint32_t)fn[c] + w.fn[c]);
    }
    if (threadIdx.x == 0 && (f & PN_FLAG_INST_RANGE)) *state_flags |= PN_FLAG_INST_RANGE;
}

// ================================================================================================ instance cleanup
struct ClWs {
    long long *bg;                   // [1] background id (the image minimum)
    unsigned long long *keys;        // [cap] ids (+ 2^63 - 1, so that INT64_MIN, never inserted, is PN_EMPTY)
    uint32_t *n, *n2;                // [cap] pixels after the opening / after the outlier rejection
    long long *sy, *sx, *syy, *sxx;  // [cap] moments; cl_centre_kernel overwrites sy / sx / syy with cy / cx / mean d^2 (fp64 bits)
    unsigned long long *sd;          // [cap] distance sum in 2^-20 units; cl_thresh_kernel overwrites it with the threshold (fp64 bits)
    int32_t *slot;                   // [N] per pixel: its id's slot, -1 for background / removed pixels
};

__host__ inline int64_t cl_ws_bytes(int64_t N) {
    const int64_t cap = pn_cap(N);
    return pn_align(16) + pn_align(8 * cap) + pn_align(2 * 4 * cap) + pn_align(5 * 8 * cap) + pn_align(4 * N);
}

__host__ inline ClWs cl_ws(void *base, int64_t N, int64_t *key_bytes, int64_t *zero_bytes) {
    const int64_t cap = pn_cap(N);
    unsigned char *p = reinterpret_cast<unsigned char *>(base);
    ClWs w;
    w.bg = reinterpret_cast<long long *>(p);
    p += pn_align(16);
    w.keys = reinterpret_cast<unsigned long long *>(p);
    *key_bytes = pn_align(8 * cap);
    p += *key_bytes;
    w.n = reinterpret_cast<uint32_t *>(p);
    w.n2 = w.n + cap;
    p += pn_align(2 * 4 * cap);
    w.sy = reinterpret_cast<long long *>(p);
    w.sx = w.sy + cap;
    w.syy = w.sx + cap;
    w.sxx = w.syy + cap;
    w.sd = reinterpret_cast<unsigned long long *>(w.sxx + cap);
    *zero_bytes = pn_align(2 * 4 * cap) + pn_align(5 * 8 * cap);
    p += pn_align(5 * 8 * cap);
    w.slot = reinterpret_cast<int32_t *>(p);
    return w;
}

__device__ __forceinline__ unsigned long long cl_key(long long id) { return (unsigned long long)id + 0x7fffffffffffffffull; }

__global__ void cl_init_kernel(ClWs w) { *w.bg = INT64_MAX; }

__global__ __launch_bounds__(256) void cl_min_kernel(const void *ids, int dtype, int64_t H, int64_t W, int64_t sy, int64_t sx, ClWs w) {
    const int64_t N = H * W;
    long long m = INT64_MAX;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = i / W, x = i - y * W;
        const long long v = pn_ld(ids, dtype, y * sy + x * sx);
        m = v < m ? v : m;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const long long a = __shfl_xor(m, o);
        m = a < m ? a : m;
    }
    if (__lane_id() == 0) atomicMin(w.bg, m);
}

// Tile of CL_TH rows x CL_TW columns, one wave per row.  kornia's flat 3x3 opening of each mask (geodesic borders: erosion counts pixels outside the
// image as inside, dilation as outside) on disjoint masks: pixel p is in the erosion of its own id iff every in-image pixel of its 3x3 neighbourhood
// carries that id; q keeps its id iff some in-image 3x3 neighbour p of q (q included) of the same id is in the erosion.
__global__ __launch_bounds__(256) void cl_open_kernel(const void *ids, int dtype, int64_t H, int64_t W, int64_t sy, int64_t sx, int open, ClWs w,
                                                      uint32_t cap) {
    __shared__ long long s_id[CL_TH + 4][CL_TW + 4];
    __shared__ uint8_t s_er[CL_TH + 2][CL_TW + 2];
    const int64_t x0 = (int64_t)blockIdx.x * CL_TW, y0 = (int64_t)blockIdx.y * CL_TH;
    const long long bg = *w.bg;
    if (open) {
        for (int t = threadIdx.x; t < (CL_TH + 4) * (CL_TW + 4); t += blockDim.x) {
            const int ty = t / (CL_TW + 4), tx = t - ty * (CL_TW + 4);
            const int64_t y = y0 + ty - 2, x = x0 + tx - 2;
            s_id[ty][tx] = (y >= 0 && y < H && x >= 0 && x < W) ? pn_ld(ids, dtype, y * sy + x * sx) : 0;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < (CL_TH + 2) * (CL_TW + 2); t += blockDim.x) {
            const int ty = t / (CL_TW + 2), tx = t - ty * (CL_TW + 2);
            const int64_t y = y0 + ty - 1, x = x0 + tx - 1;
            bool er = false;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const long long v = s_id[ty + 1][tx + 1];
                er = true;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int64_t yy = y + dy, xx = x + dx;
                        if (yy >= 0 && yy < H && xx >= 0 && xx < W && s_id[ty + 1 + dy][tx + 1 + dx] != v) er = false;
                    }
            }
            s_er[ty][tx] = er;
        }
        __syncthreads();
    }
    const int row = threadIdx.x >> 6, lane = __lane_id();
    const int64_t y = y0 + row, x = x0 + lane;
    const bool in = y < H && x < W;
    long long v = 0;
    bool keep = false;
    if (in) {
        v = open ? s_id[row + 2][lane + 2] : pn_ld(ids, dtype, y * sy + x * sx);
        keep = v != bg;
        if (keep && open) {
            bool any = false;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    any |= s_er[row + 1 + dy][lane + 1 + dx] && s_id[row + 2 + dy][lane + 2 + dx] == v;   // s_er is 0 outside the image
            keep = any;
        }
    }
    // wave-aggregated moments of the surviving pixels
    const unsigned long long key = cl_key(v);
    unsigned long long pending = __ballot(keep);
    int32_t mine = -1;
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const unsigned long long lk = __shfl(key, leader);
        const bool match = keep && key == lk;
        const unsigned long long m = __ballot(match);
        const unsigned long long fy = match ? (unsigned long long)y : 0, fx = match ? (unsigned long long)x : 0;
        const unsigned long long s_y = wave_sum(fy), s_x = wave_sum(fx), s_yy = wave_sum(fy * fy), s_xx = wave_sum(fx * fx);
        uint32_t slot = 0;
        if (lane == leader) {
            slot = pn_insert(w.keys, cap, lk);
            atomicAdd(&w.n[slot], (uint32_t)__popcll(m));
            atomicAdd((unsigned long long *)&w.sy[slot], s_y);
            atomicAdd((unsigned long long *)&w.sx[slot], s_x);
            atomicAdd((unsigned long long *)&w.syy[slot], s_yy);
            atomicAdd((unsigned long long *)&w.sxx[slot], s_xx);
        }
        slot = __shfl(slot, leader);
        if (match) mine = (int32_t)slot;
        pending &= ~m;
    }
    if (in) w.slot[y * W + x] = mine;
}

__device__ __forceinline__ double cl_bits_d(long long v) { return __longlong_as_double(v); }
__device__ __forceinline__ long long cl_d_bits(double v) { return __double_as_longlong(v); }

__global__ __launch_bounds__(256) void cl_centre_kernel(ClWs w, uint32_t cap) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (int64_t)gridDim.x * blockDim.x) {
        if (w.keys[s] == PN_EMPTY) continue;
        const double n = (double)w.n[s];
        const double cy = (double)w.sy[s] / n, cx = (double)w.sx[s] / n;
        const double msq = ((double)w.syy[s] / n - cy * cy) + ((double)w.sxx[s] / n - cx * cx);     // mean of d^2 over the mask
        w.sy[s] = cl_d_bits(cy);
        w.sx[s] = cl_d_bits(cx);
        w.syy[s] = cl_d_bits(msq);
    }
}

__device__ __forceinline__ double cl_dist(const ClWs &w, int32_t s, int64_t y, int64_t x) {
    const double dy = (double)y - cl_bits_d(w.sy[s]), dx = (double)x - cl_bits_d(w.sx[s]);
    return sqrt(dy * dy + dx * dx);
}

__global__ __launch_bounds__(256) void cl_dist_kernel(int64_t H, int64_t W, ClWs w) {
    const int64_t N = H * W;
    const int lane = __lane_id();
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < N; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        const int32_t s = i < N ? w.slot[i] : -1;
        const bool on = s >= 0;
        unsigned long long f = 0;
        if (on) {
            const int64_t y = i / W, x = i - y * W;
            f = (unsigned long long)(cl_dist(w, s, y, x) * CL_FIX + 0.5);
        }
        unsigned long long pending = __ballot(on);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int32_t ls = __shfl(s, leader);
            const bool match = on && s == ls;
            const unsigned long long sum = wave_sum(match ? f : 0);
            if (lane == leader) atomicAdd(&w.sd[ls], sum);
            pending &= ~__ballot(match);
        }
    }
}

__global__ __launch_bounds__(256) void cl_thresh_kernel(ClWs w, uint32_t cap, double std_threshold) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (int64_t)gridDim.x * blockDim.x) {
        if (w.keys[s] == PN_EMPTY) continue;
        const double n = (double)w.n[s];
        const double mean = (double)w.sd[s] / CL_FIX / n;
        const double var = cl_bits_d(w.syy[s]) - mean * mean;                  // population variance: mean of d^2 - mean(d)^2
        const double thr = mean + std_threshold * sqrt(var > 0.0 ? var : 0.0);
        w.sd[s] = (unsigned long long)cl_d_bits(thr);
    }
}

__global__ __launch_bounds__(256) void cl_keep_kernel(int64_t H, int64_t W, ClWs w) {
    const int64_t N = H * W;
    const int lane = __lane_id();
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < N; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        int32_t s = i < N ? w.slot[i] : -1;
        if (s >= 0) {
            const int64_t y = i / W, x = i - y * W;
            if (!(cl_dist(w, s, y, x) <= cl_bits_d((long long)w.sd[s]))) {
                s = -1;
                w.slot[i] = -1;
            }
        }
        const bool on = s >= 0;
        unsigned long long pending = __ballot(on);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int32_t ls = __shfl(s, leader);
            const unsigned long long m = __ballot(on && s == ls);
            if (lane == leader) atomicAdd(&w.n2[ls], (uint32_t)__popcll(m));
            pending &= ~m;
        }
    }
}

__global__ __launch_bounds__(256) void cl_out_kernel(const void *ids, int dtype, int64_t H, int64_t W, int64_t sy, int64_t sx, int outlier,
                                                     long long min_area, ClWs w, void *out) {
    const int64_t N = H * W;
    const long long bg = *w.bg;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = w.slot[i];
        long long v = bg;
        if (s >= 0 && (long long)(outlier ? w.n2[s] : w.n[s]) >= min_area) {
            const int64_t y = i / W, x = i - y * W;
            v = pn_ld(ids, dtype, y * sy + x * sx);
        }
        if (dtype == PAG_I64) reinterpret_cast<int64_t *>(out)[i] = v;
        else reinterpret_cast<int32_t *>(out)[i] = (int32_t)v;
    }
}

// ================================================================================================ confusion matrix
struct CmImg {
    const void *ptr;
    int dtype;
    int64_t s[4];
};

template <bool LDS>
__global__ __launch_bounds__(256) void cm_kernel(CmImg P, CmImg T, int64_t n1, int64_t n2, int64_t n3, int64_t N, int C, unsigned long long *confmat) {
    __shared__ uint32_t s_h[LDS ? 64 * 64 : 1];
    if (LDS) {
        for (int i = threadIdx.x; i < C * C; i += blockDim.x) s_h[i] = 0;
        __syncthreads();
    }
    const int lane = __lane_id();
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < N; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        int key = -1;
        if (i < N) {
            int64_t r = i;
            const int64_t i3 = r % n3; r /= n3;
            const int64_t i2 = r % n2; r /= n2;
            const int64_t i1 = r % n1, i0 = r / n1;
            const long long p = pn_ld(P.ptr, P.dtype, i0 * P.s[0] + i1 * P.s[1] + i2 * P.s[2] + i3 * P.s[3]);
            const long long t = pn_ld(T.ptr, T.dtype, i0 * T.s[0] + i1 * T.s[1] + i2 * T.s[2] + i3 * T.s[3]);
            if (p >= 0 && p < C && t >= 0 && t < C) key = (int)(t * C + p);
        }
        const bool on = key >= 0;
        unsigned long long pending = __ballot(on);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int lk = __shfl(key, leader);
            const unsigned long long m = __ballot(on && key == lk);
            if (lane == leader) {
                if (LDS) atomicAdd(&s_h[lk], (uint32_t)__popcll(m));
                else atomicAdd(&confmat[lk], (unsigned long long)__popcll(m));
            }
            pending &= ~m;
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < C * C; i += blockDim.x)
            if (s_h[i]) atomicAdd(&confmat[i], (unsigned long long)s_h[i]);
    }
}

// Workspace initialisation as kernels rather than memset calls: the passes stay plain kernel launches in a captured graph.
__global__ __launch_bounds__(256) void pn_fill_kernel(unsigned long long *p, int64_t n, unsigned long long v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

inline unsigned pn_grid(int64_t n, int64_t per_block, unsigned max_blocks) {
    const int64_t g = (n + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g < max_blocks ? g : max_blocks);
}

}      // namespace

extern "C" int64_t pag_panoptic_pq_workspace_bytes(int B, int64_t H, int64_t W, int n_cat) {
    if (B < 1 || H < 1 || W < 1 || n_cat < 1 || n_cat > PN_MAX_CATS || (int64_t)B * H * W > PN_MAX_PIXELS) return 0;
    return pq_ws_bytes(B, (int64_t)B * H * W, n_cat);
}

extern "C" int pag_panoptic_pq_update(const void *preds, int preds_dtype, const int64_t *preds_strides, const void *target, int target_dtype,
                                      const int64_t *target_strides, int B, int64_t H, int64_t W, const int64_t *cat_ids, const int32_t *cat_cont,
                                      int n_cat, int n_things, int allow_unknown, void *workspace, int64_t workspace_bytes, double *iou_sum,
                                      int32_t *true_positives, int32_t *false_positives, int32_t *false_negatives, int32_t *state_flags,
                                      void *stream) {
    PAG_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= PN_MAX_PIXELS && n_cat >= 2 && n_cat <= PN_MAX_CATS && n_things >= 1 &&
                      n_things < n_cat,
                  "pag_panoptic_pq_update: sizes (B %d, H %lld, W %lld, n_cat %d, n_things %d; B*H*W <= 2^28, n_cat <= %d)", B, (long long)H,
                  (long long)W, n_cat, n_things, PN_MAX_CATS);
    PAG_CHECK_ARG((preds_dtype == PAG_I32 || preds_dtype == PAG_I64) && (target_dtype == PAG_I32 || target_dtype == PAG_I64),
                  "pag_panoptic_pq_update: dtypes %d / %d (int32 or int64)", preds_dtype, target_dtype);
    PAG_CHECK_ARG(preds && target && preds_strides && target_strides && cat_ids && cat_cont && workspace && iou_sum && true_positives &&
                      false_positives && false_negatives && state_flags,
                  "pag_panoptic_pq_update: NULL argument");
    const int64_t N = (int64_t)B * H * W;
    PAG_CHECK_ARG(workspace_bytes >= pq_ws_bytes(B, N, n_cat), "pag_panoptic_pq_update: workspace %lld < %lld bytes", (long long)workspace_bytes,
                  (long long)pq_ws_bytes(B, N, n_cat));
    hipStream_t st = (hipStream_t)stream;
    int64_t head_bytes, key_bytes, count_bytes;
    const PqWs w = pq_ws(workspace, B, N, n_cat, &head_bytes, &key_bytes, &count_bytes);
    const uint32_t cap = (uint32_t)pn_cap(N);
    PqImg P{preds, preds_dtype, {preds_strides[0], preds_strides[1], preds_strides[2], preds_strides[3]}};
    PqImg T{target, target_dtype, {target_strides[0], target_strides[1], target_strides[2], target_strides[3]}};
    hipLaunchKernelGGL(pn_fill_kernel, dim3(pn_grid(head_bytes / 8, 256, 64)), dim3(256), 0, st, (unsigned long long *)workspace, head_bytes / 8, 0ull);
    hipLaunchKernelGGL(pn_fill_kernel, dim3(pn_grid(key_bytes / 8, 256, 2048)), dim3(256), 0, st, w.kp, key_bytes / 8, PN_EMPTY);
    hipLaunchKernelGGL(pn_fill_kernel, dim3(pn_grid(count_bytes / 8, 256, 2048)), dim3(256), 0, st, (unsigned long long *)w.cp, count_bytes / 8, 0ull);
    if (B > 1) {
        hipLaunchKernelGGL(pq_init_kernel, dim3(1), dim3(256), 0, st, w, B);
        hipLaunchKernelGGL(pq_max_kernel, dim3(pn_grid(H * W, 256, 64), B), dim3(256), 0, st, P, T, H, W, w);
    }
    hipLaunchKernelGGL(pq_seg_kernel, dim3(pn_grid(N, 256, 2048)), dim3(256), 0, st, P, T, B, H, W, (const long long *)cat_ids, cat_cont, n_cat,
                       n_things, w, cap);
    hipLaunchKernelGGL(pq_pair_kernel, dim3(pn_grid(N, 256, 2048)), dim3(256), 0, st, N, w, cap);
    hipLaunchKernelGGL(pq_match_kernel, dim3(pn_grid(cap, 256, 2048)), dim3(256), 0, st, w, cap, cat_cont, n_cat);
    hipLaunchKernelGGL(pq_unmatched_kernel, dim3(pn_grid(cap, 256, 2048)), dim3(256), 0, st, w, cap, cat_cont, n_cat);
    hipLaunchKernelGGL(pq_commit_kernel, dim3(1), dim3(256), 0, st, w, n_cat, allow_unknown, iou_sum, true_positives, false_positives,
                       false_negatives, state_flags);
    PAG_CHECK_LAUNCH("pag_panoptic_pq_update");
    return PAG_OK;
}

extern "C" int64_t pag_panoptic_clean_workspace_bytes(int64_t H, int64_t W) {
    if (H < 1 || W < 1 || H > PN_MAX_SIDE || W > PN_MAX_SIDE || H * W > PN_MAX_PIXELS) return 0;
    return cl_ws_bytes(H * W);
}

extern "C" int pag_panoptic_clean(const void *ids, int dtype, int64_t H, int64_t W, int64_t stride_y, int64_t stride_x, int num_openings,
                                  int outlier_rejection, int64_t min_area, double std_threshold, void *workspace, int64_t workspace_bytes, void *out,
                                  void *stream) {
    PAG_CHECK_ARG(H >= 1 && W >= 1 && H <= PN_MAX_SIDE && W <= PN_MAX_SIDE && H * W <= PN_MAX_PIXELS && num_openings >= 0,
                  "pag_panoptic_clean: sizes (H %lld, W %lld, num_openings %d; H, W <= 32768, H*W <= 2^28)", (long long)H, (long long)W, num_openings);
    PAG_CHECK_ARG(dtype == PAG_I32 || dtype == PAG_I64, "pag_panoptic_clean: dtype %d (int32 or int64)", dtype);
    PAG_CHECK_ARG(ids && workspace && out, "pag_panoptic_clean: NULL argument");
    const int64_t N = H * W;
    PAG_CHECK_ARG(workspace_bytes >= cl_ws_bytes(N), "pag_panoptic_clean: workspace %lld < %lld bytes", (long long)workspace_bytes,
                  (long long)cl_ws_bytes(N));
    hipStream_t st = (hipStream_t)stream;
    int64_t key_bytes, zero_bytes;
    const ClWs w = cl_ws(workspace, N, &key_bytes, &zero_bytes);
    const uint32_t cap = (uint32_t)pn_cap(N);
    hipLaunchKernelGGL(pn_fill_kernel, dim3(pn_grid(key_bytes / 8, 256, 2048)), dim3(256), 0, st, w.keys, key_bytes / 8, PN_EMPTY);
    hipLaunchKernelGGL(pn_fill_kernel, dim3(pn_grid(zero_bytes / 8, 256, 2048)), dim3(256), 0, st, (unsigned long long *)w.n, zero_bytes / 8, 0ull);
    hipLaunchKernelGGL(cl_init_kernel, dim3(1), dim3(1), 0, st, w);
    hipLaunchKernelGGL(cl_min_kernel, dim3(pn_grid(N, 256, 512)), dim3(256), 0, st, ids, dtype, H, W, stride_y, stride_x, w);
    hipLaunchKernelGGL(cl_open_kernel, dim3((unsigned)((W + CL_TW - 1) / CL_TW), (unsigned)((H + CL_TH - 1) / CL_TH)), dim3(CL_TW * CL_TH), 0, st, ids,
                       dtype, H, W, stride_y, stride_x, num_openings > 0 ? 1 : 0, w, cap);
    if (outlier_rejection) {
        hipLaunchKernelGGL(cl_centre_kernel, dim3(pn_grid(cap, 256, 2048)), dim3(256), 0, st, w, cap);
        hipLaunchKernelGGL(cl_dist_kernel, dim3(pn_grid(N, 256, 2048)), dim3(256), 0, st, H, W, w);
        hipLaunchKernelGGL(cl_thresh_kernel, dim3(pn_grid(cap, 256, 2048)), dim3(256), 0, st, w, cap, std_threshold);
        hipLaunchKernelGGL(cl_keep_kernel, dim3(pn_grid(N, 256, 2048)), dim3(256), 0, st, H, W, w);
    }
    hipLaunchKernelGGL(cl_out_kernel, dim3(pn_grid(N, 256, 2048)), dim3(256), 0, st, ids, dtype, H, W, stride_y, stride_x, outlier_rejection ? 1 : 0,
                       (long long)min_area, w, out);
    PAG_CHECK_LAUNCH("pag_panoptic_clean");
    return PAG_OK;
}

extern "C" int pag_confusion_matrix(const void *preds, int preds_dtype, const int64_t *preds_strides, const void *target, int target_dtype,
                                    const int64_t *target_strides, const int64_t *shape, int C, int64_t *confmat, void *stream) {
    PAG_CHECK_ARG(C >= 1 && C <= 65536, "pag_confusion_matrix: num_classes %d (1 .. 65536)", C);
    PAG_CHECK_ARG((preds_dtype == PAG_I32 || preds_dtype == PAG_I64) && (target_dtype == PAG_I32 || target_dtype == PAG_I64),
                  "pag_confusion_matrix: dtypes %d / %d (int32 or int64)", preds_dtype, target_dtype);
    PAG_CHECK_ARG(preds_strides && target_strides && shape && confmat, "pag_confusion_matrix: NULL argument");
    PAG_CHECK_ARG(shape[0] >= 0 && shape[1] >= 0 && shape[2] >= 0 && shape[3] >= 0, "pag_confusion_matrix: negative shape");
    const int64_t N = shape[0] * shape[1] * shape[2] * shape[3];
    if (N == 0) return PAG_OK;
    PAG_CHECK_ARG(preds && target, "pag_confusion_matrix: NULL input");
    hipStream_t st = (hipStream_t)stream;
    CmImg P{preds, preds_dtype, {preds_strides[0], preds_strides[1], preds_strides[2], preds_strides[3]}};
    CmImg T{target, target_dtype, {target_strides[0], target_strides[1], target_strides[2], target_strides[3]}};
    if (C <= 64)
        hipLaunchKernelGGL(cm_kernel<true>, dim3(pn_grid(N, 1024, 512)), dim3(256), 0, st, P, T, shape[1], shape[2], shape[3], N, C,
                           (unsigned long long *)confmat);
    else
        hipLaunchKernelGGL(cm_kernel<false>, dim3(pn_grid(N, 256, 2048)), dim3(256), 0, st, P, T, shape[1], shape[2], shape[3], N, C,
                           (unsigned long long *)confmat);
    PAG_CHECK_LAUNCH("pag_confusion_matrix");
    return PAG_OK;
}
