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
//
//   ap_ids_kernel       mask mAP (trainer.py:794-798): per pixel, the ids of pred_raw and of target into two 8192-slot tables
//   ap_rank_kernel      one workgroup per table: ids compacted and sorted ascending in LDS, rank = position - 1 per slot
//   ap_pair_kernel      per pixel: (detection rank of the pred id, ground-truth rank of the target id) counted in a dense [max_det, 4096] array
//   ap_match_kernel     one wave per IoU threshold: fp64 IoUs of exact integers, COCOeval's greedy matching, one slot word per detection
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

// ================================================================================================ mask mean average precision
// One image of MeanAveragePrecision(iou_type="segm") as the trainer feeds it (trainer.py:674-675, :794-798, :839-843): one class, every score 1, the
// masks given as label images.  The masks of one label image are disjoint, so the per-id areas and the pairwise intersection counts of two label
// images carry everything the [K, H, W] mask stacks do.  The id tables hold AP_CAP slots whatever the image size; more than AP_MAX_IDS distinct
// ids on either side is flagged and the update dropped.
constexpr uint32_t AP_CAP = 8192;             // slots of an id table: twice AP_MAX_IDS, so a legal image never fills it
constexpr int AP_MAX_IDS = 4096;              // distinct ids per label image, the smallest included
constexpr int AP_THRESHOLDS = 10;
constexpr int AP_FLAG_IDS = 1;                // more than AP_MAX_IDS distinct ids, or the id INT64_MIN (its key is PN_EMPTY)
constexpr int AP_FLAG_PRED_ID = 2;            // an id of pred that pred_raw lacks

struct ApWs {
    int32_t *flags;                  // [1] this call's flags
    int32_t *n_raw, *n_tgt;          // [1] distinct ids of pred_raw / target
    uint32_t *cr, *ct;               // [AP_CAP] pixels per id
    int32_t *rr, *rt;                // [AP_CAP] per slot: position of the id in ascending order - 1 (the smallest id: -1)
    uint32_t *area_g;                // [AP_MAX_IDS] ground-truth areas by rank
    uint32_t *inter;                 // [max_det][AP_MAX_IDS] pixels of detection d (rank in pred_raw) with target column c = rank + 1 (0: the smallest
                                     //                       target id, which is no ground truth); a row's sum is the detection's area in pred
    unsigned long long *kr, *kt;     // [AP_CAP] id keys (cl_key) of pred_raw / target
};

__host__ inline int64_t ap_zero_bytes(int max_det) { return pn_align(256 + 4 * 4 * (int64_t)AP_CAP + 4 * (int64_t)AP_MAX_IDS * (1 + (int64_t)max_det)); }
__host__ inline int64_t ap_ws_bytes(int max_det) { return ap_zero_bytes(max_det) + pn_align(2 * 8 * (int64_t)AP_CAP); }

__host__ inline ApWs ap_ws(void *base, int max_det) {
    unsigned char *p = reinterpret_cast<unsigned char *>(base);
    ApWs w;
    w.flags = reinterpret_cast<int32_t *>(p);
    w.n_raw = w.flags + 1;
    w.n_tgt = w.flags + 2;
    w.cr = reinterpret_cast<uint32_t *>(p + 256);
    w.ct = w.cr + AP_CAP;
    w.rr = reinterpret_cast<int32_t *>(w.ct + AP_CAP);
    w.rt = w.rr + AP_CAP;
    w.area_g = reinterpret_cast<uint32_t *>(w.rt + AP_CAP);
    w.inter = w.area_g + AP_MAX_IDS;
    w.kr = reinterpret_cast<unsigned long long *>(p + ap_zero_bytes(max_det));
    w.kt = w.kr + AP_CAP;
    return w;
}

struct ApImg {
    const void *ptr;
    int dtype;
    int64_t sy, sx;
};

struct ApThr {
    double t[AP_THRESHOLDS];
};

// Pixel pass 1: the distinct ids of pred_raw and of target into their tables, with pixel counts.
__global__ __launch_bounds__(256) void ap_ids_kernel(ApImg R, ApImg T, int64_t H, int64_t W, ApWs w) {
    const int64_t N = H * W;
    const int lane = __lane_id();
    bool bad = false;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < N; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        const bool on = i < N;
        long long vr = 0, vt = 0;
        if (on) {
            const int64_t y = i / W, x = i - y * W;
            vr = pn_ld(R.ptr, R.dtype, y * R.sy + x * R.sx);
            vt = pn_ld(T.ptr, T.dtype, y * T.sy + x * T.sx);
            bad |= vr == INT64_MIN || vt == INT64_MIN;
        }
        pn_wave_insert_count(w.kr, w.cr, AP_CAP, cl_key(vr), on);
        pn_wave_insert_count(w.kt, w.ct, AP_CAP, cl_key(vt), on);
    }
    if (bad) atomicOr(w.flags, AP_FLAG_IDS);
}

// Workgroup 0: pred_raw's table, workgroup 1: target's.  The ids are compacted into LDS and sorted ascending (cl_key keeps the order of the signed
// ids); every slot gets rank = position - 1, and the target's areas are laid out by rank.
__global__ __launch_bounds__(256) void ap_rank_kernel(ApWs w) {
    __shared__ unsigned long long s_k[AP_MAX_IDS];
    __shared__ int s_n;
    const bool tgt = blockIdx.x == 1;
    const unsigned long long *keys = tgt ? w.kt : w.kr;
    const uint32_t *counts = tgt ? w.ct : w.cr;
    int32_t *rank = tgt ? w.rt : w.rr;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < AP_CAP; s += blockDim.x) {
        const unsigned long long k = keys[s];
        if (k == PN_EMPTY) continue;
        const int i = atomicAdd(&s_n, 1);
        if (i < AP_MAX_IDS) s_k[i] = k;
    }
    __syncthreads();
    const int n = s_n;
    if (n > AP_MAX_IDS) {                                          // the same for every thread
        if (threadIdx.x == 0) atomicOr(w.flags, AP_FLAG_IDS);
        return;
    }
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + threadIdx.x; i < n2; i += blockDim.x) s_k[i] = PN_EMPTY;      // padding sorts last
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)                              // bitonic sort; n2 <= AP_MAX_IDS bounds every loop
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += blockDim.x) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = s_k[i], b = s_k[l];
                    if ((a > b) == ((i & k) == 0)) {
                        s_k[i] = b;
                        s_k[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (int p = threadIdx.x; p < n; p += blockDim.x) {
        const int64_t s = pn_find(keys, AP_CAP, s_k[p]);
        if (s < 0) continue;
        rank[s] = p - 1;
        if (tgt && p >= 1) w.area_g[p - 1] = counts[s];
    }
    if (threadIdx.x == 0) *(tgt ? w.n_tgt : w.n_raw) = n;
}

// Pixel pass 2: the (detection, ground truth) counts.  The lanes of a wave that share (pred id, target id) elect a leader, which looks both ranks up
// and adds the lane count once.
__global__ __launch_bounds__(256) void ap_pair_kernel(ApImg P, ApImg T, int64_t H, int64_t W, int max_det, ApWs w) {
    if (*w.flags & AP_FLAG_IDS) return;                            // set by an earlier launch: there are no ranks
    const int64_t N = H * W;
    const int lane = __lane_id();
    bool missing = false;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < N; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        const bool on = i < N;
        unsigned long long kp = 0, kt = 0;
        if (on) {
            const int64_t y = i / W, x = i - y * W;
            kp = cl_key(pn_ld(P.ptr, P.dtype, y * P.sy + x * P.sx));
            kt = cl_key(pn_ld(T.ptr, T.dtype, y * T.sy + x * T.sx));
        }
        unsigned long long pending = __ballot(on);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const unsigned long long lp = __shfl(kp, leader), lt = __shfl(kt, leader);
            const unsigned long long m = __ballot(on && kp == lp && kt == lt);
            if (lane == leader) {
                const int64_t sd = pn_find(w.kr, AP_CAP, lp), sg = pn_find(w.kt, AP_CAP, lt);
                if (sd < 0) missing = true;
                else if (sg >= 0) {
                    const int d = w.rr[sd], c = w.rt[sg] + 1;
                    if (d >= 0 && d < max_det && c >= 0 && c < AP_MAX_IDS) atomicAdd(&w.inter[(int64_t)d * AP_MAX_IDS + c], (uint32_t)__popcll(m));
                }
            }
            pending &= ~m;
        }
    }
    if (missing) atomicOr(w.flags, AP_FLAG_PRED_ID);
}

// One workgroup, one wave per IoU threshold.  Detections are visited in ascending id; the lanes of a wave go over the ground truths, lane l owning
// g = l, l + 64, ... with their matched bits in one 64-bit register.  COCOeval's greedy rule: the unmatched ground truth of the largest IoU that is
// >= min(t, 1 - 1e-10), the later one on a tie.
__global__ __launch_bounds__(64 * AP_THRESHOLDS) void ap_match_kernel(ApWs w, int max_det, int empty_if_single, ApThr thr, int32_t *slots,
                                                                      long long *npig, int32_t *state_flags) {
    __shared__ uint32_t s_area[AP_MAX_IDS];
    __shared__ uint32_t s_word[AP_MAX_IDS];
    const int f = *w.flags;
    if (f) {                                                       // slots and npig stay as they are
        if (threadIdx.x == 0) *state_flags |= f;
        return;
    }
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    const int nr = *w.n_raw, G = *w.n_tgt - 1;
    int D = nr - 1 < max_det ? nr - 1 : max_det;
    if (empty_if_single && nr == 1) D = 1;                         // trainer.py:780-781: one all-zero mask
    for (int d = wave; d < D; d += AP_THRESHOLDS) {
        unsigned long long a = 0;
        for (int c = lane; c <= G; c += 64) a += w.inter[(int64_t)d * AP_MAX_IDS + c];
        a = wave_sum(a);
        if (lane == 0) {
            s_area[d] = (uint32_t)a;
            s_word[d] = 1;
        }
    }
    __syncthreads();
    const double floor_t = thr.t[wave] < 1.0 - 1e-10 ? thr.t[wave] : 1.0 - 1e-10;
    unsigned long long matched = 0;
    for (int d = 0; d < D; ++d) {
        const long long a_d = s_area[d];
        double best = floor_t;
        int m = -1;
        if (a_d > 0)
            for (int j = 0, g = lane; g < G; ++j, g += 64) {
                if ((matched >> j) & 1) continue;
                const long long i = w.inter[(int64_t)d * AP_MAX_IDS + g + 1];
                if (i == 0) continue;
                const double iou = (double)i / (double)(a_d + (long long)w.area_g[g] - i);
                if (iou < best) continue;
                best = iou;
                m = g;
            }
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o);
            const int om = __shfl_xor(m, o);
            if (om >= 0 && (m < 0 || ob > best || (ob == best && om > m))) {
                best = ob;
                m = om;
            }
        }
        if (m >= 0) {
            if (lane == (m & 63)) matched |= 1ull << (m >> 6);
            if (lane == 0) atomicOr(&s_word[d], 2u << wave);
        }
    }
    __syncthreads();
    for (int d = threadIdx.x; d < max_det; d += blockDim.x) slots[d] = d < D ? (int32_t)s_word[d] : 0;
    if (threadIdx.x == 0) *npig += G;
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

extern "C" int64_t pag_mask_ap_workspace_bytes(int64_t H, int64_t W, int max_detections) {
    if (H < 1 || W < 1 || H > PN_MAX_PIXELS || W > PN_MAX_PIXELS || H * W > PN_MAX_PIXELS || max_detections < 1 || max_detections > AP_MAX_IDS) return 0;
    return ap_ws_bytes(max_detections);
}

extern "C" int pag_mask_ap_update(const void *pred, int pred_dtype, int64_t pred_stride_y, int64_t pred_stride_x, const void *pred_raw,
                                  int raw_dtype, int64_t raw_stride_y, int64_t raw_stride_x, const void *target, int target_dtype,
                                  int64_t target_stride_y, int64_t target_stride_x, int64_t H, int64_t W, int max_detections,
                                  int empty_detection_if_single_id, const double *thresholds, void *workspace, int64_t workspace_bytes,
                                  int32_t *slots, int64_t *npig, int32_t *state_flags, void *stream) {
    PAG_CHECK_ARG(H >= 1 && W >= 1 && H <= PN_MAX_PIXELS && W <= PN_MAX_PIXELS && H * W <= PN_MAX_PIXELS && max_detections >= 1 &&
                      max_detections <= AP_MAX_IDS,
                  "pag_mask_ap_update: sizes (H %lld, W %lld, max_detections %d; 1 <= H*W <= 2^28, 1 <= max_detections <= %d)", (long long)H,
                  (long long)W, max_detections, AP_MAX_IDS);
    PAG_CHECK_ARG((pred_dtype == PAG_I32 || pred_dtype == PAG_I64) && (raw_dtype == PAG_I32 || raw_dtype == PAG_I64) &&
                      (target_dtype == PAG_I32 || target_dtype == PAG_I64),
                  "pag_mask_ap_update: dtypes %d / %d / %d (int32 or int64)", pred_dtype, raw_dtype, target_dtype);
    PAG_CHECK_ARG(pred && pred_raw && target && thresholds && workspace && slots && npig && state_flags, "pag_mask_ap_update: NULL argument");
    PAG_CHECK_ARG(workspace_bytes >= ap_ws_bytes(max_detections), "pag_mask_ap_update: workspace %lld < %lld bytes", (long long)workspace_bytes,
                  (long long)ap_ws_bytes(max_detections));
    hipStream_t st = (hipStream_t)stream;
    const ApWs w = ap_ws(workspace, max_detections);
    const int64_t N = H * W, zero_words = ap_zero_bytes(max_detections) / 8, key_words = 2 * (int64_t)AP_CAP;
    const ApImg P{pred, pred_dtype, pred_stride_y, pred_stride_x}, R{pred_raw, raw_dtype, raw_stride_y, raw_stride_x},
        T{target, target_dtype, target_stride_y, target_stride_x};
    ApThr thr;
    for (int k = 0; k < AP_THRESHOLDS; ++k) thr.t[k] = thresholds[k];
    hipLaunchKernelGGL(pn_fill_kernel, dim3(pn_grid(zero_words, 256, 2048)), dim3(256), 0, st, (unsigned long long *)workspace, zero_words, 0ull);
    hipLaunchKernelGGL(pn_fill_kernel, dim3(pn_grid(key_words, 256, 2048)), dim3(256), 0, st, w.kr, key_words, PN_EMPTY);
    hipLaunchKernelGGL(ap_ids_kernel, dim3(pn_grid(N, 256, 2048)), dim3(256), 0, st, R, T, H, W, w);
    hipLaunchKernelGGL(ap_rank_kernel, dim3(2), dim3(256), 0, st, w);
    hipLaunchKernelGGL(ap_pair_kernel, dim3(pn_grid(N, 256, 2048)), dim3(256), 0, st, P, T, H, W, max_detections, w);
    hipLaunchKernelGGL(ap_match_kernel, dim3(1), dim3(64 * AP_THRESHOLDS), 0, st, w, max_detections, empty_detection_if_single_id ? 1 : 0, thr, slots,
                       (long long *)npig, state_flags);
    PAG_CHECK_LAUNCH("pag_mask_ap_update");
    return PAG_OK;
}
