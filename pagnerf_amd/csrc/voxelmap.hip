// Fused panoptic voxel map: the exported map points of all views (map.hip) reduced to one row per occupied voxel, and the per-instance table of it.
// Further down: the connected components of the fused map (a lock-free union-find over the sorted rows), and two fused maps joined by voxel key:
// the overlap table of their ids, the cost of the id association, and the merged map.
//
// As tensor ops the fusion is `unique` over voxel keys, `unique` over (key, id) pairs, several index_add_ calls, a scatter-arg-max with tie handling
// and a boolean gather: about twenty launches and, the output sizes being dynamic, several host synchronisations.  Here:
//   1. voxel_keys_kernel    one thread per point: key = iz | iy << 21 | ix << 42 with i = floorf((p - o) / v) per axis (x slowest: the lattice order of
//                           get_dense_occupied_points), INT64_MAX for a dropped row
//   -  the host layer orders the rows by (key, id) with two stable torch.sort calls (rocPRIM's radix sort; plumbing)
//   2. an ORDERED APPEND over the sorted rows (ordered_append.h: count, scan and write pass) with "row starts a kept run" as the predicate and as
//      the write pass voxel_fuse_kernel, a 16-lane group per kept run / label_table_kernel, the 256-thread workgroup per kept run
// A run's end is found by a galloping upper_bound over the sorted keys (ids inside a voxel run are sorted too: the same search gives the id runs).
// Lane j of a group takes rows j, j + W, ... of the run in that order, the lane partials are combined by an xor-shuffle tree (W = 16) or by the
// shuffle tree of each wave and then the four waves in wave order (W = 256): the order of every sum depends on the sorted sequence and W alone, not
// on the grid, the occupancy or how the points were chunked.  No float atomics; rows at or past the capacity are counted and not written.
// The vote: the id with the most rows in the run, on equal counts the smaller id (signed): a max-reduction over the id-run heads under the total
// order (length descending, id ascending).  Compiled with -ffp-contract=off: the key is two roundings (subtract, divide), the mean one division.
#include "ordered_append.h"

namespace {

constexpr int VOX_GROUP = 16;                       // lanes per voxel run
constexpr int VOX_GROUPS = PAG_WAVE / VOX_GROUP;    // runs a wave serves per pass
constexpr int VOX_MAX_IGNORE = 8;
constexpr int64_t VOX_DROPPED = INT64_MAX;
constexpr int64_t VOX_MAX_ROWS = (int64_t)1 << 31;
constexpr float VOX_AXIS = 2097152.0f;              // 2^21 cells per axis
constexpr int64_t CC_AXIS_MAX = 0x1fffff;

// a voxel's key, x slowest: ix << 42 | iy << 21 | iz, every index in [0, CC_AXIS_MAX]
__device__ __forceinline__ int64_t vox_pack(int64_t x, int64_t y, int64_t z) { return x << 42 | y << 21 | z; }
__device__ __forceinline__ void vox_unpack(int64_t key, int64_t &x, int64_t &y, int64_t &z) {
    x = key >> 42, y = key >> 21 & CC_AXIS_MAX, z = key & CC_AXIS_MAX;
}

struct KeyArgs {
    const float *points;
    int64_t n;
    float origin[3], voxel_size;
    int has_limits;
    float lo[3], hi[3];
    int64_t *keys;
};

__global__ __launch_bounds__(OA_BLOCK) void voxel_keys_kernel(KeyArgs a) {
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    bool ok = true;
    int64_t key = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p = a.points[i * 3 + k];
        const float f = floorf((p - a.origin[k]) / a.voxel_size);
        ok = ok && f >= 0.0f && f < VOX_AXIS;       // false for NaN / inf, which a non-finite coordinate gives
        if (a.has_limits) ok = ok && p > a.lo[k] && p < a.hi[k];
        key = key << 21 | (ok ? (int64_t)f : 0);
    }
    a.keys[i] = ok ? key : VOX_DROPPED;
}

// First index in (lo, n] whose element differs from v = a[lo]; a is ascending from lo on.  Doubling steps, then bisection: about 2 log2(run) reads.
__device__ __forceinline__ int64_t run_end(const int64_t *__restrict__ a, int64_t lo, int64_t n, int64_t v) {
    int64_t known = lo, step = 1;
    while (known + step < n && a[known + step] == v) {
        known += step;
        step <<= 1;
    }
    int64_t hi = known + step < n ? known + step : n;      // a[hi] != v, or hi == n
    int64_t l = known + 1;
    while (l < hi) {
        const int64_t mid = l + ((hi - l) >> 1);
        if (a[mid] == v) l = mid + 1;
        else hi = mid;
    }
    return l;
}

// rows ordered by (key, id); a row is kept when it starts a run of at least min_votes equal keys (the keys are sorted: the run is that long iff the
// row min_votes - 1 further on has the same key)
struct FusePred {
    const int64_t *keys;
    int64_t n;
    int64_t min_votes;
    __device__ __forceinline__ bool operator()(int64_t i) const {
        if (i >= n) return false;
        const int64_t k = keys[i];
        if (k == VOX_DROPPED || (i > 0 && keys[i - 1] == k)) return false;
        const int64_t last = i + min_votes - 1;
        return last < n && keys[last] == k;
    }
};

// voxel rows ordered by label; a row is kept when it starts a run of a label that is not ignored
struct LabelPred {
    const int64_t *labels;
    int64_t n;
    int n_ignore;
    int64_t ignore[VOX_MAX_IGNORE];
    __device__ __forceinline__ bool operator()(int64_t i) const {
        if (i >= n) return false;
        const int64_t v = labels[i];
        if (i > 0 && labels[i - 1] == v) return false;
        bool keep = true;
#pragma unroll
        for (int k = 0; k < VOX_MAX_IGNORE; ++k) keep = keep && !(k < n_ignore && ignore[k] == v);
        return keep;
    }
};

struct FuseArgs {
    const int64_t *ids;
    const float *points, *color;
    float *points_out, *color_out, *agreement;
    int64_t *ids_out;
    int32_t *count_out, *voxels;
    int64_t cap;
};

// the vote's total order: more rows win, on equal rows the smaller id
__device__ __forceinline__ bool vote_better(int64_t la, int64_t ia, int64_t lb, int64_t ib) { return la > lb || (la == lb && ia < ib); }

__global__ __launch_bounds__(OA_BLOCK) void voxel_fuse_kernel(FusePred p, FuseArgs a, const int64_t *__restrict__ block_offset) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    const bool keep = p(i);
    __shared__ int wc[OA_WAVES];
    __shared__ uint8_t kept_lane[OA_WAVES][PAG_WAVE];
    const OaVote vote = oa_vote(keep);
    const int wcount = vote.wcount;
    if (lane == 0) wc[wave] = wcount;
    if (keep) kept_lane[wave][vote.rank] = (uint8_t)lane;
    __syncthreads();
    const int64_t wbase = oa_wave_base(block_offset, wc);
    // the wave's kept runs, four per pass: group g of 16 lanes takes the run that starts at kept row k0 + g, whose destination is wbase + k0 + g
    const int g = lane / VOX_GROUP, l = lane % VOX_GROUP;
    const int64_t row0 = (int64_t)blockIdx.x * OA_BLOCK + wave * PAG_WAVE;
    for (int k0 = 0; k0 < wcount; k0 += VOX_GROUPS) {       // wcount is uniform over the wave
        const int k = k0 + g;
        const bool active = k < wcount && wbase + k < a.cap;
        float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        int64_t best_len = 0, best_id = 0, start = 0, end = 0;
        if (active) {
            start = row0 + kept_lane[wave][k];
            end = run_end(p.keys, start, p.n, p.keys[start]);
            for (int64_t r = start + l; r < end; r += VOX_GROUP) {
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c] += a.points[r * 3 + c];
                if (a.color)
#pragma unroll
                    for (int c = 0; c < 3; ++c) s[3 + c] += a.color[r * 3 + c];
                const int64_t id = a.ids[r];
                if (r == start || a.ids[r - 1] != id) {     // an id run starts here
                    const int64_t len = run_end(a.ids, r, end, id) - r;
                    if (vote_better(len, id, best_len, best_id)) {
                        best_len = len;
                        best_id = id;
                    }
                }
            }
        }
#pragma unroll
        for (int x = VOX_GROUP / 2; x >= 1; x >>= 1) {
#pragma unroll
            for (int c = 0; c < 6; ++c) s[c] += __shfl_xor(s[c], x);
            const long long ol = __shfl_xor((long long)best_len, x), oi = __shfl_xor((long long)best_id, x);
            if (vote_better(ol, oi, best_len, best_id)) {
                best_len = ol;
                best_id = oi;
            }
        }
        if (active && l == 0) {
            const int64_t dst = wbase + k, rows = end - start, key = p.keys[start];
            const float fn = (float)rows;
#pragma unroll
            for (int c = 0; c < 3; ++c) a.points_out[dst * 3 + c] = s[c] / fn;
            if (a.color)
#pragma unroll
                for (int c = 0; c < 3; ++c) a.color_out[dst * 3 + c] = s[3 + c] / fn;
            a.ids_out[dst] = best_id;
            a.count_out[dst] = rows > INT32_MAX ? INT32_MAX : (int32_t)rows;
            a.agreement[dst] = (float)best_len / fn;
            int64_t ix, iy, iz;
            vox_unpack(key, ix, iy, iz);
            a.voxels[dst * 3 + 0] = (int32_t)ix;
            a.voxels[dst * 3 + 1] = (int32_t)iy;
            a.voxels[dst * 3 + 2] = (int32_t)iz;
        }
    }
}

struct TableArgs {
    const float *points, *color;
    const int32_t *count;
    int64_t *ids_out, *voxels_out, *obs_out;
    float *centroid, *bbox_min, *bbox_max, *color_out;
    int64_t cap;
};

__global__ __launch_bounds__(OA_BLOCK) void label_table_kernel(LabelPred p, TableArgs a, const int64_t *__restrict__ block_offset) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t block0 = (int64_t)blockIdx.x * OA_BLOCK;
    const bool keep = p(block0 + threadIdx.x);
    __shared__ int wc[OA_WAVES];
    __shared__ uint8_t kept_row[OA_BLOCK];
    __shared__ float part_f[OA_WAVES][12];
    __shared__ int64_t part_obs[OA_WAVES];
    const OaVote vote = oa_vote(keep);
    if (lane == 0) wc[wave] = vote.wcount;
    __syncthreads();
    // the kept rows of the whole block are listed (a run is served by all four waves), so the wave counts are used as they are, not as a wave base
    int below = 0, total = 0;
#pragma unroll
    for (int q = 0; q < OA_WAVES; ++q) {
        below += q < wave ? wc[q] : 0;
        total += wc[q];
    }
    if (keep) kept_row[below + vote.rank] = (uint8_t)threadIdx.x;
    __syncthreads();
    const int64_t base = block_offset[blockIdx.x];
    // the block's kept runs one after the other, each reduced by the whole workgroup: thread t takes rows t, t + 256, ... of the run
    for (int h = 0; h < total; ++h) {                       // total and base are uniform over the workgroup
        const int64_t dst = base + h;
        if (dst >= a.cap) break;
        const int64_t start = block0 + kept_row[h];
        const int64_t label = p.labels[start];
        const int64_t end = run_end(p.labels, start, p.n, label);
        float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        int64_t obs = 0;
        for (int64_t r = start + threadIdx.x; r < end; r += OA_BLOCK) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = a.points[r * 3 + c];
                s[c] += v;
                lo[c] = fminf(lo[c], v);
                hi[c] = fmaxf(hi[c], v);
            }
            if (a.color)
#pragma unroll
                for (int c = 0; c < 3; ++c) s[3 + c] += a.color[r * 3 + c];
            obs += a.count[r];
        }
#pragma unroll
        for (int x = PAG_WAVE / 2; x >= 1; x >>= 1) {
#pragma unroll
            for (int c = 0; c < 6; ++c) s[c] += __shfl_xor(s[c], x);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lo[c] = fminf(lo[c], __shfl_xor(lo[c], x));
                hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], x));
            }
            obs += __shfl_xor((long long)obs, x);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 6; ++c) part_f[wave][c] = s[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                part_f[wave][6 + c] = lo[c];
                part_f[wave][9 + c] = hi[c];
            }
            part_obs[wave] = obs;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float t[12];
#pragma unroll
            for (int c = 0; c < 12; ++c) t[c] = part_f[0][c];
            int64_t o = part_obs[0];
            for (int w = 1; w < OA_WAVES; ++w) {           // the waves in wave order
#pragma unroll
                for (int c = 0; c < 6; ++c) t[c] += part_f[w][c];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    t[6 + c] = fminf(t[6 + c], part_f[w][6 + c]);
                    t[9 + c] = fmaxf(t[9 + c], part_f[w][9 + c]);
                }
                o += part_obs[w];
            }
            const float fn = (float)(end - start);
            a.ids_out[dst] = label;
            a.voxels_out[dst] = end - start;
            a.obs_out[dst] = o;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a.centroid[dst * 3 + c] = t[c] / fn;
                a.bbox_min[dst * 3 + c] = t[6 + c];
                a.bbox_max[dst * 3 + c] = t[9 + c];
                if (a.color_out) a.color_out[dst * 3 + c] = t[3 + c] / fn;
            }
        }
        __syncthreads();                                    // the partials are reused by the next run
    }
}

// ------------------------------------------------------------------------------------------- connected components of the fused map
// The map's rows ascend by key with z fastest, so the neighbours of a voxel in column (ix + dx, iy + dy) are adjacent rows found by ONE lower-bound
// search, and (0, 0, -1) is the row before.  A row visits the lexicographically negative half of its neighbourhood (all of them earlier rows) and
// unites itself with each neighbour it finds in a lock-free union-find over int32 parent[V]:
//   cc_prepare_kernel   key of every row (-1: an index outside [0, 2^21)), parent[i] = i, the contract bits of `status`
//   cc_link_kernel      the unions: find both roots, hook the LARGER root under the smaller with a compare-and-swap
//   cc_flatten_kernel   root[i], a walk over the finished forest
//   cc_number_kernel    the write pass of the ordered append over "row is its own root and not ignored" (CcRootPred): root rows get 1, 2, ... in
//                       row order
//   cc_label_kernel     every other row takes its root's number, ignored rows 0
// parent[x] <= x always and only a root (parent[x] == x) is ever hooked, under a smaller index: a component's final root is its smallest row, however
// the lanes interleave, so the numbering is that of the definition.  NO THREAD WAITS ON ANOTHER: a failed compare-and-swap means another thread
// hooked that root under a strictly smaller one, and the retry goes on from there; every walk and retry loop is also capped at V + 1 rounds
// (CC_CAP in `status`, never reached on valid input).  In the link kernel parent is read and written by relaxed agent-scope atomics only.
constexpr int CC_ORDER = 1, CC_RANGE = 2, CC_CAP = 4;      // bits of the status word

struct IgnoreSet {
    int n;
    int64_t v[VOX_MAX_IGNORE];
    __device__ __forceinline__ bool has(int64_t id) const {
        bool hit = false;
#pragma unroll
        for (int k = 0; k < VOX_MAX_IGNORE; ++k) hit = hit || (k < n && v[k] == id);
        return hit;
    }
};

struct CcArgs {
    const int32_t *voxels;
    const int64_t *ids;
    int64_t n;
    int max_nonzero, same_id;       // offsets with at most 1 / 2 / 3 non-zero components: 6 / 18 / 26 neighbours
    IgnoreSet ignore;
    int64_t *keys;
    int32_t *parent, *root, *status;
};

__device__ __forceinline__ int64_t cc_key(const int32_t *__restrict__ voxels, int64_t i) {
    const int64_t x = voxels[i * 3], y = voxels[i * 3 + 1], z = voxels[i * 3 + 2];
    const bool ok = x >= 0 && x <= CC_AXIS_MAX && y >= 0 && y <= CC_AXIS_MAX && z >= 0 && z <= CC_AXIS_MAX;
    return ok ? vox_pack(x, y, z) : -1;
}

__global__ __launch_bounds__(OA_BLOCK) void cc_prepare_kernel(CcArgs a) {
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int64_t key = cc_key(a.voxels, i);
    a.keys[i] = key;
    a.parent[i] = (int32_t)i;
    int bad = key < 0 ? CC_RANGE : 0;
    if (key >= 0 && i > 0 && cc_key(a.voxels, i - 1) >= key) bad |= CC_ORDER;
    if (bad) atomicOr(a.status, bad);
}

__device__ __forceinline__ int32_t cc_load(int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// true: *p was `expected` and is now `desired`; false: `expected` holds what was there
__device__ __forceinline__ bool cc_cas(int32_t *p, int32_t &expected, int32_t desired) {
    return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x; every step goes to a strictly smaller index.  On the way x's parent is replaced by its grandparent (only where x is not a
// root, and only by an ancestor: whether that swap succeeds does not matter).
__device__ __forceinline__ int32_t cc_find(int32_t *parent, int32_t x, int64_t cap, int32_t *status) {
    for (int64_t it = 0; it < cap; ++it) {
        const int32_t p = cc_load(parent + x);
        if (p == x) return x;
        const int32_t g = cc_load(parent + p);
        if (g != p) {
            int32_t was = p;
            cc_cas(parent + x, was, g);
        }
        x = g;
    }
    atomicOr(status, CC_CAP);
    return x;
}

__device__ __forceinline__ void cc_union(int32_t *parent, int32_t a, int32_t b, int64_t cap, int32_t *status) {
    int32_t ra = cc_find(parent, a, cap, status), rb = cc_find(parent, b, cap, status);
    for (int64_t it = 0; it < cap; ++it) {
        if (ra == rb) return;
        const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int32_t seen = hi;
        if (cc_cas(parent + hi, seen, lo)) return;
        ra = cc_find(parent, seen, cap, status);        // hi was hooked under seen < hi meanwhile: go on from there
        rb = lo;
    }
    atomicOr(status, CC_CAP);
}

__device__ __forceinline__ void cc_link(const CcArgs &a, int64_t i, int64_t j, int64_t id, int64_t cap) {
    const int64_t other = a.ids[j];
    if (a.same_id ? other != id : a.ignore.has(other)) return;
    cc_union(a.parent, (int32_t)i, (int32_t)j, cap, a.status);
}

__global__ __launch_bounds__(OA_BLOCK) void cc_link_kernel(CcArgs a) {
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int64_t key = a.keys[i];
    if (key < 0 || (i > 0 && a.keys[i - 1] >= key)) return;       // the contract is broken here (status says so): the row links nothing
    const int64_t id = a.ids[i];
    if (a.ignore.has(id)) return;
    const int64_t cap = a.n + 1;
    int64_t ix, iy, iz;
    vox_unpack(key, ix, iy, iz);
    if (i > 0 && iz > 0 && a.keys[i - 1] == key - 1) cc_link(a, i, i - 1, id, cap);       // (0, 0, -1)
#pragma unroll
    for (int q = 0; q < 4; ++q) {                           // (dx, dy) = (-1, -1), (-1, 0), (-1, 1), (0, -1)
        const int dx = q < 3 ? -1 : 0, dy = q < 3 ? q - 1 : -1;
        const int planar = (dx != 0) + (dy != 0);
        if (planar > a.max_nonzero) continue;
        const int64_t nx = ix + dx, ny = iy + dy;
        if (nx < 0 || ny < 0 || ny > CC_AXIS_MAX) continue; // no such column: nothing is borrowed from the next axis
        const bool dz = planar < a.max_nonzero;             // dz = -1, +1 are in the neighbourhood as well
        const int64_t column = vox_pack(nx, ny, 0);
        const int64_t first = column | (dz && iz > 0 ? iz - 1 : iz), last = column | (dz && iz < CC_AXIS_MAX ? iz + 1 : iz);
        int64_t lo = 0, hi = i;                             // the neighbours are earlier rows: lower bound of `first` in keys[0, i)
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.keys[mid] < first) lo = mid + 1;
            else hi = mid;
        }
        for (int t = 0; t < 3; ++t) {
            const int64_t j = lo + t;
            if (j >= i) break;
            const int64_t k = a.keys[j];
            if (k < first || k > last) break;
            cc_link(a, i, j, id, cap);
        }
    }
}

__global__ __launch_bounds__(OA_BLOCK) void cc_flatten_kernel(CcArgs a) {
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int64_t cap = a.n + 1;
    int32_t x = (int32_t)i;
    int64_t it = 0;
    for (; it < cap; ++it) {
        const int32_t p = a.parent[x];
        if (p == x) break;
        x = p;
    }
    if (it == cap) atomicOr(a.status, CC_CAP);
    a.root[i] = x;
}

// rows in map order; a row is kept when it is the root of its component and its id is not ignored
struct CcRootPred {
    const int32_t *root;
    const int64_t *ids, *keys;
    int64_t n;
    IgnoreSet ignore;
    __device__ __forceinline__ bool operator()(int64_t i) const { return i < n && root[i] == (int32_t)i && keys[i] >= 0 && !ignore.has(ids[i]); }
};

// the write pass of the ordered append: root row i, the k-th kept row of the map, gets component k + 1
__global__ __launch_bounds__(OA_BLOCK) void cc_number_kernel(CcRootPred p, const int64_t *__restrict__ block_offset, int64_t *__restrict__ component) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    const bool keep = p(i);
    __shared__ int wc[OA_WAVES];
    const OaVote vote = oa_vote(keep);
    if (lane == 0) wc[wave] = vote.wcount;
    __syncthreads();
    const int64_t base = oa_wave_base(block_offset, wc);
    if (keep) component[i] = base + vote.rank + 1;
}

// Every other row: its root's number (a root row that was kept, written by the launch before and not here), 0 for a root that was not kept.
__global__ __launch_bounds__(OA_BLOCK) void cc_label_kernel(CcRootPred p, int64_t *component) {
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= p.n) return;
    const int32_t r = p.root[i];
    if (r != (int32_t)i) component[i] = component[r];
    else if (!p(i)) component[i] = 0;
}

// ------------------------------------------------------------------------------------------- two fused maps: the join, the overlap table, the merge
// Both maps ascend strictly by key, so "which voxels do they share, and under which pair of ids" is a join of two sorted columns:
//   ov_prepare_kernel   per map: key of every row (cc_key; the contract bits of `status` as above) and the row's SLOT, the position of its id in the
//                       map's sorted distinct ids (a lower-bound search; the list is staged in LDS when it has at most OV_LDS_IDS entries)
//   ov_join_kernel      one thread per row of a: a lower-bound search for its key in b's keys; a hit adds 1 to table[slot_a * Tb + slot_b]
//   ov_cost_kernel      the fp32 IoU of every table entry and the cost 1 - IoU of the active sub-matrix, in the orientation the solver takes
//   voxel_merge_kernel  the write pass of the ordered append (MergePred) over the rows of both maps sorted stably by key (a's rows first): a run
//                       of one row is copied, a run of two (one of each map) is merged, in key order behind the device counter
// The search is the plain per-thread one over all of b.  The range of b that a workgroup's 256 rows need could be found once and staged in LDS, but
// its length is not bounded (a sparse block of a spans any number of rows of b), so the staged form needs this search as its fallback anyway; it also
// puts two dependent searches and a barrier in front of every lane's own.  Neighbouring lanes hold neighbouring keys: the upper levels of their
// searches read the same addresses (one request per wave) and the lower ones neighbouring lines, which stay in L2 (b's keys: 8 bytes a voxel).
// The adds are combined before they leave the wave (HIP guide, Guideline 12): contiguous rows mostly share their pair, and background x background
// may own most of the map, all on one address.  Per round the first remaining lane's pair is broadcast, the lanes holding it are balloted, the
// leader adds the popcount: at most 64 rounds, one when the wave is of one pair.  Integer atomics only: the table does not depend on arrival order.
// NO THREAD WAITS ON ANOTHER.  Every index taken from data (slot, search bound, table offset, sort order) is checked before it is an address.
constexpr int OV_ID = 8, OV_RUN = 16;                      // further bits of the status word: an id missing from its list, a run the merge cannot reduce
constexpr int OV_LDS_IDS = 2048;

template <class P, class I>
__device__ __forceinline__ I ov_lower_bound(P a, I n, int64_t v) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(OA_BLOCK) void ov_prepare_kernel(const int32_t *__restrict__ voxels, const int64_t *__restrict__ ids, int64_t n,
                                                               const int64_t *__restrict__ uniq, int T, int64_t *__restrict__ keys,
                                                               int32_t *__restrict__ slot, int32_t *__restrict__ status) {
    __shared__ int64_t staged[OV_LDS_IDS];
    const bool in_lds = T <= OV_LDS_IDS;                    // uniform over the grid
    if (in_lds) {
        for (int t = threadIdx.x; t < T; t += OA_BLOCK) staged[t] = uniq[t];
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t key = cc_key(voxels, i);
    keys[i] = key;
    int bad = key < 0 ? CC_RANGE : 0;
    if (key >= 0 && i > 0 && cc_key(voxels, i - 1) >= key) bad |= CC_ORDER;
    const int64_t id = ids[i];
    int s = in_lds ? ov_lower_bound((const int64_t *)staged, T, id) : ov_lower_bound(uniq, T, id);
    if (s >= T || (in_lds ? staged[s] : uniq[s]) != id) {
        s = -1;
        bad |= OV_ID;
    }
    slot[i] = s;
    if (bad) atomicOr(status, bad);
}

template <bool COMBINE>
__global__ __launch_bounds__(OA_BLOCK) void ov_join_kernel(const int64_t *__restrict__ keys_a, const int32_t *__restrict__ slot_a, int64_t na,
                                                            const int64_t *__restrict__ keys_b, const int32_t *__restrict__ slot_b, int64_t nb, int Ta,
                                                            int Tb, int32_t *__restrict__ table) {
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    bool has = false;
    int32_t pair = 0;
    if (i < na) {
        const int64_t key = keys_a[i];
        const int64_t lo = ov_lower_bound(keys_b, nb, key);
        const bool hit = key >= 0 && lo < nb && keys_b[lo] == key;
        if (hit) {
            const int sa = slot_a[i], sb = slot_b[lo];
            has = sa >= 0 && sa < Ta && sb >= 0 && sb < Tb;
            pair = has ? sa * Tb + sb : 0;
        }
    }
    if (!COMBINE) {
        if (has) atomicAdd(table + pair, 1);
        return;
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(has);                // uniform over the wave: every lane takes every round
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const int32_t p = __shfl(pair, leader);
        const unsigned long long same = __ballot(has && pair == p);
        if (lane == leader) atomicAdd(table + p, __popcll(same));
        todo &= ~same;
    }
}

// threads [0, Ta * Tb): iou of a table entry; threads [0, R * C): the cost of the active sub-matrix.  rows <= columns for the solver: `transposed`
// says that the solver's rows are b's active ids.  iou = (float) t / (float) (r_i + c_j - t), 0 where that denominator is 0; cost = 1.0f - iou.
__global__ __launch_bounds__(OA_BLOCK) void ov_cost_kernel(const int32_t *__restrict__ table, const int64_t *__restrict__ row_sum,
                                                            const int64_t *__restrict__ col_sum, int Ta, int Tb, const int32_t *__restrict__ act_a,
                                                            const int32_t *__restrict__ act_b, int R, int C, int transposed, float *__restrict__ iou,
                                                            float *__restrict__ cost) {
    const int64_t x = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    auto iou_of = [&](int i, int j) -> float {
        const int64_t t = table[(int64_t)i * Tb + j], den = row_sum[i] + col_sum[j] - t;
        const float num = (float)t, d = (float)den;
        return den != 0 ? num / d : 0.0f;
    };
    if (x < (int64_t)Ta * Tb) iou[x] = iou_of((int)(x / Tb), (int)(x % Tb));
    if (x < (int64_t)R * C) {
        const int r = (int)(x / C), c = (int)(x % C);
        const int i = transposed ? act_a[c] : act_a[r], j = transposed ? act_b[r] : act_b[c];
        const bool ok = i >= 0 && i < Ta && j >= 0 && j < Tb;
        cost[x] = ok ? 1.0f - iou_of(i, j) : 1.0f;
    }
}

// the rows of both maps sorted stably by key; a row is kept when it starts a run
struct MergePred {
    const int64_t *keys;
    int64_t n;
    __device__ __forceinline__ bool operator()(int64_t i) const { return i < n && (i == 0 || keys[i - 1] != keys[i]); }
};

struct MergeArgs {
    const int64_t *order;           // sorted position -> row of the concatenation (a's rows, then b's)
    int64_t na, nb;
    const float *points[2], *color[2], *agreement[2];
    const int64_t *ids_a;
    const int32_t *count[2], *voxels[2], *slot_b;
    const int64_t *mapping;         // b's id by slot
    int Tb;
    float *points_out, *color_out, *agreement_out;
    int64_t *ids_out;
    int32_t *count_out, *voxels_out, *status;
    int64_t cap;
};

__device__ __forceinline__ int64_t merge_id(const MergeArgs &a, int m, int64_t r) {
    if (m == 0) return a.ids_a[r];
    const int s = a.slot_b[r];
    return s >= 0 && s < a.Tb ? a.mapping[s] : 0;
}

__global__ __launch_bounds__(OA_BLOCK) void voxel_merge_kernel(MergePred p, MergeArgs a, const int64_t *__restrict__ block_offset) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    const bool keep = p(i);
    __shared__ int wc[OA_WAVES];
    const OaVote vote = oa_vote(keep);
    if (lane == 0) wc[wave] = vote.wcount;
    __syncthreads();
    const int64_t dst = oa_wave_base(block_offset, wc) + vote.rank;
    if (!keep || dst >= a.cap) return;
    const int64_t key = p.keys[i], total = a.na + a.nb;
    const bool two = i + 1 < p.n && p.keys[i + 1] == key;
    int64_t s0 = a.order[i], s1 = two ? a.order[i + 1] : 0;
    s0 = s0 < 0 ? 0 : (s0 >= total ? total - 1 : s0);
    s1 = s1 < 0 ? 0 : (s1 >= total ? total - 1 : s1);
    bool merge = two && s0 < a.na && s1 >= a.na;            // the sort is stable: a's row comes first
    if ((two && !merge) || (i + 2 < p.n && p.keys[i + 2] == key)) {
        atomicOr(a.status, OV_RUN);
        merge = false;
    }
    const int m0 = s0 >= a.na;
    const int64_t r0 = m0 ? s0 - a.na : s0;
    const bool colored = a.color_out != nullptr;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.voxels_out[dst * 3 + c] = a.voxels[m0][r0 * 3 + c];
    if (!merge) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a.points_out[dst * 3 + c] = a.points[m0][r0 * 3 + c];
            if (colored) a.color_out[dst * 3 + c] = a.color[m0][r0 * 3 + c];
        }
        a.ids_out[dst] = merge_id(a, m0, r0);
        a.count_out[dst] = a.count[m0][r0];
        a.agreement_out[dst] = a.agreement[m0][r0];
        return;
    }
    const int64_t r1 = s1 - a.na;
    const int32_t ca = a.count[0][r0], cb = a.count[1][r1];
    const int64_t sum = (int64_t)ca + cb;
    const int32_t cn = sum > INT32_MAX ? INT32_MAX : (int32_t)sum;
    const float fa = (float)ca, fb = (float)cb, fn = (float)cn;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.points_out[dst * 3 + c] = (a.points[0][r0 * 3 + c] * fa + a.points[1][r1 * 3 + c] * fb) / fn;
        if (colored) a.color_out[dst * 3 + c] = (a.color[0][r0 * 3 + c] * fa + a.color[1][r1 * 3 + c] * fb) / fn;
    }
    const int64_t va = (int64_t)rintf(a.agreement[0][r0] * fa), vb = (int64_t)rintf(a.agreement[1][r1] * fb);
    const int64_t ia = merge_id(a, 0, r0), ib = merge_id(a, 1, r1);
    const bool a_wins = vote_better(va, ia, vb, ib);
    const int64_t votes = ia == ib ? va + vb : (a_wins ? va : vb);
    a.ids_out[dst] = a_wins ? ia : ib;
    a.count_out[dst] = cn;
    a.agreement_out[dst] = (float)votes / fn;
}

}  // namespace

extern "C" int64_t pag_voxel_workspace_bytes(int64_t n) {
    if (n <= 0 || n > VOX_MAX_ROWS) return 0;
    const int64_t nb = oa_blocks(n);
    return oa_align(nb * 8) + oa_align(nb * 4);
}

extern "C" int pag_voxel_keys(const float *points, int64_t n, const float *origin_host, float voxel_size, const float *limits_host, int64_t *keys,
                              void *stream) {
    PAG_CHECK_ARG(n >= 0 && n <= VOX_MAX_ROWS, "pag_voxel_keys: n %lld not in [0, 2^31]", (long long)n);
    PAG_CHECK_ARG(voxel_size > 0.0f && voxel_size <= 3.0e38f, "pag_voxel_keys: voxel_size %g is not a positive finite number", (double)voxel_size);
    PAG_CHECK_ARG(origin_host, "pag_voxel_keys: NULL origin");
    if (n == 0) return PAG_OK;
    PAG_CHECK_ARG(points && keys, "pag_voxel_keys: NULL points / keys");
    KeyArgs a = {};
    a.points = points, a.n = n, a.voxel_size = voxel_size, a.keys = keys, a.has_limits = limits_host != nullptr;
    for (int k = 0; k < 3; ++k) {
        a.origin[k] = origin_host[k];
        if (limits_host) a.lo[k] = limits_host[k], a.hi[k] = limits_host[3 + k];
    }
    hipLaunchKernelGGL(voxel_keys_kernel, dim3((unsigned)oa_blocks(n)), dim3(OA_BLOCK), 0, (hipStream_t)stream, a);
    PAG_CHECK_LAUNCH("pag_voxel_keys");
    return PAG_OK;
}

extern "C" int pag_voxel_fuse(const int64_t *keys, const int64_t *ids, const float *points, const float *color, int64_t n, int64_t min_votes,
                              float *points_out, float *color_out, int64_t *ids_out, int32_t *count_out, float *agreement, int32_t *voxels,
                              int64_t cap, int64_t *count, void *workspace, int64_t workspace_bytes, void *stream) {
    PAG_CHECK_ARG(n >= 0 && n <= VOX_MAX_ROWS && cap >= 0 && min_votes >= 1 && min_votes <= VOX_MAX_ROWS,
                  "pag_voxel_fuse: n %lld not in [0, 2^31], cap %lld < 0 or min_votes %lld not in [1, 2^31]", (long long)n, (long long)cap,
                  (long long)min_votes);
    if (n == 0) return PAG_OK;
    PAG_CHECK_ARG(keys && ids && points, "pag_voxel_fuse: NULL keys / ids / points");
    PAG_CHECK_ARG(count && (cap == 0 || (points_out && ids_out && count_out && agreement && voxels && (color_out || !color))),
                  "pag_voxel_fuse: NULL counter / output");
    FusePred p = {keys, n, min_votes};
    FuseArgs a = {};
    a.ids = ids, a.points = points, a.color = color;
    a.points_out = points_out, a.color_out = color_out, a.agreement = agreement, a.ids_out = ids_out, a.count_out = count_out, a.voxels = voxels;
    a.cap = cap;
    hipStream_t st = (hipStream_t)stream;
    return oa_append("pag_voxel_fuse", "pag_voxel_workspace_bytes(n)", pag_voxel_workspace_bytes(n), p, count, workspace, workspace_bytes, st,
                     [&](dim3 grid, dim3 block, const int64_t *block_offset) { hipLaunchKernelGGL(voxel_fuse_kernel, grid, block, 0, st, p, a, block_offset); });
}

extern "C" int pag_label_table(const int64_t *labels, const float *points, const float *color, const int32_t *voxel_count, int64_t n,
                               const int64_t *ignore_host, int n_ignore, int64_t *ids_out, int64_t *voxels_out, int64_t *observations,
                               float *centroid, float *bbox_min, float *bbox_max, float *color_out, int64_t cap, int64_t *count, void *workspace,
                               int64_t workspace_bytes, void *stream) {
    PAG_CHECK_ARG(n >= 0 && n <= VOX_MAX_ROWS && cap >= 0, "pag_label_table: n %lld not in [0, 2^31] or cap %lld < 0", (long long)n, (long long)cap);
    PAG_CHECK_ARG(n_ignore >= 0 && n_ignore <= VOX_MAX_IGNORE && (n_ignore == 0 || ignore_host), "pag_label_table: %d ignored labels (0..%d), or a NULL list",
                  n_ignore, VOX_MAX_IGNORE);
    if (n == 0) return PAG_OK;
    PAG_CHECK_ARG(labels && points && voxel_count, "pag_label_table: NULL labels / points / voxel_count");
    PAG_CHECK_ARG(count && (cap == 0 || (ids_out && voxels_out && observations && centroid && bbox_min && bbox_max && (color_out || !color))),
                  "pag_label_table: NULL counter / output");
    LabelPred p = {};
    p.labels = labels, p.n = n, p.n_ignore = n_ignore;
    for (int k = 0; k < n_ignore; ++k) p.ignore[k] = ignore_host[k];
    TableArgs a = {};
    a.points = points, a.color = color, a.count = voxel_count;
    a.ids_out = ids_out, a.voxels_out = voxels_out, a.obs_out = observations;
    a.centroid = centroid, a.bbox_min = bbox_min, a.bbox_max = bbox_max, a.color_out = color ? color_out : nullptr, a.cap = cap;
    hipStream_t st = (hipStream_t)stream;
    return oa_append("pag_label_table", "pag_voxel_workspace_bytes(n)", pag_voxel_workspace_bytes(n), p, count, workspace, workspace_bytes, st,
                     [&](dim3 grid, dim3 block, const int64_t *block_offset) { hipLaunchKernelGGL(label_table_kernel, grid, block, 0, st, p, a, block_offset); });
}

extern "C" int64_t pag_voxel_components_workspace_bytes(int64_t n) {
    if (n <= 0 || n >= VOX_MAX_ROWS) return 0;
    return oa_align(n * 8) + 2 * oa_align(n * 4) + pag_voxel_workspace_bytes(n);      // keys, parent, root, the ordered append's block tables
}

extern "C" int pag_voxel_components(const int32_t *voxels, const int64_t *ids, int64_t n, int connectivity, int same_id, const int64_t *ignore_host,
                                    int n_ignore, void *workspace, int64_t workspace_bytes, int64_t *component, int64_t *count, int32_t *status,
                                    void *stream) {
    PAG_CHECK_ARG(n >= 0 && n < VOX_MAX_ROWS, "pag_voxel_components: n %lld not in [0, 2^31)", (long long)n);
    PAG_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26, "pag_voxel_components: connectivity %d is not 6, 18 or 26", connectivity);
    PAG_CHECK_ARG(n_ignore >= 0 && n_ignore <= VOX_MAX_IGNORE && (n_ignore == 0 || ignore_host),
                  "pag_voxel_components: n_ignore %d ignored ids (0..%d), or a NULL list", n_ignore, VOX_MAX_IGNORE);
    if (n == 0) return PAG_OK;
    PAG_CHECK_ARG(voxels && ids, "pag_voxel_components: NULL voxels / ids");
    PAG_CHECK_ARG(component && count && status, "pag_voxel_components: NULL component / count / status");
    PAG_CHECK_ARG(workspace && workspace_bytes >= pag_voxel_components_workspace_bytes(n),
                  "pag_voxel_components: workspace smaller than pag_voxel_components_workspace_bytes(n)");
    const int64_t nb = oa_blocks(n);
    char *ws = (char *)workspace;
    CcArgs a = {};
    a.voxels = voxels, a.ids = ids, a.n = n, a.same_id = same_id != 0, a.status = status;
    a.max_nonzero = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
    a.ignore.n = n_ignore;
    for (int k = 0; k < n_ignore; ++k) a.ignore.v[k] = ignore_host[k];
    a.keys = (int64_t *)ws, ws += oa_align(n * 8);
    a.parent = (int32_t *)ws, ws += oa_align(n * 4);
    a.root = (int32_t *)ws, ws += oa_align(n * 4);       // the ordered append's block tables follow
    CcRootPred p = {a.root, ids, a.keys, n, a.ignore};
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    PAG_CHECK_ARG(e == hipSuccess, "pag_voxel_components: hipMemsetAsync failed: %s", hipGetErrorString(e));
    const dim3 grid((unsigned)nb), block(OA_BLOCK);
    hipLaunchKernelGGL(cc_prepare_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(cc_link_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, st, a);
    return oa_append("pag_voxel_components", "pag_voxel_components_workspace_bytes(n)", pag_voxel_workspace_bytes(n), p, count, ws,
                     workspace_bytes - (ws - (char *)workspace), st, [&](dim3, dim3, const int64_t *block_offset) {
                         hipLaunchKernelGGL(cc_number_kernel, grid, block, 0, st, p, block_offset, component);
                         hipLaunchKernelGGL(cc_label_kernel, grid, block, 0, st, p, component);
                     });
}

extern "C" int pag_voxel_overlap(const int32_t *voxels_a, const int64_t *ids_a, int64_t na, const int64_t *uniq_a, int Ta, const int32_t *voxels_b,
                                 const int64_t *ids_b, int64_t nb, const int64_t *uniq_b, int Tb, int combine, int64_t *keys_a, int32_t *slot_a,
                                 int64_t *keys_b, int32_t *slot_b, int32_t *table, int32_t *status, void *stream) {
    PAG_CHECK_ARG(na >= 0 && nb >= 0 && na + nb < VOX_MAX_ROWS, "pag_voxel_overlap: rows %lld / %lld: negative, or together not below 2^31", (long long)na,
                  (long long)nb);
    PAG_CHECK_ARG(Ta >= 0 && Tb >= 0 && (int64_t)Ta * Tb <= INT32_MAX && Ta <= na && Tb <= nb,
                  "pag_voxel_overlap: Ta %d / Tb %d ids: negative, more than rows, or a table of more than 2^31 - 1 entries", Ta, Tb);
    PAG_CHECK_ARG(status, "pag_voxel_overlap: NULL status");
    PAG_CHECK_ARG(na == 0 || (voxels_a && ids_a && uniq_a && keys_a && slot_a && Ta >= 1), "pag_voxel_overlap: NULL voxels / ids / id list / keys / slot of a, or no id");
    PAG_CHECK_ARG(nb == 0 || (voxels_b && ids_b && uniq_b && keys_b && slot_b && Tb >= 1), "pag_voxel_overlap: NULL voxels / ids / id list / keys / slot of b, or no id");
    PAG_CHECK_ARG(table || na == 0 || nb == 0, "pag_voxel_overlap: NULL table");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    PAG_CHECK_ARG(e == hipSuccess, "pag_voxel_overlap: hipMemsetAsync failed: %s", hipGetErrorString(e));
    const dim3 block(OA_BLOCK);
    if (na > 0) hipLaunchKernelGGL(ov_prepare_kernel, dim3((unsigned)oa_blocks(na)), block, 0, st, voxels_a, ids_a, na, uniq_a, Ta, keys_a, slot_a, status);
    if (nb > 0) hipLaunchKernelGGL(ov_prepare_kernel, dim3((unsigned)oa_blocks(nb)), block, 0, st, voxels_b, ids_b, nb, uniq_b, Tb, keys_b, slot_b, status);
    if (na > 0 && nb > 0) {
        if (combine)
            hipLaunchKernelGGL(ov_join_kernel<true>, dim3((unsigned)oa_blocks(na)), block, 0, st, (const int64_t *)keys_a, (const int32_t *)slot_a, na,
                               (const int64_t *)keys_b, (const int32_t *)slot_b, nb, Ta, Tb, table);
        else
            hipLaunchKernelGGL(ov_join_kernel<false>, dim3((unsigned)oa_blocks(na)), block, 0, st, (const int64_t *)keys_a, (const int32_t *)slot_a, na,
                               (const int64_t *)keys_b, (const int32_t *)slot_b, nb, Ta, Tb, table);
    }
    PAG_CHECK_LAUNCH("pag_voxel_overlap");
    return PAG_OK;
}

extern "C" int pag_overlap_cost(const int32_t *table, const int64_t *row_sum, const int64_t *col_sum, int Ta, int Tb, const int32_t *act_a, int n_a,
                                const int32_t *act_b, int n_b, float *iou, float *cost, void *stream) {
    PAG_CHECK_ARG(Ta >= 0 && Tb >= 0 && (int64_t)Ta * Tb <= INT32_MAX, "pag_overlap_cost: Ta %d / Tb %d: negative, or more than 2^31 - 1 entries", Ta, Tb);
    PAG_CHECK_ARG(n_a >= 0 && n_a <= Ta && n_b >= 0 && n_b <= Tb, "pag_overlap_cost: active ids %d / %d not in [0, Ta] / [0, Tb]", n_a, n_b);
    const int64_t entries = (int64_t)Ta * Tb, active = (int64_t)n_a * n_b;
    if (entries == 0) return PAG_OK;
    PAG_CHECK_ARG(table && row_sum && col_sum && iou, "pag_overlap_cost: NULL table / sums / iou");
    PAG_CHECK_ARG(active == 0 || (act_a && act_b && cost), "pag_overlap_cost: NULL active lists / cost");
    const int transposed = n_a > n_b;
    const int R = active == 0 ? 0 : (transposed ? n_b : n_a), C = active == 0 ? 0 : (transposed ? n_a : n_b);
    hipLaunchKernelGGL(ov_cost_kernel, dim3((unsigned)oa_blocks(entries)), dim3(OA_BLOCK), 0, (hipStream_t)stream, table, row_sum, col_sum, Ta, Tb, act_a,
                       act_b, R, C, transposed, iou, cost);
    PAG_CHECK_LAUNCH("pag_overlap_cost");
    return PAG_OK;
}

extern "C" int pag_voxel_merge(const int64_t *keys, const int64_t *order, int64_t na, int64_t nb, const float *points_a, const float *color_a,
                               const int64_t *ids_a, const int32_t *count_a, const float *agreement_a, const int32_t *voxels_a, const float *points_b,
                               const float *color_b, const int32_t *slot_b, const int64_t *mapping, int Tb, const int32_t *count_b,
                               const float *agreement_b, const int32_t *voxels_b, float *points_out, float *color_out, int64_t *ids_out,
                               int32_t *count_out, float *agreement_out, int32_t *voxels_out, int64_t cap, int64_t *count, int32_t *status,
                               void *workspace, int64_t workspace_bytes, void *stream) {
    PAG_CHECK_ARG(na >= 0 && nb >= 0 && na + nb < VOX_MAX_ROWS && cap >= 0 && Tb >= 0 && Tb <= nb,
                  "pag_voxel_merge: rows %lld / %lld: negative, or together not below 2^31; cap %lld < 0; Tb %d not in [0, rows of b]", (long long)na,
                  (long long)nb, (long long)cap, Tb);
    const int64_t n = na + nb;
    if (n == 0) return PAG_OK;
    PAG_CHECK_ARG(keys && order && count && status, "pag_voxel_merge: NULL keys / order / counter / status");
    PAG_CHECK_ARG(na == 0 || (points_a && ids_a && count_a && agreement_a && voxels_a), "pag_voxel_merge: NULL column of a");
    PAG_CHECK_ARG(nb == 0 || (points_b && slot_b && mapping && Tb >= 1 && count_b && agreement_b && voxels_b), "pag_voxel_merge: NULL column of b, or no id");
    PAG_CHECK_ARG(cap == 0 || (points_out && ids_out && count_out && agreement_out && voxels_out), "pag_voxel_merge: NULL output");
    PAG_CHECK_ARG(!color_out || ((na == 0 || color_a) && (nb == 0 || color_b)), "pag_voxel_merge: color_out without the colour of both maps");
    MergePred p = {keys, n};
    MergeArgs a = {};
    a.order = order, a.na = na, a.nb = nb, a.ids_a = ids_a, a.slot_b = slot_b, a.mapping = mapping, a.Tb = Tb;
    a.points[0] = points_a, a.points[1] = points_b, a.color[0] = color_a, a.color[1] = color_b, a.agreement[0] = agreement_a, a.agreement[1] = agreement_b;
    a.count[0] = count_a, a.count[1] = count_b, a.voxels[0] = voxels_a, a.voxels[1] = voxels_b;
    a.points_out = points_out, a.color_out = color_out, a.agreement_out = agreement_out, a.ids_out = ids_out, a.count_out = count_out;
    a.voxels_out = voxels_out, a.status = status, a.cap = cap;
    hipStream_t st = (hipStream_t)stream;
    return oa_append("pag_voxel_merge", "pag_voxel_workspace_bytes(na + nb)", pag_voxel_workspace_bytes(n), p, count, workspace, workspace_bytes, st,
                     [&](dim3 grid, dim3 block, const int64_t *block_offset) { hipLaunchKernelGGL(voxel_merge_kernel, grid, block, 0, st, p, a, block_offset); });
}
