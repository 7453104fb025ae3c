// segment_consistency_regularizer (loss/regularizers.py:5-35, called at pc_nerf/trainer.py:525-527 in every step of configs/bup20/best.yaml from epoch 601 on)
// on the rendered instance probabilities, where they already live: four launches forward, one backward, no host synchronisation.
//
// The reference loops over images and segments on the host (unique -> .cpu() -> tensor_split, then one bincount / arg-max / nll_loss per segment); the tensor-op
// restatement in pagnerf_amd/loss.py needs ~60 launches forward and as many backward - in the late-training step that is ~0.5 ms of 5 us kernels on the
// stream and ~0.8 ms of launch overhead on the host between the two halves of the backward.  What is computed (quirks included, see oracle/regularizers.py):
//   per image, EVERY distinct value of `labels` is a segment (:11-18); per segment the histogram of its rays' arg-max column (:22); a segment whose rays all
//   predict column 0 is skipped (:24-25); label = first most frequent column among 1.. (:27), 0 when bins[0] * 0.5 > bins[label] (:29-30); term = mean over the
//   segment's rays of -log p[ray, label] (:32); after an image's segments the RUNNING total is divided by that image's segment count (:33); finally / B (:35).
//
//   segreg_slots_kernel   one workgroup per image: the distinct ids through an LDS hash set, sorted by a bitonic network (the order of torch.unique), every
//                         ray's slot = rank of its id by binary search
//   segreg_argmax_kernel  one wave per ray: first arg-max of p + eps over the columns (torch.argmax: NaN counts as the maximum)
//   segreg_terms_kernel   one workgroup per (image, slot): histogram of the slot's rays in LDS (integer atomics), the label, the mean of -log(p[ray, label] + eps) -
//                         lane-strided sums and a fixed butterfly: bitwise reproducible
//   segreg_finish_kernel  one wave: the running normalisation over the images, the value, and coef[b] = d value / d (sum of image b's terms)
//   segreg_bwd_kernel     one wave per ray: the ray's row of d p - zeros and -g coef[b] / (count (p + eps)) in the label's column
//
// tv_loss (loss/regularizers.py:41-54, called through grid_tv_l1_loss / grid_tv_l2_loss at pc_nerf/trainer.py:556-574) on a channel-last lattice
// [d0, d1, d2, C] in f32 / f16 / bf16: two launches forward, one backward, no floating-point atomics, no host synchronisation.
//   tv_fwd_kernel         one item = one lattice point x one channel vector (16 bytes where C and the pointer allow it, else one element); item i sits at
//                         element i * VEC, so a wave reads whole 1 KB runs.  Per item: the point and its +1 neighbour along every axis of extent > 1, the
//                         |.| or (.)^2 of the differences summed in f32; butterfly over the wave, the four waves in order, one partial per workgroup
//   tv_finish_kernel      one workgroup: the partials in f64, thread-strided then a fixed tree; out = sum / d0 (every axis is divided by shape[0], :43,:47)
//   tv_bwd_kernel         per item the -1 and +1 neighbours along every axis: grad = sum [s phi'(v - v_minus) - s phi'(v_plus - v)], s = upstream / d0,
//                         term by term in the order of the tensor-op form's backward
// Workgroup b takes items [b * 1024, (b + 1) * 1024): workgroups are dealt round-robin over the XCDs, so all eight L2s sweep the lattice together and the
// x-neighbour (one d1 * d2 * C slab away, 2 - 4 MB at 101^3) is met again two slabs of traffic later - from the Infinity Cache; y and z neighbours are a
// row or a vector away and come from L2 / L1.  The point's (x, y, z) comes from a 64-bit split of the workgroup's first item (uniform,
// scalar unit) plus 32-bit per-thread carries.
#include "common.h"

namespace {

constexpr int SEG_SLOTS = 2048;            // distinct ids per image the set has room for (more: the value is NaN, as pagnerf_amd.loss documents)
constexpr int SEG_SET = 4096;              // hash set slots (load factor <= 1/2)
constexpr long long SEG_EMPTY = (long long)0x8000000000000000ull;      // INT64_MIN marks an empty slot; a ray carrying it counts as "too many ids"

struct SegWs {
    int32_t *slot, *arg;       // [B,P]
    int32_t *nseg, *over;      // [B]
    int32_t *chosen, *cnt;     // [B,SEG_SLOTS]
    float *term;               // [B,SEG_SLOTS]
    float *coef;               // [B]
};

__host__ __device__ inline int64_t seg_align(int64_t x) { return (x + 63) / 64 * 64; }
__host__ inline int64_t seg_ws_bytes(int64_t B, int64_t P) {
    return 2 * seg_align(B * P * 4) + 2 * seg_align(B * 4) + 3 * seg_align(B * SEG_SLOTS * 4) + seg_align(B * 4);
}
__host__ inline SegWs seg_ws(void *base, int64_t B, int64_t P) {
    unsigned char *p = reinterpret_cast<unsigned char *>(base);
    SegWs w;
    w.slot = reinterpret_cast<int32_t *>(p);   p += seg_align(B * P * 4);
    w.arg = reinterpret_cast<int32_t *>(p);    p += seg_align(B * P * 4);
    w.nseg = reinterpret_cast<int32_t *>(p);   p += seg_align(B * 4);
    w.over = reinterpret_cast<int32_t *>(p);   p += seg_align(B * 4);
    w.chosen = reinterpret_cast<int32_t *>(p); p += seg_align(B * SEG_SLOTS * 4);
    w.cnt = reinterpret_cast<int32_t *>(p);    p += seg_align(B * SEG_SLOTS * 4);
    w.term = reinterpret_cast<float *>(p);     p += seg_align(B * SEG_SLOTS * 4);
    w.coef = reinterpret_cast<float *>(p);
    return w;
}

__global__ __launch_bounds__(1024) void segreg_slots_kernel(const int64_t *__restrict__ labels, int64_t P, int32_t *__restrict__ slot, int32_t *__restrict__ nseg,
                                                            int32_t *__restrict__ over_out) {
    __shared__ long long set[SEG_SET];
    __shared__ long long ids[SEG_SLOTS];
    __shared__ int32_t over, count;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    labels += b * P;
    slot += b * P;
    for (int e = tid; e < SEG_SET; e += 1024) set[e] = SEG_EMPTY;
    for (int e = tid; e < SEG_SLOTS; e += 1024) ids[e] = 0x7fffffffffffffffll;
    if (tid == 0) over = 0, count = 0;
    __syncthreads();
    for (int64_t p = tid; p < P; p += 1024) {
        const long long id = labels[p];
        if (id == SEG_EMPTY) { over = 1; continue; }
        unsigned h = (unsigned)(((unsigned long long)id * 0x9E3779B97F4A7C15ull) >> 52);      // 12 bits
        bool done = false;
        for (int probe = 0; probe < SEG_SET && !done; ++probe) {
            const long long prev = (long long)atomicCAS(reinterpret_cast<unsigned long long *>(&set[h]), (unsigned long long)SEG_EMPTY, (unsigned long long)id);
            done = prev == SEG_EMPTY || prev == id;
            h = (h + 1) & (SEG_SET - 1);
        }
        if (!done) over = 1;
    }
    __syncthreads();
    for (int e = tid; e < SEG_SET; e += 1024) {
        const long long v = set[e];
        if (v != SEG_EMPTY) {
            const int at = atomicAdd(&count, 1);
            if (at < SEG_SLOTS) ids[at] = v;
        }
    }
    __syncthreads();
    if (count > SEG_SLOTS) {
        if (tid == 0) over = 1;
    }
    // bitonic network over the 2048 entries (1024 comparators per stage); empty entries hold INT64_MAX and sort to the end
    for (int k = 2; k <= SEG_SLOTS; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int i = ((tid / j) * 2 * j) + (tid % j), partner = i + j;
            const long long a = ids[i], c = ids[partner];
            const bool up = (i & k) == 0;
            if ((a > c) == up) { ids[i] = c; ids[partner] = a; }
            __syncthreads();
        }
    const int n = count < SEG_SLOTS ? count : SEG_SLOTS;
    for (int64_t p = tid; p < P; p += 1024) {
        const long long id = labels[p];
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ids[mid] < id) lo = mid + 1; else hi = mid;
        }
        slot[p] = lo < n ? lo : (n > 0 ? n - 1 : 0);           // ids the set could not hold (over): any valid slot, the value is NaN anyway
    }
    if (tid == 0) {
        nseg[b] = n;
        over_out[b] = over;
    }
}

__global__ __launch_bounds__(256) void segreg_argmax_kernel(const float *__restrict__ prob, int64_t P, int64_t image_stride, int64_t row_stride, int n_cols, float eps,
                                                            int32_t *__restrict__ arg_out) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (ray >= P) return;
    const float *row = prob + b * image_stride + ray * row_stride;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    bool any_nan = false;
    for (int c = lane; c < n_cols; c += 64) {
        const float x = __fadd_rn(row[c], eps);
        if (x != x) { if (!any_nan) { any_nan = true; arg = c; } }           // torch.argmax: NaN is the maximum, the first one wins
        else if (!any_nan && (x > best || arg == 0x7fffffff)) { best = x; arg = c; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ob = __shfl_xor(best, d);
        const int oa = __shfl_xor(arg, d);
        const bool on = __shfl_xor((int)any_nan, d) != 0;
        bool take;
        if (any_nan != on) take = on;                       // a NaN beats every number
        else if (any_nan) take = oa < arg;                  // both NaN: the lower column
        else take = ob > best || (ob == best && oa < arg);
        if (take) { best = ob; arg = oa; any_nan = on; }
    }
    if (lane == 0) arg_out[b * P + ray] = arg;
}

__global__ __launch_bounds__(256) void segreg_terms_kernel(const float *__restrict__ prob, int64_t P, int64_t image_stride, int64_t row_stride, int n_cols, float eps,
                                                           const int32_t *__restrict__ slot, const int32_t *__restrict__ arg, const int32_t *__restrict__ nseg,
                                                           int32_t *__restrict__ chosen, int32_t *__restrict__ cnt, float *__restrict__ term) {
    extern __shared__ int32_t bins[];                        // [n_cols]
    __shared__ int32_t w_total[4], w_bc[4], w_ba[4];
    __shared__ float w_acc[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.y;
    const int s = blockIdx.x;
    if (s >= nseg[b]) return;                                // workgroup-uniform
    slot += b * P;
    arg += b * P;
    for (int c = tid; c < n_cols; c += 256) bins[c] = 0;
    __syncthreads();
    for (int64_t p = tid; p < P; p += 256)
        if (slot[p] == s) atomicAdd(&bins[arg[p]], 1);      // :22
    __syncthreads();
    // total, and the first most frequent column among 1 .. (:27)
    int total = 0, bc = -1, ba = 0x7fffffff;
    for (int c = tid; c < n_cols; c += 256) {
        const int v = bins[c];
        total += v;
        if (c >= 1 && v > bc) { bc = v; ba = c; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        total += __shfl_xor(total, d);
        const int oc = __shfl_xor(bc, d), oa = __shfl_xor(ba, d);
        if (oc > bc || (oc == bc && oa < ba)) { bc = oc; ba = oa; }
    }
    if (lane == 0) w_total[wave] = total, w_bc[wave] = bc, w_ba[wave] = ba;
    __syncthreads();
    total = w_total[0] + w_total[1] + w_total[2] + w_total[3];
    bc = w_bc[0], ba = w_ba[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (w_bc[w] > bc || (w_bc[w] == bc && w_ba[w] < ba)) bc = w_bc[w], ba = w_ba[w];
    const int b0 = bins[0];
    int label = -1;
    if (n_cols > 1 && total - b0 > 0) {                      // :24-25: skipped when every ray predicts column 0
        label = ba;
        if (__fmul_rn((float)b0, 0.5f) > (float)bc) label = 0;      // :29-30
    }
    float acc = 0.0f;
    if (label >= 0) {                                        // workgroup-uniform
        const float *col = prob + b * image_stride + label;
        for (int64_t p = tid; p < P; p += 256)
            if (slot[p] == s) acc = __fadd_rn(acc, -logf(__fadd_rn(col[p * row_stride], eps)));      // :32
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, d));
        if (lane == 0) w_acc[wave] = acc;
        __syncthreads();
        acc = __fadd_rn(__fadd_rn(w_acc[0], w_acc[1]), __fadd_rn(w_acc[2], w_acc[3]));
    }
    if (tid == 0) {
        chosen[b * SEG_SLOTS + s] = label;
        cnt[b * SEG_SLOTS + s] = total;
        term[b * SEG_SLOTS + s] = label >= 0 ? __fdiv_rn(acc, (float)total) : 0.0f;
    }
}

__global__ __launch_bounds__(64) void segreg_finish_kernel(int B, const int32_t *__restrict__ nseg, const int32_t *__restrict__ over, const float *__restrict__ term,
                                                           float *__restrict__ coef, float *__restrict__ out) {
    const int lane = threadIdx.x;
    float reg = 0.0f;
    bool bad = false;
    for (int b = 0; b < B; ++b) {
        const int n = nseg[b];
        float acc = 0.0f;
        for (int s = lane; s < n; s += 64) acc = __fadd_rn(acc, term[(int64_t)b * SEG_SLOTS + s]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, d));
        reg = __fdiv_rn(__fadd_rn(reg, acc), (float)n);      // :33 - the running total, earlier images included
        bad = bad || over[b] != 0;
    }
    reg = __fdiv_rn(reg, (float)B);                           // :35
    if (lane == 0) {
        out[0] = bad ? __builtin_nanf("") : reg;
        float c = bad ? 0.0f : __fdiv_rn(1.0f, (float)B);
        for (int b = B - 1; b >= 0; --b) {                    // image b's terms are divided by every LATER image's segment count too
            c = __fdiv_rn(c, (float)nseg[b]);
            coef[b] = c;
        }
    }
}

__global__ __launch_bounds__(256) void segreg_bwd_kernel(const float *__restrict__ prob, int64_t P, int64_t image_stride, int64_t row_stride, int n_cols, float eps,
                                                         const int32_t *__restrict__ slot, const int32_t *__restrict__ chosen, const int32_t *__restrict__ cnt,
                                                         const float *__restrict__ coef, const float *__restrict__ grad, float *__restrict__ d_prob) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (ray >= P) return;
    const int s = slot[b * P + ray];
    const int label = chosen[b * SEG_SLOTS + s];
    float v = 0.0f;
    if (label >= 0) {
        const float p = __fadd_rn(prob[b * image_stride + ray * row_stride + label], eps);
        v = -__fdiv_rn(__fmul_rn(grad[0], coef[b]), __fmul_rn((float)cnt[b * SEG_SLOTS + s], p));
    }
    float *row = d_prob + (b * P + ray) * n_cols;
    for (int c = lane; c < n_cols; c += 64) row[c] = c == label ? v : 0.0f;
}


// ------------------------------------------------------------------------------------------------------------------ lattice total variation
constexpr int TV_THREADS = 256;
constexpr int TV_PER_THREAD = 4;
constexpr int TV_TILE = TV_THREADS * TV_PER_THREAD;          // items per workgroup
constexpr int64_t TV_BIG = 1 << 20;                           // an extent from here on is longer than any carry a tile can produce (<= TV_TILE + 1)

template <typename T, int VEC> struct alignas(sizeof(T) * VEC) TvVec { T v[VEC]; };

__device__ __forceinline__ void tv_st(float *p, float v) { *p = v; }
__device__ __forceinline__ void tv_st(bf16_t *p, float v) { *p = (bf16_t)v; }
__device__ __forceinline__ void tv_st(__half *p, float v) { *p = __float2half_rn(v); }

template <typename T, int VEC> __device__ __forceinline__ void tv_load(const T *p, float (&out)[VEC]) {
    const TvVec<T, VEC> raw = *reinterpret_cast<const TvVec<T, VEC> *>(p);
#pragma unroll
    for (int e = 0; e < VEC; ++e) out[e] = pag_ld(&raw.v[e]);
}

struct TvShape {
    int64_t d0, d1, d2;
    int64_t s0, s1;            // element strides of axis 0 and 1 (axis 2: C)
    int64_t items;             // d0 * d1 * d2 * (C / VEC)
    int C, CV;                 // channels, channel vectors per point
};

// q = a / d, a %= d for 0 <= a < d + TV_TILE + 2: a compare for a long axis, a 32-bit division otherwise (workgroup-uniform choice)
__device__ __forceinline__ int64_t tv_carry(int64_t &a, int64_t d) {
    if (d >= TV_BIG) {
        const int64_t q = a >= d ? 1 : 0;
        a -= q * d;
        return q;
    }
    const uint32_t q = (uint32_t)a / (uint32_t)d;
    a = (int64_t)((uint32_t)a - q * (uint32_t)d);
    return (int64_t)q;
}

// the workgroup's first item, split once
struct TvBase {
    int64_t x0, y0, z0;
    int r0;                    // channel vector of the first item
    int count;                 // valid items of this tile
    int64_t item0;
};

__device__ __forceinline__ TvBase tv_base(const TvShape &sh) {
    TvBase b;
    b.item0 = (int64_t)blockIdx.x * TV_TILE;
    const int64_t left = sh.items - b.item0;
    b.count = left < TV_TILE ? (int)left : TV_TILE;
    const int64_t p0 = b.item0 / sh.CV;
    b.r0 = (int)(b.item0 - p0 * sh.CV);
    b.z0 = p0 % sh.d2;
    const int64_t t = p0 / sh.d2;
    b.y0 = t % sh.d1;
    b.x0 = t / sh.d1;
    return b;
}

// item `local` of the tile -> its point (x, y, z); the item's first element is (item0 + local) * VEC
__device__ __forceinline__ void tv_point(const TvShape &sh, const TvBase &b, int local, int64_t &x, int64_t &y, int64_t &z) {
    const uint32_t dp = (uint32_t)(b.r0 + local) / (uint32_t)sh.CV;      // points past the tile's first: <= TV_TILE
    z = b.z0 + (int64_t)dp;
    y = b.y0 + tv_carry(z, sh.d2);
    x = b.x0 + tv_carry(y, sh.d1);
}

template <int POWER> __device__ __forceinline__ float tv_phi(float t) { return POWER == 1 ? fabsf(t) : __fmul_rn(t, t); }
// torch.abs differentiates to sign(t) with sign(0) = 0; pow(t, 2) to 2 t
template <int POWER> __device__ __forceinline__ float tv_dphi(float t) { return POWER == 1 ? (float)((t > 0.0f) - (t < 0.0f)) : __fmul_rn(2.0f, t); }

template <typename T, int VEC, int POWER>
__global__ __launch_bounds__(TV_THREADS) void tv_fwd_kernel(const T *__restrict__ values, TvShape sh, float *__restrict__ partial) {
    __shared__ float w_acc[TV_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TvBase b = tv_base(sh);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < TV_PER_THREAD; ++k) {
        const int local = tid + k * TV_THREADS;
        if (local >= b.count) break;
        int64_t x, y, z;
        tv_point(sh, b, local, x, y, z);
        const T *at = values + (b.item0 + local) * VEC;
        float v[VEC], n[VEC];
        tv_load<T, VEC>(at, v);
        if (x + 1 < sh.d0) {
            tv_load<T, VEC>(at + sh.s0, n);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc = __fadd_rn(acc, tv_phi<POWER>(__fsub_rn(n[e], v[e])));
        }
        if (y + 1 < sh.d1) {
            tv_load<T, VEC>(at + sh.s1, n);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc = __fadd_rn(acc, tv_phi<POWER>(__fsub_rn(n[e], v[e])));
        }
        if (z + 1 < sh.d2) {
            tv_load<T, VEC>(at + sh.C, n);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc = __fadd_rn(acc, tv_phi<POWER>(__fsub_rn(n[e], v[e])));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, d));
    if (lane == 0) w_acc[wave] = acc;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = __fadd_rn(__fadd_rn(w_acc[0], w_acc[1]), __fadd_rn(w_acc[2], w_acc[3]));
}

__global__ __launch_bounds__(TV_THREADS) void tv_finish_kernel(const float *__restrict__ partial, int64_t n, int64_t d0, float *__restrict__ out) {
    __shared__ double sums[TV_THREADS];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += TV_THREADS) acc += (double)partial[i];
    sums[tid] = acc;
    __syncthreads();
    for (int half = TV_THREADS / 2; half >= 1; half >>= 1) {
        if (tid < half) sums[tid] += sums[tid + half];
        __syncthreads();
    }
    if (tid == 0) out[0] = (float)(sums[0] / (double)d0);
}

template <typename T, int VEC, int POWER>
__global__ __launch_bounds__(TV_THREADS) void tv_bwd_kernel(const T *__restrict__ values, TvShape sh, const float *__restrict__ upstream, T *__restrict__ grad) {
    const int tid = threadIdx.x;
    const TvBase b = tv_base(sh);
    // the tensor-op form's own backward, rounding for rounding: `x / size` with a host scalar is x * (1 / size) on the device, every term is scaled on its
    // own (grad * sign(diff), grad * (2 * diff)), an axis's two faces meet first, and the axes arrive last axis first: (A2 + A1) + A0
    const float scale = __fmul_rn(upstream[0], __fdiv_rn(1.0f, (float)sh.d0));
#pragma unroll
    for (int k = 0; k < TV_PER_THREAD; ++k) {
        const int local = tid + k * TV_THREADS;
        if (local >= b.count) break;
        int64_t x, y, z;
        tv_point(sh, b, local, x, y, z);
        const int64_t off = (b.item0 + local) * VEC;
        const T *at = values + off;
        float v[VEC], n[VEC], acc[VEC];
        tv_load<T, VEC>(at, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = 0.0f;
        const int64_t pos[3] = {x, y, z}, ext[3] = {sh.d0, sh.d1, sh.d2}, stride[3] = {sh.s0, sh.s1, (int64_t)sh.C};
#pragma unroll
        for (int a = 2; a >= 0; --a) {
            float face[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) face[e] = 0.0f;
            if (pos[a] + 1 < ext[a]) {
                tv_load<T, VEC>(at + stride[a], n);
#pragma unroll
                for (int e = 0; e < VEC; ++e) face[e] = -__fmul_rn(scale, tv_dphi<POWER>(__fsub_rn(n[e], v[e])));
            }
            if (pos[a] > 0) {
                tv_load<T, VEC>(at - stride[a], n);
#pragma unroll
                for (int e = 0; e < VEC; ++e) face[e] = __fadd_rn(face[e], __fmul_rn(scale, tv_dphi<POWER>(__fsub_rn(v[e], n[e]))));
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = __fadd_rn(acc[e], face[e]);
        }
        TvVec<T, VEC> res;
#pragma unroll
        for (int e = 0; e < VEC; ++e) tv_st(&res.v[e], acc[e]);
        *reinterpret_cast<TvVec<T, VEC> *>(grad + off) = res;
    }
}

constexpr int64_t TV_MAX_C = 1 << 24;             // r0 + local stays far inside 32 bits
constexpr int64_t TV_MAX_ELEMS = (int64_t)1 << 46;

// 0 when the sizes are refused
__host__ inline int64_t tv_elems(int64_t d0, int64_t d1, int64_t d2, int64_t C) {
    if (d0 < 1 || d1 < 1 || d2 < 1 || C < 1 || C > TV_MAX_C) return 0;
    int64_t n = C;
    for (int64_t d : {d0, d1, d2}) {
        if (d > TV_MAX_ELEMS / n) return 0;
        n *= d;
    }
    return n;
}
__host__ inline int64_t tv_blocks(int64_t items) { return (items + TV_TILE - 1) / TV_TILE; }
// sized for one-element items, the most workgroups any dtype / alignment can take
__host__ inline int64_t tv_ws_bytes(int64_t elems) { return seg_align(tv_blocks(elems) * (int64_t)sizeof(float)); }

__host__ inline int tv_vec(int dtype, int64_t C, const void *a, const void *b) {
    const int vec = dtype == PAG_F32 ? 4 : 8;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b);
    return (C % vec == 0 && bits % 16 == 0) ? vec : 1;
}

__host__ inline TvShape tv_shape(int64_t d0, int64_t d1, int64_t d2, int64_t C, int vec) {
    TvShape sh;
    sh.d0 = d0, sh.d1 = d1, sh.d2 = d2;
    sh.s1 = d2 * C, sh.s0 = d1 * d2 * C;
    sh.C = (int)C, sh.CV = (int)(C / vec);
    sh.items = d0 * d1 * d2 * sh.CV;
    return sh;
}

template <typename T, int VEC> void tv_launch_fwd(const void *values, const TvShape &sh, int power, float *partial, hipStream_t st) {
    const dim3 grid((unsigned)tv_blocks(sh.items));
    if (power == 1) hipLaunchKernelGGL((tv_fwd_kernel<T, VEC, 1>), grid, dim3(TV_THREADS), 0, st, static_cast<const T *>(values), sh, partial);
    else hipLaunchKernelGGL((tv_fwd_kernel<T, VEC, 2>), grid, dim3(TV_THREADS), 0, st, static_cast<const T *>(values), sh, partial);
}

template <typename T, int VEC> void tv_launch_bwd(const void *values, const TvShape &sh, int power, const float *upstream, void *grad, hipStream_t st) {
    const dim3 grid((unsigned)tv_blocks(sh.items));
    if (power == 1) hipLaunchKernelGGL((tv_bwd_kernel<T, VEC, 1>), grid, dim3(TV_THREADS), 0, st, static_cast<const T *>(values), sh, upstream, static_cast<T *>(grad));
    else hipLaunchKernelGGL((tv_bwd_kernel<T, VEC, 2>), grid, dim3(TV_THREADS), 0, st, static_cast<const T *>(values), sh, upstream, static_cast<T *>(grad));
}

}      // namespace

extern "C" int64_t pag_tv_workspace_bytes(int64_t d0, int64_t d1, int64_t d2, int64_t C) {
    const int64_t elems = tv_elems(d0, d1, d2, C);
    return elems ? tv_ws_bytes(elems) : 0;
}

extern "C" int pag_tv_fwd(const void *values, int dtype, int64_t d0, int64_t d1, int64_t d2, int64_t C, int power, void *workspace, int64_t workspace_bytes,
                          float *out, void *stream) {
    const int64_t elems = tv_elems(d0, d1, d2, C);
    PAG_CHECK_ARG(elems > 0, "pag_tv_fwd: sizes (%lld x %lld x %lld x %lld; every extent >= 1, C <= %lld)", (long long)d0, (long long)d1, (long long)d2, (long long)C,
                  (long long)TV_MAX_C);
    PAG_CHECK_ARG(power == 1 || power == 2, "pag_tv_fwd: power %d (1 or 2)", power);
    PAG_CHECK_ARG(dtype == PAG_F32 || dtype == PAG_F16 || dtype == PAG_BF16, "pag_tv_fwd: dtype %d", dtype);
    PAG_CHECK_ARG(values && workspace && out, "pag_tv_fwd: NULL input/output");
    PAG_CHECK_ARG(workspace_bytes >= tv_ws_bytes(elems), "pag_tv_fwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)tv_ws_bytes(elems));
    hipStream_t st = (hipStream_t)stream;
    const int vec = tv_vec(dtype, C, values, nullptr);
    const TvShape sh = tv_shape(d0, d1, d2, C, vec);
    PAG_CHECK_ARG(tv_blocks(sh.items) <= 0x7fffffffll, "pag_tv_fwd: %lld workgroups", (long long)tv_blocks(sh.items));
    float *partial = static_cast<float *>(workspace);
    if (dtype == PAG_F32) { if (vec == 4) tv_launch_fwd<float, 4>(values, sh, power, partial, st); else tv_launch_fwd<float, 1>(values, sh, power, partial, st); }
    else if (dtype == PAG_F16) { if (vec == 8) tv_launch_fwd<__half, 8>(values, sh, power, partial, st); else tv_launch_fwd<__half, 1>(values, sh, power, partial, st); }
    else { if (vec == 8) tv_launch_fwd<bf16_t, 8>(values, sh, power, partial, st); else tv_launch_fwd<bf16_t, 1>(values, sh, power, partial, st); }
    hipLaunchKernelGGL(tv_finish_kernel, dim3(1), dim3(TV_THREADS), 0, st, partial, tv_blocks(sh.items), d0, out);
    PAG_CHECK_LAUNCH("pag_tv_fwd");
    return PAG_OK;
}

extern "C" int pag_tv_bwd(const void *values, int dtype, int64_t d0, int64_t d1, int64_t d2, int64_t C, int power, const float *upstream, void *grad, void *stream) {
    const int64_t elems = tv_elems(d0, d1, d2, C);
    PAG_CHECK_ARG(elems > 0, "pag_tv_bwd: sizes (%lld x %lld x %lld x %lld; every extent >= 1, C <= %lld)", (long long)d0, (long long)d1, (long long)d2, (long long)C,
                  (long long)TV_MAX_C);
    PAG_CHECK_ARG(power == 1 || power == 2, "pag_tv_bwd: power %d (1 or 2)", power);
    PAG_CHECK_ARG(dtype == PAG_F32 || dtype == PAG_F16 || dtype == PAG_BF16, "pag_tv_bwd: dtype %d", dtype);
    PAG_CHECK_ARG(values && upstream && grad, "pag_tv_bwd: NULL input/output");
    hipStream_t st = (hipStream_t)stream;
    const int vec = tv_vec(dtype, C, values, grad);
    const TvShape sh = tv_shape(d0, d1, d2, C, vec);
    PAG_CHECK_ARG(tv_blocks(sh.items) <= 0x7fffffffll, "pag_tv_bwd: %lld workgroups", (long long)tv_blocks(sh.items));
    if (dtype == PAG_F32) { if (vec == 4) tv_launch_bwd<float, 4>(values, sh, power, upstream, grad, st); else tv_launch_bwd<float, 1>(values, sh, power, upstream, grad, st); }
    else if (dtype == PAG_F16) { if (vec == 8) tv_launch_bwd<__half, 8>(values, sh, power, upstream, grad, st); else tv_launch_bwd<__half, 1>(values, sh, power, upstream, grad, st); }
    else { if (vec == 8) tv_launch_bwd<bf16_t, 8>(values, sh, power, upstream, grad, st); else tv_launch_bwd<bf16_t, 1>(values, sh, power, upstream, grad, st); }
    PAG_CHECK_LAUNCH("pag_tv_bwd");
    return PAG_OK;
}

extern "C" int64_t pag_segment_reg_workspace_bytes(int B, int64_t P) { return (B < 0 || P < 0) ? 0 : seg_ws_bytes(B, P); }

extern "C" int pag_segment_reg_fwd(const float *prob, int B, int64_t P, int64_t image_stride, int64_t row_stride, int n_cols, float eps, const int64_t *labels,
                                   void *workspace, int64_t workspace_bytes, float *out, void *stream) {
    PAG_CHECK_ARG(B >= 1 && B <= 65535 && P >= 1 && n_cols >= 1 && n_cols <= 4096 && row_stride >= n_cols, "pag_segment_reg_fwd: sizes (B %d, P %lld, n_cols %d)", B,
                  (long long)P, n_cols);
    PAG_CHECK_ARG(prob && labels && workspace && out, "pag_segment_reg_fwd: NULL input/output");
    PAG_CHECK_ARG(workspace_bytes >= seg_ws_bytes(B, P), "pag_segment_reg_fwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)seg_ws_bytes(B, P));
    hipStream_t st = (hipStream_t)stream;
    const SegWs w = seg_ws(workspace, B, P);
    hipLaunchKernelGGL(segreg_slots_kernel, dim3(B), dim3(1024), 0, st, labels, P, w.slot, w.nseg, w.over);
    hipLaunchKernelGGL(segreg_argmax_kernel, dim3((unsigned)((P + 3) / 4), B), dim3(256), 0, st, prob, P, image_stride, row_stride, n_cols, eps, w.arg);
    const int64_t slots = P < SEG_SLOTS ? P : SEG_SLOTS;
    hipLaunchKernelGGL(segreg_terms_kernel, dim3((unsigned)slots, B), dim3(256), n_cols * sizeof(int32_t), st, prob, P, image_stride, row_stride, n_cols,
                       eps, w.slot, w.arg, w.nseg, w.chosen, w.cnt, w.term);
    hipLaunchKernelGGL(segreg_finish_kernel, dim3(1), dim3(64), 0, st, B, w.nseg, w.over, w.term, w.coef, out);
    PAG_CHECK_LAUNCH("pag_segment_reg_fwd");
    return PAG_OK;
}

extern "C" int pag_segment_reg_bwd(const float *prob, int B, int64_t P, int64_t image_stride, int64_t row_stride, int n_cols, float eps, const void *workspace,
                                   int64_t workspace_bytes, const float *grad, float *d_prob, void *stream) {
    PAG_CHECK_ARG(B >= 1 && B <= 65535 && P >= 1 && n_cols >= 1 && row_stride >= n_cols, "pag_segment_reg_bwd: sizes");
    PAG_CHECK_ARG(prob && workspace && grad && d_prob, "pag_segment_reg_bwd: NULL input/output");
    PAG_CHECK_ARG(workspace_bytes >= seg_ws_bytes(B, P), "pag_segment_reg_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)seg_ws_bytes(B, P));
    const SegWs w = seg_ws(const_cast<void *>(workspace), B, P);
    hipLaunchKernelGGL(segreg_bwd_kernel, dim3((unsigned)((P + 3) / 4), B), dim3(256), 0, (hipStream_t)stream, prob, P, image_stride, row_stride, n_cols, eps, w.slot,
                       w.chosen, w.cnt, w.coef, grad, d_prob);
    PAG_CHECK_LAUNCH("pag_segment_reg_bwd");
    return PAG_OK;
}
