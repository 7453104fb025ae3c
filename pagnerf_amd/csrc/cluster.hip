// Mean-shift clustering of the instance embedding (utils/clustering/mean_shift.py::MeanShift, utils/embedding.py::mean_class_embedding, sklearn's
// estimate_bandwidth / MeanShift(bin_seeding=False, cluster_all=True) / predict) on the device.
//
// The reference copies the class centres to the host and runs sklearn there (seconds per validation at a few thousand centres), and predict_clusters
// copies every validation image's embedding to the host.  Here every pass runs on the device, nothing is read back inside a pass, no float atomics are
// used and every sum runs in a fixed order, so two runs are bitwise identical.  No K x K matrix is stored: distances are recomputed where needed.
//
//   ms_sort_*            (image, label, row) order of the B*P rows: bitonic sort of (label, row index) pairs, LDS stages for spans <= 2048
//   ms_segments_kernel   one workgroup: the heads of the (image, label) runs -> segment starts and K, in image order with ascending labels
//   ms_means_kernel      one workgroup per segment: fp32 sum of its rows (4 waves, rows strided, combined in wave order) / count -> means [K, D]
//                        and a transposed copy [D, Kcap] for coalesced distance loops
//   ms_kth_kernel        8 rows per workgroup: the exact k-th smallest squared distance (fp64 from the fp32 centres, k = max(1, int(K quantile)), the row
//                        itself included) by an 8-pass radix select on the fp64 bit pattern, each pass recomputing the distances
//   ms_bw_kernel         bandwidth = mean of the k-th distances (fixed-order fp64 sum)
//   ms_shift_kernel      4 seeds per workgroup, every centre is a seed: m <- mean of the centres with ||c - m|| <= bw (summed in ascending index order in
//                        fp64, rounded to fp32) until ||m_new - m_old|| <= 1e-3 bw or max_iter; the neighbour sets live in LDS bitmasks
//   ms_dedup_kernel      sklearn keys its result dict by the converged mean: seeds with equal means collapse to one entry (the first seed's slot) holding
//                        the last such seed's intensity; seeds whose last neighbourhood was empty are dropped
//   ms_rank_kernel       position of each entry in the order (intensity, coordinates lexicographically) descending
//   ms_suppress_kernel   one workgroup walks that order: an entry is kept unless an earlier kept one lies within bw -> cluster_centers_
//   ms_predict_kernel    argmin_c ||x - c||: ||c||^2 - 2 x.c on the f32-input MFMA (16 rows per wave), best and second best tracked per row; rows whose
//                        two best scores lie within a rigorous bound of the fp32 rounding error are recomputed exactly in fp64 (ties: lowest index)
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MS_MAX_K = 32768;
constexpr int MS_MAX_D = 512;
constexpr int64_t MS_MAX_ROWS = 1 << 24;
constexpr int MS_TILE = 2048;           // sort elements per workgroup of the LDS stages (1024 threads, one pair each)
constexpr int MS_KROWS = 8;             // bandwidth: query rows per workgroup
constexpr int MS_SEEDS = 4;             // mean shift: seeds per workgroup (one wave each for the per-seed reductions)

__host__ __device__ inline int64_t ms_align(int64_t x) { return (x + 255) / 256 * 256; }
__host__ inline int64_t ms_pow2(int64_t n) {
    int64_t p = MS_TILE;
    while (p < n) p <<= 1;
    return p;
}
__host__ inline int ms_kcap(int64_t n) { return (int)(n < MS_MAX_K ? n : MS_MAX_K); }

struct MsWs {
    long long *skey;                 // [Np] labels in sort order
    int32_t *sidx;                   // [Np] row index g = b P + p in sort order (-1: padding)
    int32_t *seg;                    // [Kcap + 1] first sorted position of each (image, label) run
    float *ct;                       // [D][Kcap] class means, transposed
    double *kdist;                   // [Kcap] k-th nearest distance of each centre
    float *msm;                      // [Kcap][D] converged means
    int32_t *inten, *iters, *rep, *order;    // [Kcap]
};

__host__ inline int64_t ms_ws_bytes(int64_t N, int D) {
    const int64_t np = ms_pow2(N), kc = ms_kcap(N);
    return ms_align(np * 8) + ms_align(np * 4) + ms_align((kc + 1) * 4) + 2 * ms_align(kc * D * 4) + ms_align(kc * 8) + 4 * ms_align(kc * 4);
}

__host__ inline MsWs ms_ws(void *base, int64_t N, int D) {
    const int64_t np = ms_pow2(N), kc = ms_kcap(N);
    unsigned char *p = reinterpret_cast<unsigned char *>(base);
    MsWs w;
    w.skey = reinterpret_cast<long long *>(p);  p += ms_align(np * 8);
    w.sidx = reinterpret_cast<int32_t *>(p);    p += ms_align(np * 4);
    w.seg = reinterpret_cast<int32_t *>(p);     p += ms_align((kc + 1) * 4);
    w.ct = reinterpret_cast<float *>(p);        p += ms_align(kc * D * 4);
    w.msm = reinterpret_cast<float *>(p);       p += ms_align(kc * D * 4);
    w.kdist = reinterpret_cast<double *>(p);    p += ms_align(kc * 8);
    w.inten = reinterpret_cast<int32_t *>(p);   p += ms_align(kc * 4);
    w.iters = reinterpret_cast<int32_t *>(p);   p += ms_align(kc * 4);
    w.rep = reinterpret_cast<int32_t *>(p);     p += ms_align(kc * 4);
    w.order = reinterpret_cast<int32_t *>(p);
    return w;
}

__device__ __forceinline__ float ms_ld(const void *x, int dtype, int64_t e) {
    return dtype == PAG_BF16 ? (float)reinterpret_cast<const bf16_t *>(x)[e] : reinterpret_cast<const float *>(x)[e];
}

// ------------------------------------------------------------------------------------------------ class means

// (image, label, row) order; padding (g < 0) sorts last
__device__ __forceinline__ bool ms_less(long long la, int ga, long long lb, int gb, long long P) {
    if (ga < 0 || gb < 0) return gb < 0 && ga >= 0;
    const long long ba = ga / P, bb = gb / P;
    if (ba != bb) return ba < bb;
    if (la != lb) return la < lb;
    return ga < gb;
}

__global__ __launch_bounds__(256) void ms_sort_init_kernel(const int64_t *__restrict__ labels, int64_t N, int64_t np, MsWs w) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= np) return;
    w.skey[g] = g < N ? labels[g] : 0;
    w.sidx[g] = g < N ? (int32_t)g : -1;
}

// Bitonic stages k in [k_first, k_last] (powers of two), with the partner distances j < MS_TILE, inside one tile of MS_TILE elements in LDS
__global__ __launch_bounds__(1024) void ms_sort_local_kernel(long long P, int64_t k_first, int64_t k_last, MsWs w) {
    __shared__ long long sk[MS_TILE];
    __shared__ int32_t si[MS_TILE];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * MS_TILE;
    for (int e = t; e < MS_TILE; e += 1024) {
        sk[e] = w.skey[base + e];
        si[e] = w.sidx[base + e];
    }
    __syncthreads();
    for (int64_t k = k_first; k <= k_last; k <<= 1) {
        for (int j = (int)(k / 2 < MS_TILE / 2 ? k / 2 : MS_TILE / 2); j > 0; j >>= 1) {
            const int i = 2 * t - (t & (j - 1)), l = i + j;
            const bool asc = ((base + i) & k) == 0;
            const bool swap = asc ? ms_less(sk[l], si[l], sk[i], si[i], P) : ms_less(sk[i], si[i], sk[l], si[l], P);
            if (swap) {
                const long long a = sk[i];
                const int32_t b = si[i];
                sk[i] = sk[l], si[i] = si[l];
                sk[l] = a, si[l] = b;
            }
            __syncthreads();
        }
    }
    for (int e = t; e < MS_TILE; e += 1024) {
        w.skey[base + e] = sk[e];
        w.sidx[base + e] = si[e];
    }
}

// One bitonic step (k, j) with j >= MS_TILE: one thread per pair
__global__ __launch_bounds__(256) void ms_sort_global_kernel(long long P, int64_t k, int64_t j, MsWs w) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = 2 * t - (t & (j - 1)), l = i + j;
    const bool asc = (i & k) == 0;
    const long long ki = w.skey[i], kl = w.skey[l];
    const int32_t gi = w.sidx[i], gl = w.sidx[l];
    const bool swap = asc ? ms_less(kl, gl, ki, gi, P) : ms_less(ki, gi, kl, gl, P);
    if (swap) {
        w.skey[i] = kl, w.sidx[i] = gl;
        w.skey[l] = ki, w.sidx[l] = gi;
    }
}

// info = {K, C, n_iter, flags}; flags bit 0: K > MS_MAX_K (nothing past the count is computed)
__global__ __launch_bounds__(1024) void ms_segments_kernel(int64_t N, long long P, MsWs w, int32_t *__restrict__ info) {
    __shared__ int32_t s_cnt[16];
    __shared__ int64_t s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int64_t p0 = 0; p0 < N; p0 += 1024) {
        const int64_t p = p0 + tid;
        bool h = false;
        if (p < N) h = p == 0 || w.sidx[p] / P != w.sidx[p - 1] / P || w.skey[p] != w.skey[p - 1];
        const unsigned long long bal = __ballot(h);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int64_t off = s_base;
        int total = 0;
        for (int v = 0; v < 16; ++v) {
            off += v < wave ? s_cnt[v] : 0;
            total += s_cnt[v];
        }
        if (h) {
            const int64_t s = off + __popcll(bal & ((1ull << lane) - 1ull));
            if (s < MS_MAX_K) w.seg[s] = (int32_t)p;
        }
        __syncthreads();
        if (tid == 0) s_base += total;
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t K = s_base;
        w.seg[K < MS_MAX_K ? K : MS_MAX_K] = (int32_t)N;
        info[0] = (int32_t)(K < MS_MAX_K ? K : MS_MAX_K + 1);
        info[1] = 0;
        info[2] = 0;
        info[3] = K > MS_MAX_K ? 1 : 0;
    }
}

// Without labels every row is its own class
__global__ void ms_rows_info_kernel(int32_t K, int32_t *__restrict__ info) {
    info[0] = K;
    info[1] = 0;
    info[2] = 0;
    info[3] = 0;
}

__global__ __launch_bounds__(256) void ms_means_kernel(const void *__restrict__ x, int dtype, long long P, int D, int64_t image_stride, int64_t row_stride,
                                                       bool by_label, int Kcap, MsWs w, const int32_t *__restrict__ info, float *__restrict__ means) {
    __shared__ float part[4][MS_MAX_D];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x;
    if (info[3] || s >= info[0]) return;
    const int64_t r0 = by_label ? w.seg[s] : s, r1 = by_label ? w.seg[s + 1] : s + 1;
    float acc[MS_MAX_D / 64];
#pragma unroll
    for (int u = 0; u < MS_MAX_D / 64; ++u) acc[u] = 0.0f;
    for (int64_t r = r0 + wave; r < r1; r += 4) {
        const int64_t g = by_label ? w.sidx[r] : r;
        const int64_t b = g / P, p = g - b * P;
        const int64_t row = b * image_stride + p * row_stride;
#pragma unroll
        for (int u = 0; u < MS_MAX_D / 64; ++u) {
            const int k = lane + 64 * u;
            if (k < D) acc[u] += ms_ld(x, dtype, row + k);
        }
    }
#pragma unroll
    for (int u = 0; u < MS_MAX_D / 64; ++u) {
        const int k = lane + 64 * u;
        if (k < D) part[wave][k] = acc[u];
    }
    __syncthreads();
    const float cnt = (float)(r1 - r0);
    for (int k = tid; k < D; k += 256) {
        const float m = (((part[0][k] + part[1][k]) + part[2][k]) + part[3][k]) / cnt;
        means[(int64_t)s * D + k] = m;
        w.ct[(int64_t)k * Kcap + s] = m;
    }
}

// ------------------------------------------------------------------------------------------------ bandwidth

__global__ __launch_bounds__(256) void ms_kth_kernel(const float *__restrict__ means, int Kcap, int D, double quantile, MsWs w,
                                                     const int32_t *__restrict__ info) {
    __shared__ double q[MS_KROWS][MS_MAX_D];
    __shared__ int32_t hist[MS_KROWS][256];
    __shared__ unsigned long long pre[MS_KROWS];
    __shared__ int32_t need[MS_KROWS];
    const int tid = threadIdx.x;
    const int K = info[0];
    const int i0 = blockIdx.x * MS_KROWS;
    if (info[3] || i0 >= K) return;
    const int nr = K - i0 < MS_KROWS ? K - i0 : MS_KROWS;
    int kth = (int)((double)K * quantile);
    kth = kth < 1 ? 1 : kth;
    for (int e = tid; e < MS_KROWS * D; e += 256) {
        const int r = e / D, k = e - r * D;
        q[r][k] = r < nr ? (double)means[(int64_t)(i0 + r) * D + k] : 0.0;
    }
    if (tid < MS_KROWS) {
        pre[tid] = 0ull;
        need[tid] = kth;
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int e = tid; e < MS_KROWS * 256; e += 256) hist[e >> 8][e & 255] = 0;
        __syncthreads();
        const unsigned long long hm = shift == 56 ? 0ull : (~0ull << (shift + 8));
        for (int j = tid; j < K; j += 256) {
            double acc[MS_KROWS];
#pragma unroll
            for (int r = 0; r < MS_KROWS; ++r) acc[r] = 0.0;
            for (int k = 0; k < D; ++k) {
                const double c = (double)w.ct[(int64_t)k * Kcap + j];
#pragma unroll
                for (int r = 0; r < MS_KROWS; ++r) {
                    const double d = c - q[r][k];
                    acc[r] = fma(d, d, acc[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < MS_KROWS; ++r) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(acc[r]);
                if (r < nr && (bits & hm) == pre[r]) atomicAdd(&hist[r][(bits >> shift) & 255], 1);
            }
        }
        __syncthreads();
        if (tid < nr) {
            int c = 0, sel = 255;
            for (int b = 0; b < 256; ++b) {
                if (c + hist[tid][b] >= need[tid]) {
                    sel = b;
                    break;
                }
                c += hist[tid][b];
            }
            need[tid] -= c;
            pre[tid] |= (unsigned long long)sel << shift;
        }
        __syncthreads();
    }
    if (tid < nr) w.kdist[i0 + tid] = sqrt(__longlong_as_double((long long)pre[tid]));
}

__device__ __forceinline__ double ms_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(256) void ms_bw_kernel(MsWs w, const int32_t *__restrict__ info, double *__restrict__ bandwidth) {
    __shared__ double part[4];
    const int tid = threadIdx.x;
    const int K = info[0];
    if (info[3]) return;
    double s = 0.0;
    for (int i = tid; i < K; i += 256) s += w.kdist[i];
    s = ms_wave_sum(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) bandwidth[0] = (((part[0] + part[1]) + part[2]) + part[3]) / (double)K;
}

// ------------------------------------------------------------------------------------------------ mean shift

__global__ __launch_bounds__(256) void ms_shift_kernel(const float *__restrict__ means, int Kcap, int D, int max_iter, MsWs w,
                                                       const int32_t *__restrict__ info, const double *__restrict__ bandwidth) {
    __shared__ double m[MS_SEEDS][MS_MAX_D];
    __shared__ unsigned long long nb[MS_SEEDS][MS_MAX_K / 64];
    __shared__ double dpart[MS_SEEDS][4];
    __shared__ int32_t cnt[MS_SEEDS], active[MS_SEEDS], inten[MS_SEEDS], iters[MS_SEEDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = info[0];
    const int s0 = blockIdx.x * MS_SEEDS;
    if (info[3] || s0 >= K) return;
    const int ns = K - s0 < MS_SEEDS ? K - s0 : MS_SEEDS;
    const double bw = bandwidth[0], bw2 = bw * bw, thresh = 1e-3 * bw;
    const int nw = (K + 63) / 64;
    for (int e = tid; e < MS_SEEDS * D; e += 256) {
        const int r = e / D, k = e - r * D;
        m[r][k] = r < ns ? (double)means[(int64_t)(s0 + r) * D + k] : 0.0;
    }
    if (tid < MS_SEEDS) {
        active[tid] = tid < ns;
        cnt[tid] = 0;
        inten[tid] = 0;
        iters[tid] = 0;
    }
    int completed = 0;                        // sklearn's completed_iterations of every seed still active (all start together)
    for (;;) {
        __syncthreads();
        if (!(active[0] | active[1] | active[2] | active[3])) break;
        // neighbour sets: bit j of nb[r] <=> ||c_j - m_r|| <= bw
        for (int j0 = 0; j0 < K; j0 += 256) {
            const int j = j0 + tid;
            double acc[MS_SEEDS];
#pragma unroll
            for (int r = 0; r < MS_SEEDS; ++r) acc[r] = 0.0;
            if (j < K) {
                for (int k = 0; k < D; ++k) {
                    const double c = (double)w.ct[(int64_t)k * Kcap + j];
#pragma unroll
                    for (int r = 0; r < MS_SEEDS; ++r) {
                        const double d = c - m[r][k];
                        acc[r] = fma(d, d, acc[r]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < MS_SEEDS; ++r) {
                const unsigned long long bal = __ballot(j < K && acc[r] <= bw2);
                if (lane == 0 && (j0 >> 6) + wave < nw) nb[r][(j0 >> 6) + wave] = bal;
            }
        }
        __syncthreads();
        {       // wave r counts seed r's neighbours
            int c = 0;
            for (int v = lane; v < nw; v += 64) c += __popcll(nb[wave][v]);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
            if (lane == 0) cnt[wave] = c;
        }
        __syncthreads();
        // new means: thread tid owns columns tid, tid + 256; the neighbours in ascending index order, fp64, then rounded to fp32
        double dd[MS_SEEDS];
#pragma unroll
        for (int r = 0; r < MS_SEEDS; ++r) {
            dd[r] = 0.0;
            if (!active[r] || cnt[r] == 0) continue;
            for (int k = tid; k < D; k += 256) {
                double acc = 0.0;
                for (int v = 0; v < nw; ++v) {
                    unsigned long long bits = nb[r][v];
                    while (bits) {
                        int js[8];
                        int n = 0;
                        while (bits && n < 8) {
                            js[n++] = 64 * v + __ffsll((long long)bits) - 1;
                            bits &= bits - 1ull;
                        }
                        float vals[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) vals[e] = e < n ? means[(int64_t)js[e] * D + k] : 0.0f;
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (e < n) acc += (double)vals[e];
                    }
                }
                const double nm = (double)(float)(acc / (double)cnt[r]);
                const double diff = nm - m[r][k];
                dd[r] = fma(diff, diff, dd[r]);
                m[r][k] = nm;                     // column k is read and written by this thread only in this phase
            }
        }
#pragma unroll
        for (int r = 0; r < MS_SEEDS; ++r) {
            const double v = ms_wave_sum(dd[r]);
            if (lane == 0) dpart[r][wave] = v;
        }
        __syncthreads();
        if (tid < MS_SEEDS && active[tid]) {
            const int r = tid;
            if (cnt[r] == 0) {
                active[r] = 0;                    // nothing within bw of the mean: sklearn drops the seed (intensity 0)
            } else {
                const double nrm = sqrt(((dpart[r][0] + dpart[r][1]) + dpart[r][2]) + dpart[r][3]);
                if (nrm <= thresh || completed == max_iter) active[r] = 0;
            }
            if (!active[r]) {
                inten[r] = cnt[r];                // the neighbour count of the last iteration
                iters[r] = completed;
            }
        }
        ++completed;
    }
    for (int e = tid; e < ns * D; e += 256) {
        const int r = e / D, k = e - r * D;
        w.msm[(int64_t)(s0 + r) * D + k] = (float)m[r][k];
    }
    if (tid < ns) {
        w.inten[s0 + tid] = inten[tid];
        w.iters[s0 + tid] = iters[tid];
    }
}

// One wave per seed i, lanes over the other seeds j
__global__ __launch_bounds__(256) void ms_dedup_kernel(int Kcap, int D, MsWs w, const int32_t *__restrict__ info) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= Kcap) return;
    const int K = info[0];
    if (info[3] || i >= K || w.inten[i] == 0) {
        if (lane == 0) w.rep[i] = 0;
        return;
    }
    const float *mi = w.msm + (int64_t)i * D;
    const float f0 = mi[0];
    bool earlier = false;
    int last = -1;                                 // the highest seed j > i with the same mean
    for (int j0 = 0; j0 < K; j0 += 64) {
        const int j = j0 + lane;
        bool eq = false;
        if (j < K && j != i && w.inten[j] != 0) {
            const float *mj = w.msm + (int64_t)j * D;
            eq = mj[0] == f0;
            for (int k = 1; k < D && eq; ++k) eq = mj[k] == mi[k];
        }
        earlier |= eq && j < i;
        if (eq && j > i) last = j;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(last, d);
        last = o > last ? o : last;
    }
    const bool any_earlier = __ballot(earlier) != 0ull;
    if (lane == 0) w.rep[i] = any_earlier ? 0 : w.inten[last >= 0 ? last : i];
}

__global__ __launch_bounds__(256) void ms_rank_kernel(int D, MsWs w, const int32_t *__restrict__ info) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int K = info[0];
    if (info[3] || i >= K) return;
    const int ri = w.rep[i];
    if (ri == 0) return;
    const float *mi = w.msm + (int64_t)i * D;
    int rank = 0;
    for (int j = lane; j < K; j += 64) {
        const int rj = w.rep[j];
        if (rj == 0 || j == i) continue;
        bool greater = rj > ri;
        if (rj == ri) {
            const float *mj = w.msm + (int64_t)j * D;
            int k = 0;
            while (k < D - 1 && mj[k] == mi[k]) ++k;
            greater = mj[k] > mi[k];
        }
        rank += greater;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) rank += __shfl_xor(rank, d);
    if (lane == 0) w.order[rank] = i;
}

__global__ __launch_bounds__(1024) void ms_suppress_kernel(int D, MsWs w, const double *__restrict__ bandwidth, int32_t *__restrict__ info,
                                                           float *__restrict__ centers) {
    extern __shared__ uint16_t kept[];            // K <= 32768: the kept entries' seed indices fit 16 bits (64 KB of LDS at most)
    __shared__ int32_t s_m[16], s_it[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = info[0];
    if (info[3]) return;
    int mcount = 0, it = 0;
    for (int i = tid; i < K; i += 1024) {
        mcount += w.rep[i] > 0;
        it = w.iters[i] > it ? w.iters[i] : it;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mcount += __shfl_xor(mcount, d);
        const int o = __shfl_xor(it, d);
        it = o > it ? o : it;
    }
    if (lane == 0) s_m[wave] = mcount, s_it[wave] = it;
    __syncthreads();
    mcount = 0;
    it = 0;
    for (int v = 0; v < 16; ++v) {
        mcount += s_m[v];
        it = s_it[v] > it ? s_it[v] : it;
    }
    const double bw = bandwidth[0], bw2 = bw * bw;
    int C = 0;                                     // uniform: every thread sees the same barrier results
    for (int p = 0; p < mcount; ++p) {
        const int i = w.order[p];
        double cv[MS_MAX_D / 64];
#pragma unroll
        for (int u = 0; u < MS_MAX_D / 64; ++u) {
            const int k = lane + 64 * u;
            cv[u] = k < D ? (double)w.msm[(int64_t)i * D + k] : 0.0;
        }
        bool hit = false;
        for (int q = wave; q < C && !hit; q += 16) {
            const float *mk = w.msm + (int64_t)kept[q] * D;
            double d2 = 0.0;
#pragma unroll
            for (int u = 0; u < MS_MAX_D / 64; ++u) {
                const int k = lane + 64 * u;
                if (k < D) {
                    const double d = cv[u] - (double)mk[k];
                    d2 = fma(d, d, d2);
                }
            }
            hit = ms_wave_sum(d2) <= bw2;
        }
        if (!__syncthreads_or(hit)) {
            if (tid == 0) kept[C] = (uint16_t)i;
            ++C;
        }
        __syncthreads();
    }
    for (int64_t e = tid; e < (int64_t)C * D; e += 1024) {
        const int c = (int)(e / D), k = (int)(e - (int64_t)c * D);
        centers[e] = w.msm[(int64_t)kept[c] * D + k];
    }
    if (tid == 0) {
        info[1] = C;
        info[2] = it;
    }
}

// ------------------------------------------------------------------------------------------------ predict

// 64 rows per workgroup (16 per wave), 16 NT centres per LDS block.  Lane l holds row (l & 15)'s dimensions 16g + 4(l>>4) .. +3 of every group g in
// registers (the B operand); the A operand is centre 16t + (l & 15) from LDS; acc[t][r] = x_(l&15) . c_(16t + 4(l>>4) + r).
template <int NQ, int NT, bool VEC>
__global__ __launch_bounds__(256) void ms_predict_kernel(const void *__restrict__ x, int dtype, int64_t N, int D, int64_t row_stride,
                                                         const float *__restrict__ centers, int C, int64_t *__restrict__ out) {
    extern __shared__ float smem[];
    __shared__ float s_cmax[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Dp = (D + 15) / 16 * 16, nq = Dp / 16, stride = Dp + 4;
    constexpr int CB = 16 * NT;
    const int nblk = (C + CB - 1) / CB;
    float *sC = smem;
    float *sCC = smem + CB * stride;
    float cmax2 = 0.0f;                           // max ||c||^2 over the blocks staged so far
    auto stage = [&](int blk) {
        __syncthreads();
        const int c0 = blk * CB;
        for (int e = tid; e < CB * Dp; e += 256) {
            const int r = e / Dp, k = e - r * Dp;
            sC[r * stride + k] = (c0 + r < C && k < D) ? centers[(int64_t)(c0 + r) * D + k] : 0.0f;
        }
        __syncthreads();
        float mx = 0.0f;
        if (tid < CB) {
            float s = 0.0f;
            for (int k = 0; k < D; ++k) s = fmaf(sC[tid * stride + k], sC[tid * stride + k], s);
            sCC[tid] = s;
            mx = c0 + tid < C ? s : 0.0f;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
        if (lane == 0) s_cmax[wave] = mx;
        __syncthreads();
        cmax2 = fmaxf(cmax2, fmaxf(fmaxf(s_cmax[0], s_cmax[1]), fmaxf(s_cmax[2], s_cmax[3])));
    };
    if (nblk == 1) stage(0);
    const int64_t ntiles = (N + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * 64 + 16 * wave + (lane & 15);
        const bool row_ok = row < N;
        f32x4 xv[NQ];
        float xx = 0.0f;
#pragma unroll
        for (int g = 0; g < NQ; ++g) {
            xv[g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const int k = 16 * g + 4 * (lane >> 4);
            if (g < nq && row_ok && k < D) {
                const int64_t e = row * row_stride + k;
                if constexpr (VEC) {
                    xv[g] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(x) + e);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) xv[g][s] = k + s < D ? ms_ld(x, dtype, e + s) : 0.0f;
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) xx = fmaf(xv[g][s], xv[g][s], xx);
            }
        }
        xx += __shfl_xor(xx, 16);
        xx += __shfl_xor(xx, 32);
        float best = INFINITY, second = INFINITY;
        int bi = 0;
        for (int blk = 0; blk < nblk; ++blk) {
            if (nblk > 1) stage(blk);
            f32x4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int g = 0; g < NQ; ++g) {
                if (g < nq) {
                    const int k = 16 * g + 4 * (lane >> 4);
                    f32x4 av[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) av[t] = *reinterpret_cast<const f32x4 *>(sC + (16 * t + (lane & 15)) * stride + k);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][s], xv[g][s], acc[t], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int cl = 16 * t + 4 * (lane >> 4) + r, c = blk * CB + cl;
                    if (c < C) {
                        const float sc = sCC[cl] - 2.0f * acc[t][r];
                        if (sc < best) {
                            second = best;
                            best = sc;
                            bi = c;
                        } else if (sc < second) {
                            second = sc;
                        }
                    }
                }
        }
        // the four lanes of a row (bits 4, 5), ties to the lower index
#pragma unroll
        for (int d = 16; d <= 32; d <<= 1) {
            const float ob = __shfl_xor(best, d), os = __shfl_xor(second, d);
            const int oi = __shfl_xor(bi, d);
            if (ob < best || (ob == best && oi < bi)) {
                second = fminf(best, os);
                best = ob;
                bi = oi;
            } else {
                second = fminf(second, ob);
            }
        }
        // |error| of each score <= (D + 1) u (||c||^2 + 2 ||x|| ||c||) (fp32 dot products of D terms and one subtraction, u = 2^-24); the gap of
        // two scores is trusted beyond twice that, with a further factor 2 for the rounding of the bound itself and of the gap
        const float cm = sqrtf(cmax2);
        const float guard = 4.0f * (float)(D + 2) * 5.9604645e-8f * (cmax2 + 2.0f * sqrtf(xx) * cm) + 1e-30f;
        const bool flag = row_ok && !(second - best > guard);
        unsigned long long fl = __ballot(flag) & 0xffffull;
        while (fl) {
            const int rr = __ffsll((long long)fl) - 1;
            fl &= fl - 1ull;
            const int64_t rrow = tile * 64 + 16 * wave + rr;
            double xd[MS_MAX_D / 64];
#pragma unroll
            for (int u = 0; u < MS_MAX_D / 64; ++u) {
                const int k = lane + 64 * u;
                xd[u] = k < D ? (double)ms_ld(x, dtype, rrow * row_stride + k) : 0.0;
            }
            double bd = 0.0;
            int bc = 0;
            for (int c = 0; c < C; ++c) {
                double d2 = 0.0;
#pragma unroll
                for (int u = 0; u < MS_MAX_D / 64; ++u) {
                    const int k = lane + 64 * u;
                    if (k < D) {
                        const double d = xd[u] - (double)centers[(int64_t)c * D + k];
                        d2 = fma(d, d, d2);
                    }
                }
                d2 = ms_wave_sum(d2);
                if (c == 0 || d2 < bd) {
                    bd = d2;
                    bc = c;
                }
            }
            if ((lane & 15) == rr) bi = bc;
        }
        if (row_ok && lane < 16) out[row] = bi;
    }
}

template <int NQ, int NT>
int ms_predict_launch(const void *x, int dtype, int64_t N, int D, int64_t row_stride, const float *centers, int C, int64_t *out, hipStream_t st) {
    const int Dp = (D + 15) / 16 * 16;
    const size_t lds = (size_t)16 * NT * (Dp + 4) * 4 + 16 * NT * 4;
    const int64_t ntiles = (N + 63) / 64;
    const unsigned grid = (unsigned)(ntiles < 2048 ? ntiles : 2048);
    const bool vec = dtype == PAG_F32 && row_stride % 4 == 0 && D % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    static bool attr = false;                     // up to 66 KB of LDS (Dp = 256 with 64 centres, Dp = 512 with 32)
    if (!attr) {
        hipFuncSetAttribute((const void *)ms_predict_kernel<NQ, NT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        hipFuncSetAttribute((const void *)ms_predict_kernel<NQ, NT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        attr = true;
    }
    if (vec) hipLaunchKernelGGL((ms_predict_kernel<NQ, NT, true>), dim3(grid), dim3(256), lds, st, x, dtype, N, D, row_stride, centers, C, out);
    else hipLaunchKernelGGL((ms_predict_kernel<NQ, NT, false>), dim3(grid), dim3(256), lds, st, x, dtype, N, D, row_stride, centers, C, out);
    return PAG_OK;
}

}      // namespace

extern "C" int64_t pag_meanshift_workspace_bytes(int B, int64_t P, int D) {
    return (B < 1 || P < 1 || (int64_t)B * P > MS_MAX_ROWS || D < 1 || D > MS_MAX_D) ? 0 : ms_ws_bytes((int64_t)B * P, D);
}

extern "C" int pag_meanshift_fit(const void *features, int dtype, int B, int64_t P, int D, int64_t image_stride, int64_t row_stride, const int64_t *labels,
                                 double quantile, int max_iter, int stages, void *workspace, int64_t workspace_bytes, float *means, double *bandwidth,
                                 float *centers, int32_t *info, void *stream) {
    PAG_CHECK_ARG(B >= 1 && P >= 1 && (int64_t)B * P <= MS_MAX_ROWS && D >= 1 && D <= MS_MAX_D && row_stride >= D && image_stride >= 0,
                  "pag_meanshift_fit: sizes (B %d, P %lld, D %d, row_stride %lld; B*P <= %lld, 1 <= D <= %d)", B, (long long)P, D, (long long)row_stride,
                  (long long)MS_MAX_ROWS, MS_MAX_D);
    PAG_CHECK_ARG(labels != nullptr || (int64_t)B * P <= MS_MAX_K, "pag_meanshift_fit: %lld rows without labels > K limit %d", (long long)B * P, MS_MAX_K);
    PAG_CHECK_ARG(dtype == PAG_F32 || dtype == PAG_BF16, "pag_meanshift_fit: dtype %d (f32 or bf16)", dtype);
    PAG_CHECK_ARG(stages >= 1 && stages <= 3, "pag_meanshift_fit: stages %d (1: class means, 2: + bandwidth, 3: + mean shift)", stages);
    PAG_CHECK_ARG(quantile >= 0.0 && quantile <= 1.0 && max_iter >= 0, "pag_meanshift_fit: quantile %g in [0, 1], max_iter %d >= 0", quantile, max_iter);
    PAG_CHECK_ARG(features && workspace && means && info && (stages < 2 || bandwidth) && (stages < 3 || centers), "pag_meanshift_fit: NULL input/output");
    const int64_t N = (int64_t)B * P;
    PAG_CHECK_ARG(workspace_bytes >= ms_ws_bytes(N, D), "pag_meanshift_fit: workspace %lld < %lld bytes", (long long)workspace_bytes,
                  (long long)ms_ws_bytes(N, D));
    hipStream_t st = (hipStream_t)stream;
    const MsWs w = ms_ws(workspace, N, D);
    const int Kcap = ms_kcap(N);
    if (labels) {
        const int64_t np = ms_pow2(N);
        hipLaunchKernelGGL(ms_sort_init_kernel, dim3((unsigned)(np / 256)), dim3(256), 0, st, labels, N, np, w);
        hipLaunchKernelGGL(ms_sort_local_kernel, dim3((unsigned)(np / MS_TILE)), dim3(1024), 0, st, (long long)P, (int64_t)2, (int64_t)MS_TILE, w);
        for (int64_t k = 2 * MS_TILE; k <= np; k <<= 1) {
            for (int64_t j = k / 2; j >= MS_TILE; j >>= 1)
                hipLaunchKernelGGL(ms_sort_global_kernel, dim3((unsigned)(np / 2 / 256)), dim3(256), 0, st, (long long)P, k, j, w);
            hipLaunchKernelGGL(ms_sort_local_kernel, dim3((unsigned)(np / MS_TILE)), dim3(1024), 0, st, (long long)P, k, k, w);
        }
        hipLaunchKernelGGL(ms_segments_kernel, dim3(1), dim3(1024), 0, st, N, (long long)P, w, info);
    } else {
        hipLaunchKernelGGL(ms_rows_info_kernel, dim3(1), dim3(1), 0, st, (int32_t)N, info);
    }
    hipLaunchKernelGGL(ms_means_kernel, dim3(Kcap), dim3(256), 0, st, features, dtype, (long long)P, D, image_stride, row_stride, labels != nullptr, Kcap,
                       w, (const int32_t *)info, means);
    if (stages >= 2) {
        hipLaunchKernelGGL(ms_kth_kernel, dim3((Kcap + MS_KROWS - 1) / MS_KROWS), dim3(256), 0, st, (const float *)means, Kcap, D, quantile, w,
                           (const int32_t *)info);
        hipLaunchKernelGGL(ms_bw_kernel, dim3(1), dim3(256), 0, st, w, (const int32_t *)info, bandwidth);
    }
    if (stages >= 3) {
        hipLaunchKernelGGL(ms_shift_kernel, dim3((Kcap + MS_SEEDS - 1) / MS_SEEDS), dim3(256), 0, st, (const float *)means, Kcap, D, max_iter, w,
                           (const int32_t *)info, (const double *)bandwidth);
        hipLaunchKernelGGL(ms_dedup_kernel, dim3((Kcap + 3) / 4), dim3(256), 0, st, Kcap, D, w, (const int32_t *)info);
        hipLaunchKernelGGL(ms_rank_kernel, dim3((Kcap + 3) / 4), dim3(256), 0, st, D, w, (const int32_t *)info);
        static bool attr = false;                 // the kept list: up to 64 KB of LDS next to the static part
        if (!attr) {
            hipFuncSetAttribute((const void *)ms_suppress_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
            attr = true;
        }
        hipLaunchKernelGGL(ms_suppress_kernel, dim3(1), dim3(1024), (size_t)Kcap * 2, st, D, w, (const double *)bandwidth, info, centers);
    }
    PAG_CHECK_LAUNCH("pag_meanshift_fit");
    return PAG_OK;
}

extern "C" int pag_meanshift_predict(const void *x, int dtype, int64_t N, int D, int64_t row_stride, const float *centers, int C, int64_t *labels_out,
                                     void *stream) {
    PAG_CHECK_ARG(N >= 0 && D >= 1 && D <= MS_MAX_D && C >= 1 && C <= MS_MAX_K && row_stride >= D,
                  "pag_meanshift_predict: sizes (N %lld, D %d, C %d, row_stride %lld; 1 <= D <= %d, 1 <= C <= %d)", (long long)N, D, C,
                  (long long)row_stride, MS_MAX_D, MS_MAX_K);
    PAG_CHECK_ARG(dtype == PAG_F32 || dtype == PAG_BF16, "pag_meanshift_predict: dtype %d (f32 or bf16)", dtype);
    if (N == 0) return PAG_OK;
    PAG_CHECK_ARG(x && centers && labels_out, "pag_meanshift_predict: NULL input/output");
    hipStream_t st = (hipStream_t)stream;
    const int Dp = (D + 15) / 16 * 16;
    if (Dp <= 64) ms_predict_launch<4, 4>(x, dtype, N, D, row_stride, centers, C, labels_out, st);
    else if (Dp <= 128) ms_predict_launch<8, 4>(x, dtype, N, D, row_stride, centers, C, labels_out, st);
    else if (Dp <= 256) ms_predict_launch<16, 4>(x, dtype, N, D, row_stride, centers, C, labels_out, st);
    else ms_predict_launch<32, 2>(x, dtype, N, D, row_stride, centers, C, labels_out, st);
    PAG_CHECK_LAUNCH("pag_meanshift_predict");
    return PAG_OK;
}
