// Ray sampling of a device-resident multiview dataset (pagnerf_amd/dataset.py; datasets/transforms/ray_sampler.py:17-40 and the collation of
// datasets/multiview_dataset.py:177-192 as one launch).
//
// Thread (b, j) computes pixel idx = slot slot_begin + j of the keyed permutation of [0, n) of view views[b] - pagnerf_amd.dataset.sample_indices is the
// definition, reproduced here bit for bit (uint32 arithmetic only) - and copies row idx of every mode to row b * slot_count + j of that mode's output:
//   key    s = DOMAIN; for w in (seed lo, seed hi, draw lo, draw hi, view): s = fmix32((s ^ w) + GOLDEN);   rk[r] = fmix32(s + (r + 1) * GOLDEN)
//   round  (L, R) -> (R, L ^ (fmix32(R ^ rk[r]) & mask)) on two h-bit halves, 2h = the smallest even width >= max(2, bit_length(n - 1)), 6 rounds
//   walk   x = slot; do x = rounds(x) while x >= n      (a bijection of [0, 2^2h) followed until it re-enters [0, n): a bijection of [0, n); 2^2h < 4n)
// fmix32 is the murmur3 finaliser.  {seed, draw} are read from device memory, so a captured graph replays with whatever pag_sample_advance left there.
// The launch is bound by the latency of B * slot_count * n_modes random row reads of a few bytes each; neighbouring threads write neighbouring rows, so
// the stores coalesce.  No atomics, no LDS, no workspace.  Bytes moved: B * slot_count * sum(row_bytes) written and as many read (a quarter for a
// uint8 -> f32 mode), in sectors of which a row uses a small part.
#include "common.h"

namespace {

constexpr uint32_t SAMPLE_GOLDEN = 0x9e3779b9u;
constexpr uint32_t SAMPLE_DOMAIN = 0x52415953u;      // "RAYS": pagnerf_amd.dataset.DOMAIN_RAYS (epoch_views uses another constant, on the host)
constexpr int SAMPLE_ROUNDS = 6;

struct SampleMode {
    const unsigned char *src;
    unsigned char *dst;
    int32_t row_bytes;        // of a destination row
    int32_t per_view;
    int32_t convert;
    int32_t width;            // bytes per copy element (byte copy) / source bytes per step (uint8 -> f32: 4 or 1)
};

struct SampleModes {
    SampleMode m[PAG_SAMPLE_MAX_MODES];
};

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

template <typename T>
__device__ __forceinline__ void copy_row(const unsigned char *__restrict__ s, unsigned char *__restrict__ d, int bytes, bool valid) {
    const int cnt = bytes / (int)sizeof(T);
    const T *sp = reinterpret_cast<const T *>(s);
    T *dp = reinterpret_cast<T *>(d);
    for (int i = 0; i < cnt; ++i) dp[i] = valid ? sp[i] : T{};
}

__global__ __launch_bounds__(256) void sample_batch_kernel(const int64_t *__restrict__ state, const int32_t *__restrict__ views, int num_views, uint32_t n,
                                                           int half_bits, uint32_t slot_begin, uint32_t slot_count, SampleModes modes, int n_modes,
                                                           int64_t *__restrict__ ray_idx, int32_t *__restrict__ cam_idx) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= slot_count) return;
    const int b = blockIdx.y;
    const int32_t view = views[b];
    const bool valid = (uint32_t)view < (uint32_t)num_views;           // a view outside the dataset reads nothing: zero rows, ray_idx -1
    const uint64_t seed = (uint64_t)state[0], draw = (uint64_t)state[1];
    uint32_t s = SAMPLE_DOMAIN;
    s = fmix32((s ^ (uint32_t)seed) + SAMPLE_GOLDEN);
    s = fmix32((s ^ (uint32_t)(seed >> 32)) + SAMPLE_GOLDEN);
    s = fmix32((s ^ (uint32_t)draw) + SAMPLE_GOLDEN);
    s = fmix32((s ^ (uint32_t)(draw >> 32)) + SAMPLE_GOLDEN);
    s = fmix32((s ^ (uint32_t)view) + SAMPLE_GOLDEN);
    uint32_t rk[SAMPLE_ROUNDS];
#pragma unroll
    for (int r = 0; r < SAMPLE_ROUNDS; ++r) rk[r] = fmix32(s + (uint32_t)(r + 1) * SAMPLE_GOLDEN);
    const uint32_t mask = (1u << half_bits) - 1u;
    uint32_t x = slot_begin + j;                                        // < min(k, n) <= n: checked on the host
    do {
        uint32_t l = x >> half_bits, r = x & mask;
#pragma unroll
        for (int i = 0; i < SAMPLE_ROUNDS; ++i) {
            const uint32_t t = l ^ (fmix32(r ^ rk[i]) & mask);
            l = r;
            r = t;
        }
        x = (l << half_bits) | r;
    } while (x >= n);
    const int64_t out_row = (int64_t)b * slot_count + j;
    if (ray_idx) ray_idx[out_row] = valid ? (int64_t)x : -1;
    if (cam_idx) cam_idx[out_row] = view;
    const int64_t view_row = valid ? (int64_t)view * n + x : 0;         // 64-bit: V * n * row_bytes passes 2^32 for a real dataset
    for (int m = 0; m < n_modes; ++m) {
        const SampleMode md = modes.m[m];
        const int64_t src_row = md.per_view ? view_row : (int64_t)(valid ? x : 0u);
        unsigned char *d = md.dst + out_row * md.row_bytes;
        if (md.convert == PAG_SAMPLE_U8_TO_F32) {
            const int C = md.row_bytes >> 2;
            const unsigned char *sp = md.src + src_row * C;
            float *dp = reinterpret_cast<float *>(d);
            if (md.width == 4) {
                for (int c = 0; c < C; c += 4) {
                    const uchar4 u = valid ? *reinterpret_cast<const uchar4 *>(sp + c) : uchar4{0, 0, 0, 0};
                    *reinterpret_cast<float4 *>(dp + c) = float4{(float)u.x / 255.0f, (float)u.y / 255.0f, (float)u.z / 255.0f, (float)u.w / 255.0f};
                }
            } else {
                for (int c = 0; c < C; ++c) dp[c] = valid ? (float)sp[c] / 255.0f : 0.0f;
            }
            continue;
        }
        const unsigned char *sp = md.src + src_row * md.row_bytes;
        switch (md.width) {
            case 16: copy_row<uint4>(sp, d, md.row_bytes, valid); break;
            case 8: copy_row<uint2>(sp, d, md.row_bytes, valid); break;
            case 4: copy_row<uint32_t>(sp, d, md.row_bytes, valid); break;
            case 2: copy_row<uint16_t>(sp, d, md.row_bytes, valid); break;
            default: copy_row<unsigned char>(sp, d, md.row_bytes, valid); break;
        }
    }
}

__global__ void sample_advance_kernel(int64_t *state) { state[1] += 1; }

// the widest of 16 / 8 / 4 / 2 / 1 bytes that divides the row and both base addresses (rows are row_bytes apart, so every row is then aligned)
int copy_width(const void *src, const void *dst, int64_t row_bytes) {
    const uint64_t bits = (uint64_t)(uintptr_t)src | (uint64_t)(uintptr_t)dst | (uint64_t)row_bytes;
    for (int w = 16; w > 1; w >>= 1)
        if ((bits & (uint64_t)(w - 1)) == 0) return w;
    return 1;
}

}  // namespace

extern "C" int pag_sample_copy_width(const void *src, const void *dst, int64_t row_bytes, int convert) {
    if (row_bytes <= 0) return 0;
    if (convert == PAG_SAMPLE_U8_TO_F32) {
        if (row_bytes % 4) return 0;
        // uchar4 in, float4 out: 4 source bytes per step
        return ((row_bytes / 4) % 4 == 0 && ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 15) == 0) ? 4 : 1;
    }
    if (convert != PAG_SAMPLE_COPY) return 0;
    return copy_width(src, dst, row_bytes);
}

extern "C" int pag_sample_batch(const int64_t *state, const int32_t *views, int B, int num_views, int64_t n, int64_t k, int64_t slot_begin, int64_t slot_count,
                                const pag_sample_mode *modes, int n_modes, int64_t *ray_idx, int32_t *cam_idx, void *stream) {
    PAG_CHECK_ARG(n >= 1 && n <= ((int64_t)1 << 30), "pag_sample_batch: n %lld not in [1,2^30]", (long long)n);
    PAG_CHECK_ARG(k >= 1, "pag_sample_batch: k %lld < 1", (long long)k);
    PAG_CHECK_ARG(B >= 0 && B <= 65535 && num_views >= 1, "pag_sample_batch: B %d not in [0,65535] or num_views %d < 1", B, num_views);
    PAG_CHECK_ARG(n_modes >= 0 && n_modes <= PAG_SAMPLE_MAX_MODES, "pag_sample_batch: n_modes %d not in [0,%d]", n_modes, PAG_SAMPLE_MAX_MODES);
    const int64_t take = k < n ? k : n;
    PAG_CHECK_ARG(slot_begin >= 0 && slot_count >= 0 && slot_begin + slot_count <= take, "pag_sample_batch: slots [%lld, %lld) outside [0, min(k, n) = %lld)",
                  (long long)slot_begin, (long long)(slot_begin + slot_count), (long long)take);
    PAG_CHECK_ARG(n_modes == 0 || modes, "pag_sample_batch: NULL modes");
    SampleModes km = {};
    for (int m = 0; m < n_modes; ++m) {
        const pag_sample_mode &md = modes[m];
        PAG_CHECK_ARG(md.row_bytes >= 1 && md.row_bytes <= ((int64_t)1 << 20), "pag_sample_batch: mode %d: row_bytes %lld not in [1,2^20]", m, (long long)md.row_bytes);
        PAG_CHECK_ARG(md.convert == PAG_SAMPLE_COPY || md.convert == PAG_SAMPLE_U8_TO_F32, "pag_sample_batch: mode %d: conversion code %d", m, md.convert);
        PAG_CHECK_ARG(md.convert != PAG_SAMPLE_U8_TO_F32 || md.row_bytes % 4 == 0, "pag_sample_batch: mode %d: conversion uint8 -> f32 needs row_bytes %lld to be a multiple of 4",
                      m, (long long)md.row_bytes);
        PAG_CHECK_ARG(md.src && md.dst, "pag_sample_batch: mode %d: NULL src / dst", m);
        km.m[m] = SampleMode{static_cast<const unsigned char *>(md.src), static_cast<unsigned char *>(md.dst), (int32_t)md.row_bytes, md.per_view ? 1 : 0, md.convert,
                             pag_sample_copy_width(md.src, md.dst, md.row_bytes, md.convert)};
    }
    if (B == 0 || slot_count == 0) return PAG_OK;
    PAG_CHECK_ARG(state && views, "pag_sample_batch: NULL state / views");
    int bits = 0;
    while (bits < 32 && ((uint64_t)(n - 1) >> bits)) ++bits;           // bit_length(n - 1)
    if (bits < 2) bits = 2;
    const int half_bits = (bits + 1) / 2;
    hipLaunchKernelGGL(sample_batch_kernel, dim3((unsigned)((slot_count + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, state, views, num_views, (uint32_t)n,
                       half_bits, (uint32_t)slot_begin, (uint32_t)slot_count, km, n_modes, ray_idx, cam_idx);
    PAG_CHECK_LAUNCH("pag_sample_batch");
    return PAG_OK;
}

extern "C" int pag_sample_advance(int64_t *state, void *stream) {
    PAG_CHECK_ARG(state, "pag_sample_advance: NULL state");
    hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
    PAG_CHECK_LAUNCH("pag_sample_advance");
    return PAG_OK;
}
