// The ORDERED APPEND behind a running device counter that map.hip and voxelmap.hip build their outputs with: of n rows the kept ones, in row order,
// land at rows *count, *count + 1, ... of the output and *count grows by their number, in three launches and without the host:
//   1. oa_count_kernel<Pred>  one thread per row: the predicate, a 64-bit ballot per wave, the kept rows of each 256-row block -> block_count
//   2. oa_scan_kernel         one workgroup: exclusive scan of the block counts on top of the counter -> block_offset; counter += kept rows
//   3. the caller's write kernel: the predicate again (the same functor on the same inputs), oa_vote and the store of the wave's kept count before
//      its barrier, oa_wave_base after it; destination = wave base + rank.  Rows at or past the caller's capacity are counted and not written.
// A predicate is a functor with `int64_t n` and `bool operator()(int64_t i) const`, false for i >= n.  oa_append is the host side.  Integer work only.
#pragma once
#include "common.h"

namespace {

constexpr int OA_BLOCK = 256;
constexpr int OA_WAVES = OA_BLOCK / PAG_WAVE;

int64_t oa_blocks(int64_t n) { return (n + OA_BLOCK - 1) / OA_BLOCK; }
int64_t oa_align(int64_t b) { return (b + 255) / 256 * 256; }

template <class Pred>
__global__ __launch_bounds__(OA_BLOCK) void oa_count_kernel(Pred p, int32_t *__restrict__ block_count) {
    const int64_t i = (int64_t)blockIdx.x * OA_BLOCK + threadIdx.x;
    const unsigned long long m = __ballot(p(i));
    __shared__ int wc[OA_WAVES];
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < OA_WAVES; ++w) s += wc[w];
        block_count[blockIdx.x] = s;
    }
}

// One workgroup: block_offset[b] = *count + (kept rows of the blocks below b), then *count += all kept rows.  The counter is read and written by
// this workgroup alone, and the stream orders the calls, so appends of successive calls line up without the host.
__global__ __launch_bounds__(OA_BLOCK) void oa_scan_kernel(const int32_t *__restrict__ block_count, int64_t nb, int64_t *__restrict__ block_offset,
                                                           int64_t *__restrict__ count) {
    __shared__ int64_t sh[OA_BLOCK];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = *count;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nb; b0 += OA_BLOCK) {
        const int64_t b = b0 + threadIdx.x;
        const int64_t mine = b < nb ? (int64_t)block_count[b] : 0;
        sh[threadIdx.x] = mine;
        __syncthreads();
        for (int s = 1; s < OA_BLOCK; s <<= 1) {
            const int64_t add = (int)threadIdx.x >= s ? sh[threadIdx.x - s] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        const int64_t base = carry;
        if (b < nb) block_offset[b] = base + sh[threadIdx.x] - mine;
        __syncthreads();
        if (threadIdx.x == OA_BLOCK - 1) carry = base + sh[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}

// The write pass's preamble, in two steps around a barrier that the CALLER owns (it may fill LDS of its own between the steps).
struct OaVote {
    int rank, wcount;       // kept lanes below this one; kept lanes of the wave
};

// before the barrier: the wave's vote.  Lane 0 of every wave then stores wcount into wc[wave], the caller's __shared__ int [OA_WAVES].  That store
// is the caller's line: as a branch inside this helper it made the compiler place the rank behind it, and map_write_kernel and label_table_kernel
// came out in another instruction order (scripts/kernel_digest.py).
__device__ __forceinline__ OaVote oa_vote(bool keep) {
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(keep);
    return {(int)__popcll(m & ((1ull << lane) - 1ull)), (int)__popcll(m)};
}

// after the barrier: the destination of the wave's first kept row, from the wave counts stored before it
__device__ __forceinline__ int64_t oa_wave_base(const int64_t *__restrict__ block_offset, const int (&wc)[OA_WAVES]) {
    const int wave = threadIdx.x >> 6;
    int64_t base = block_offset[blockIdx.x];
    for (int q = 0; q < wave; ++q) base += wc[q];
    return base;
}

// The host side: the block tables at the start of `workspace` (block_offset at 0, block_count at align(nb * 8)), the count and scan launches, then
// write(grid, block, block_offset) launches the caller's write pass.  `name` is the public entry point, `ws_call` the public size call it documents.
template <class Pred, class Write>
int oa_append(const char *name, const char *ws_call, int64_t ws_need, Pred p, int64_t *count, void *workspace, int64_t workspace_bytes, hipStream_t st,
              Write write) {
    PAG_CHECK_ARG(workspace && workspace_bytes >= ws_need, "%s: workspace smaller than %s", name, ws_call);
    const int64_t nb = oa_blocks(p.n);
    int64_t *block_offset = (int64_t *)workspace;
    int32_t *block_count = (int32_t *)((char *)workspace + oa_align(nb * 8));
    const dim3 grid((unsigned)nb), block(OA_BLOCK);
    hipLaunchKernelGGL(oa_count_kernel<Pred>, grid, block, 0, st, p, block_count);
    hipLaunchKernelGGL(oa_scan_kernel, dim3(1), block, 0, st, (const int32_t *)block_count, nb, block_offset, count);
    write(grid, block, (const int64_t *)block_offset);
    PAG_CHECK_LAUNCH(name);
    return PAG_OK;
}

}  // namespace
