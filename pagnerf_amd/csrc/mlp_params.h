// What the decoder kernels of mlp.hip are launched with (mlp.hip and its family headers include this; nothing else does): the parameter
// structs the host layer fills (fwd_params / bwd_params in mlp.hip), the decoder families, and the grid of the 4-wave grid-strided kernels.
#pragma once
#include "mlp_common.h"

namespace {

struct FwdParams {
    const void *x1;
    const float *x2;
    const int32_t *x2_index;
    int k1, k2p, in_dim, in_pad, out_dim, act;
    const float *W[3];
    const float *b[3];
    void *out;
    void *hsave[2];
    int64_t M;
    int grp_L, grp_F;      // x1 in PAG_LAYOUT_XCD8 (bf16 [8][M][8]) when grp_L > 0
    float *stats;          // optional f32 [M,2]: (max logit * log2e, 1 / sum exp) of the output softmax
    float *col0_relu;      // optional f32 [M]: relu(x1[m][0]) (strided bf16 x1) - the density read off the colour decoder's input
    // companion head of mlp_fwd_wide_stats<.., PAIR = true>: a two-layer softmax decoder (out2_dim <= 8, bf16 out2 [M, out2_dim]) on the same x1
    const float *W2[2];
    const float *b2[2];
    void *out2;
    int out2_dim;
};

struct BwdParams {
    const void *grad_out;      // same dtype as `out` (autograd hands back the output's dtype); unused in rank-1 mode
    // rank-1 upstream gradient (composited panoptic heads): g[m][c] = g_scale[m] * g_ray[g_index[m]][c]
    const float *g_ray;
    const float *g_scale;
    const float *g_ray_scale;  // optional per-ray factor: g[m][c] = g_scale[m] * g_ray_scale[g_index[m]] * g_ray[g_index[m]][c]
    const int32_t *g_index;
    const void *out;
    int k1, in_dim, in_pad, out_dim, act;
    const float *W[3];
    const void *hsave[2];
    void *dz[3];
    void *dx1;
    int64_t M;
    int grp_L, grp_F;      // dx1 (and layer-0 weight columns) in PAG_LAYOUT_XCD8 order when grp_L > 0
    const float *stats;    // forward's softmax statistics + last-layer bias: the wide kernel recomputes the probabilities
    const float *b_last;
    int dx1_acc;           // XCD8 dx1: add to the existing contents instead of overwriting
    const float *dx_col0;  // strided dx1: f32 [M] added to column 0
    const float *dx_col0_gate;   // optional f32 [M]: the addend counts only where gate[m] > 0 (relu of that column)
    // fused weight gradients (mlp_bwd_fused, mlp_bwd_pair, mlp_bwd_wide_blocks): the forward's layer-0 input and one slab set per layer
    const void *x1;            // bf16: [8][M][8] (grp_L > 0) or [M, k1]
    const float *x2;           // optional f32 [R, k2p] gathered through x2_index (view embedding)
    const int32_t *x2_index;
    int k2p;
    float *slabs[3];           // per layer: f32 [4 * gridDim.x][rows_pad][WG_SLAB_COLS]  (cols 0..63 dW, col 64 db)
    const float *b[3];         // biases of the hidden layers: mlp_bwd_fused recomputes the hidden activations instead of reading saved ones
    float *dz0_slots;          // colour-like fused kernel, DZ0 == 2: f32 [(ceil(M / 32) + R)][64] column sums of dz_0 per (tile, ray), row = tile + ray
};

// mlp_bwd_pair: the two decoders of one launch
struct PairParams {
    BwdParams i, s;
};

// head_composite_fwd_kernel and the second argument of head_fwd_once_kernel
struct HeadCompParams {
    const int64_t *pack_start;
    const int32_t *ray_of_pack;
    int64_t P;
    const bf16_t *hidden;      // [M,64] last hidden layer (hidden_save of the forward)
    const float *W, *b;        // [out_dim,64], [out_dim]
    int out_dim;
    const float *stats;        // [M,2]
    int per_wave;              // 1: one WAVE per pack (short packs: the voxel regime has ~80 samples per ray), 0: one workgroup per pack
    const float *weights;      // [M]
    const float *alpha;        // [N]
    float *out;                // [N,out_dim]
};

// The decoder shapes that have kernels of their own, forward (mlp_fwd_fast, mlp_fwd_wide_stats, head_fwd_once_kernel) and backward (mlp_bwd_fused,
// mlp_bwd_wide_blocks); anything else runs the generic kernels.  The first three are the KIND template argument of mlp_fwd_fast / mlp_bwd_fused.
enum DecoderFamily {
    FAM_GENERIC = -1,
    FAM_DENSITY = 0,      // XCD8 input, no output activation, bf16 output of a multiple of 4 channels <= 32
    FAM_COLOUR = 1,       // strided bf16 [M,16] input + per-ray x2 [R,32], sigmoid, f32 output of <= 4 channels, the density read off column 0 of x1
    FAM_SOFTMAX = 2,      // XCD8 input, softmax, bf16 output of <= 8 channels (the semantic head)
    FAM_WIDE = 3,         // XCD8 input, three layers, softmax over 193 .. 224 channels kept as statistics + last hidden layer (the instance head)
};

// grid of the kernels whose 256-thread workgroups take four 32-sample tiles at a time
// (mlp_fwd_mfma, mlp_bwd_mfma, mlp_fwd_fast, mlp_fwd_density_colour)
inline unsigned mlp_grid(int64_t M) {
    int64_t tiles = (M + 31) / 32;
    int64_t blocks = (tiles + 3) / 4;
    int64_t cap = 256 * 6;   // a few workgroups per CU; tiles are grid-strided
    return (unsigned)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

}  // namespace
