/*
 * pagnerf_hip.h - C ABI of libpagnerf_hip.so: the MI355X (gfx950) kernels behind the
 * kaolin-wisp grid / nef / tracer plugin API that PAg-NeRF's trainer drives.
 *
 * The reference is 100 % Python and has no FFI of its own; each entry point below replaces
 * a call the reference makes into a third-party CUDA package (or an in-tree torch op
 * sequence) at the cited file:line of the upstream repository.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is allocated by the caller (device memory
 *     unless the name ends in _host); the library owns nothing and keeps no global state
 *     except the thread-local last-error string.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and is safe to capture into a hipGraph (no allocation, no synchronisation).
 *   - return value: 0 on success, negative PAG_ERR_* otherwise (pag_last_error_string()).
 *   - "dtype" arguments take PAG_F32 / PAG_F16 / PAG_BF16.
 *   - strides are in ELEMENTS; a [M, C] row-major tensor has stride_m = C, stride_c = 1,
 *     a feature-major one stride_m = 1, stride_c = M.
 */
#ifndef PAGNERF_HIP_H
#define PAGNERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAG_ABI_VERSION 15

enum { PAG_F32 = 0, PAG_F16 = 1, PAG_BF16 = 2 };
enum { PAG_OK = 0, PAG_ERR_ARG = -1, PAG_ERR_LAUNCH = -2, PAG_ERR_UNSUPPORTED = -3 };
enum { PAG_ACT_NONE = 0, PAG_ACT_SIGMOID = 1, PAG_ACT_SOFTMAX = 2 };
enum { PAG_MLP_MFMA_BF16 = 0, PAG_MLP_FP32 = 1 };
enum { PAG_BG_BLACK = 0, PAG_BG_WHITE = 1 };
/* feature-tensor layouts of the encoders / decoder inputs:
 *   PAG_LAYOUT_STRIDED  [M, L*F] addressed through (stride_m, stride_c); column = level*F + f
 *   PAG_LAYOUT_XCD8     bf16 [8][M][8]: element e = j*F + f of group g holds level 8j + g (j even) or 8j + 7 - g (j odd) - every group,
 *                       i.e. every XCD of the encoders' launches, gets a mix of coarse and fine levels - zero padded (ABI 6; before: 8j + g)
 *                       (requires ceil(L/8)*F <= 8).  Strides are ignored. */
enum { PAG_LAYOUT_STRIDED = 0, PAG_LAYOUT_XCD8 = 1 };
/* `flags` of the encode entry points:
 *   PAG_ENC_HALF_COORDS  xyz is rounded to fp16 (round-to-nearest-even) and widened back to f32 before anything else uses it -
 *                        what `@torch.cuda.amp.custom_fwd(cast_inputs=torch.half)` + `.type(torch.float)` do to the coordinates under
 *                        the reference trainer's autocast (grids/permuto_grid.py:65,71; grids/hash_grid_tinycudann.py:36-41).
 *                        Forward, table gradient and position gradient must be called with the same flags. */
enum { PAG_ENC_HALF_COORDS = 1 };
#define PAG_MAX_LEVELS 32
#define PAG_MAX_FEATS 64

int pag_abi_version(void);
const char *pag_last_error_string(void);

/* ------------------------------------------------------------------------------------------
 * Grid feature interpolation ("encode")
 * ------------------------------------------------------------------------------------------ */

/* Multiresolution hash grid.  Replaces HashEmbedder.forward (grids/hash_grid_torch.py:95-108:
 * get_voxel_vertices :26-46, hash :13-24, trilinear_interp :69-93) as reached through
 * HashGridTorch.interpolate (:130-140); also the tinycudann-backed variant
 * (grids/hash_grid_tinycudann.py:36-47) with its own resolution list.
 *   xyz          f32 [M,3]
 *   tables       [L, 2^log2_T, F] (F = 2 or 4), PAG_F32 or PAG_F16
 *   resolutions_host  f32 [L]  (grids/hash_grid_torch.py:99)
 *   feat_scale_host   f32 [L*F] or NULL: per-feature multiplier (nef.lod_weights,
 *                     pc_nerf/panoptic_delta_nef.py:171)
 *   out          [M, L*F] via strides, PAG_F32 or PAG_BF16; column = level*F + f
 * fp32 tables + fp32 out reproduce the reference's fp32 op order (no FMA contraction). */
int pag_hash_encode_fwd(const float *xyz, int64_t M, const void *tables, int table_dtype,
                        int n_levels, int n_feat, int log2_T, const float *resolutions_host,
                        const float *feat_scale_host, void *out, int out_dtype,
                        int64_t out_stride_m, int64_t out_stride_c, int layout, int flags, void *stream);

/* d loss / d tables (what autograd through grids/hash_grid_torch.py:95-108 yields).
 *   grad_out  [M, L*F] via strides (PAG_F32 or PAG_BF16);  grad_tables f32 [L,T,F], ACCUMULATED
 *   into (caller zeroes).  workspace: see pag_encode_bwd_workspace_bytes(). */
int pag_hash_encode_bwd(const float *xyz, int64_t M, const void *grad_out, int grad_dtype,
                        int64_t g_stride_m, int64_t g_stride_c, int layout, int n_levels, int n_feat,
                        int log2_T, const float *resolutions_host, const float *feat_scale_host,
                        float *grad_tables, void *workspace, int64_t workspace_bytes, int flags, void *stream);

/* Permutohedral-lattice hash encoding.  Replaces permutohedral_encoding.PermutoEncoding's
 * forward as called at grids/permuto_grid.py:57-62,71.
 *   scale_factor_host f32 [L,3] = 1/(sqrt((i+1)(i+2)) * scale[l]), scale = np.geomspace(...)
 *                     (grids/permuto_grid.py:53)
 *   shift_host        f32 [L,3] per-level random shift
 *   capacity          table rows per level (need not be a power of two) */
int pag_permuto_encode_fwd(const float *xyz, int64_t M, const void *tables, int table_dtype,
                           int n_levels, int n_feat, uint32_t capacity,
                           const float *scale_factor_host, const float *shift_host,
                           const float *feat_scale_host, void *out, int out_dtype,
                           int64_t out_stride_m, int64_t out_stride_c, int layout, int flags, void *stream);

/* Same encoders writing  out = bf16(addend + bf16(features))  in the XCD8 layout (addend, out: bf16 [8][M][8]).
 * pc_nerf/panoptic_delta_nef.py:226 forms the panoptic features as `feats.detach() + delta`; with the main grid's
 * features as addend the delta grid's encoder emits that sum directly (bit-identical to the separate bf16 add). */
int pag_hash_encode_fwd_add(const float *xyz, int64_t M, const void *tables, int table_dtype,
                            int n_levels, int n_feat, int log2_T, const float *resolutions_host,
                            const float *feat_scale_host, const void *addend, void *out, int flags, void *stream);
int pag_permuto_encode_fwd_add(const float *xyz, int64_t M, const void *tables, int table_dtype,
                               int n_levels, int n_feat, uint32_t capacity,
                               const float *scale_factor_host, const float *shift_host,
                               const float *feat_scale_host, const void *addend, void *out, int flags, void *stream);

int pag_permuto_encode_bwd(const float *xyz, int64_t M, const void *grad_out, int grad_dtype,
                           int64_t g_stride_m, int64_t g_stride_c, int layout, int n_levels, int n_feat,
                           uint32_t capacity, const float *scale_factor_host,
                           const float *shift_host, const float *feat_scale_host,
                           float *grad_tables, void *workspace, int64_t workspace_bytes, int flags, void *stream);

/* As pag_hash_encode_bwd / pag_permuto_encode_bwd, but grad_tables is OVERWRITTEN: every row of every level is written
 * (zeros where no gradient arrived), so the caller need not clear the table first and the reduce pass does not read it.
 * Binned algorithm only (workspace required).  M == 0 leaves grad_tables untouched. */
int pag_hash_encode_bwd_set(const float *xyz, int64_t M, const void *grad_out, int grad_dtype,
                            int64_t g_stride_m, int64_t g_stride_c, int layout, int n_levels, int n_feat,
                            int log2_T, const float *resolutions_host, const float *feat_scale_host,
                            float *grad_tables, void *workspace, int64_t workspace_bytes, int flags, void *stream);
int pag_permuto_encode_bwd_set(const float *xyz, int64_t M, const void *grad_out, int grad_dtype,
                               int64_t g_stride_m, int64_t g_stride_c, int layout, int n_levels, int n_feat,
                               uint32_t capacity, const float *scale_factor_host, const float *shift_host,
                               const float *feat_scale_host, float *grad_tables, void *workspace,
                               int64_t workspace_bytes, int flags, void *stream);

/* d loss / d xyz of the two encoders (camera pose optimisation, pc_nerf/ba_pipeline.py:85-92: the
 * samples o + t*d depend on the learnable extrinsics).  The reference gets this from autograd through
 * grids/hash_grid_torch.py:69-108 (hash) and from permutohedral_encoding's position gradient
 * (permuto); within a cell / simplex the features are (tri)linear in xyz.
 *   tables     as in *_encode_fwd (F32 or F16);  grad_out / strides / layout as in *_encode_bwd
 *   d_xyz      f32 [M,3] (out, overwritten)
 *   workspace  >= 8*M*3 floats: per-XCD-group partial sums, added deterministically */
int pag_hash_encode_bwd_xyz(const float *xyz, int64_t M, const void *tables, int table_dtype,
                            const void *grad_out, int grad_dtype, int64_t g_stride_m,
                            int64_t g_stride_c, int layout, int n_levels, int n_feat, int log2_T,
                            const float *resolutions_host, const float *feat_scale_host,
                            float *d_xyz, void *workspace, int64_t workspace_bytes, int flags, void *stream);
int pag_permuto_encode_bwd_xyz(const float *xyz, int64_t M, const void *tables, int table_dtype,
                               const void *grad_out, int grad_dtype, int64_t g_stride_m,
                               int64_t g_stride_c, int layout, int n_levels, int n_feat,
                               uint32_t capacity, const float *scale_factor_host,
                               const float *shift_host, const float *feat_scale_host, float *d_xyz,
                               void *workspace, int64_t workspace_bytes, int flags, void *stream);

/* Scratch size for the atomic-free ("binned") backward of either encoder: n_vertices = 8 (hash) or
 * 4 (permuto), rows_per_level = 2^log2_T or capacity.  The caller allocates it (device memory) and
 * passes it as `workspace`; with workspace == NULL the backward falls back to per-vertex fp32
 * global atomics (slow on MI355X, kept as the reference path for tests). */
int64_t pag_encode_bwd_workspace_bytes(int64_t M, int n_levels, int n_feat, int n_vertices,
                                       int64_t rows_per_level);

/* ------------------------------------------------------------------------------------------
 * Tiny-MLP decoders
 * ------------------------------------------------------------------------------------------ */

/* One wisp BasicDecoder (n_layers Linear layers, ReLU between, none after the last) fused in
 * one launch, with an optional output activation.  Replaces decoder_density / decoder_color /
 * decoder_semantics / decoder_inst (pc_nerf/panoptic_nef.py:114-164) as applied at
 * pc_nerf/panoptic_delta_nef.py:184,203,240-243,250-255, including the input concat of
 * :198-199 (x2 rows are gathered per sample through x2_index, so the view embedding is never
 * repeated in memory).
 *   x1        [M, k1] row-major (x1_dtype F32 or BF16), k1 % 8 == 0
 *   x2        f32 [R, k2p] row-major or NULL; k2p % 8 == 0 (caller zero-pads), x2_index i32 [M]
 *   W[i]      f32 [out_i, in_i] row-major (nn.Linear.weight), b[i] f32 [out_i];
 *             in_0 = in_dim <= k1 + k2p (columns beyond in_dim are treated as absent)
 *   n_layers  2 or 3; hidden width = 64; out_dim <= 224
 *   out       [M, out_dim] row-major (out_dtype F32 or BF16), after out_act
 *   hidden_save[i]  bf16 (MFMA mode) or f32 (FP32 mode) [M, 64] row-major post-ReLU
 *             activations of hidden layer i, or NULL when no backward will follow
 *   mode      PAG_MLP_MFMA_BF16: bf16 operands, fp32 accumulate on the matrix cores;
 *             PAG_MLP_FP32: fp32 FMA chain in k order (parity path) */
struct pag_head_composite_args;
typedef struct pag_mlp_fwd_args {
    const void *x1; int x1_dtype; int k1;
    int x1_layout; int x1_levels; int x1_feats;   /* PAG_LAYOUT_XCD8: x1 is the encoders' bf16 [8][M][8]
                                                     output for (levels, feats); k1 = 64, in_dim = levels*feats */
    const float *x2; int k2p; const int32_t *x2_index;
    int in_dim; int n_layers; int out_dim;
    const float *W[3]; const float *b[3];
    int out_act;
    void *out; int out_dtype;
    void *hidden_save[2];
    int mode;
    float *softmax_stats;   /* optional (MFMA mode, out_act SOFTMAX, out_dim > 64): f32 [M,2] = (max logit * log2(e),
                               1 / sum exp) per sample, from which the backward and pag_head_composite_fwd rebuild the
                               probabilities; `out` may then be NULL (nothing but the statistics is written) */
    float *x1_col0_relu;    /* optional (MFMA mode, strided bf16 x1, out_dim <= 64): f32 [M] = relu(x1[m][0]) written by the
                               same launch - the density pc_nerf/panoptic_delta_nef.py:188 reads off column 0 of the density
                               decoder's output, which is this (colour) decoder's x1 */
    /* Optional, statistics-only wide softmax head only (out NULL): a second decoder on the SAME XCD8 input - two layers, softmax,
     * out_dim <= 8, bf16 out, no hidden_save (the semantic head next to the instance head) - evaluated in this call's launch while the
     * tile is in registers.  The caller does not call pag_mlp_fwd for it.  pag_mlp_fwd_pair_supported() tells whether the pair qualifies. */
    const struct pag_mlp_fwd_args *pair;
    /* Optional (ABI 12), statistics-only wide softmax head only: the per-ray weighted sum of pag_head_composite_fwd formed in the SAME launch, in one pass
     * over the logits (each logit and each exponential once instead of twice) - out[ray] = alpha[ray] * sum_i weights[i] * softmax(...)[i] over the ray's
     * pack.  softmax_stats and hidden_save[1] are written as without it (for the backward); samples past pack_start[P] (fillers of a padded batch) get
     * statistics that rebuild to probability 0 and a zero hidden row.  The caller does not call pag_head_composite_fwd.
     * pag_mlp_fwd_composite_supported() tells whether the arguments qualify (pair included). */
    const struct pag_head_composite_args *composite;
    /* Optional (ABI 12), colour-like decoder only (strided bf16 x1 [M,16] + per-ray x2, three layers, sigmoid, x1_col0_relu, no hidden_save): the
     * density-like decoder whose `out` IS this decoder's x1 (XCD8 bf16 input, two layers, no activation, out_dim 16, bf16 out, no hidden_save) is
     * evaluated in the same launch - its output is written as without this field and handed on in registers (pc_nerf/panoptic_delta_nef.py:184 ->
     * :198-203 as one launch instead of two; bit-identical outputs).  The caller does not call pag_mlp_fwd for the producer.
     * pag_mlp_fwd_producer_supported() tells whether the two argument blocks qualify. */
    const struct pag_mlp_fwd_args *x1_producer;
} pag_mlp_fwd_args;
typedef struct pag_head_composite_args {
    const int64_t *pack_start; const int32_t *ray_of_pack; int64_t P;      /* as pag_head_composite_fwd */
    const float *weights;       /* f32 [M] compositing weights w_i */
    const float *alpha;         /* f32 [N] */
    float *out;                 /* f32 [N, out_dim]: rows of rays that have a pack are overwritten */
    int64_t n_samples;          /* pack_start[P] as the host knows it (0 = unknown): a speed hint only */
} pag_head_composite_args;
int pag_mlp_fwd(const pag_mlp_fwd_args *args, int64_t M, void *stream);
int pag_mlp_fwd_pair_supported(const pag_mlp_fwd_args *args, const pag_mlp_fwd_args *pair);
int pag_mlp_fwd_composite_supported(const pag_mlp_fwd_args *args, int64_t M);
int pag_mlp_fwd_producer_supported(const pag_mlp_fwd_args *args, const pag_mlp_fwd_args *producer, int64_t M);

/* Data gradients of pag_mlp_fwd.  grad_out is d loss / d (activated output); `out` is the
 * activated output saved from the forward (needed for sigmoid / softmax).  Writes
 *   dz[i]   [M, out_i (padded to 64 for hidden layers)] pre-activation gradients of layer i
 *           (bf16 in MFMA mode, f32 in FP32 mode); dz of the last layer is [M, out_dim]
 *   dx1     [M, k1] (dx1_dtype) or NULL
 * Weight gradients are dz[i]^T @ input_i - a plain GEMM left to the caller's BLAS. */
typedef struct pag_mlp_bwd_args {
    const void *grad_out; const void *out; int out_dtype; int out_act;   /* grad_out has out's dtype */
    int k1; int in_dim; int n_layers; int out_dim;
    int x1_layout; int x1_levels; int x1_feats;   /* as in pag_mlp_fwd_args: dx1 is then written as bf16 [8][M][8] */
    const float *W[3];
    const void *hidden_save[2];
    void *dz[3];          /* with wgrad_workspace (fused weight gradients) no dz tensor is written - except dz[0] (bf16 [M,64], optional) by the
                           * colour-like kernel: the caller sums it per ray for the gradient of the per-ray input x2 (pose optimisation) */
    void *dx1; int dx1_dtype;
    int mode;
    /* Optional rank-1 upstream gradient (MFMA mode): grad_out[m][c] = g_scale[m] * g_ray[g_index[m]][c] with
     * g_ray f32 [N, out_dim].  This is exactly d(feats) of tracers/panoptic_packed_rf_tracer.py:197-205
     * (alpha * w_m * d out[ray]) - passing it in this form means the [M, out_dim] gradient of the composited
     * semantic / instance probabilities is never materialised.  grad_out may then be NULL. */
    const float *g_ray; const float *g_scale; const int32_t *g_index;
    /* Optional (MFMA mode, out_act SOFTMAX, out_dim > 64, bf16 out): with the forward's softmax_stats and the last layer's
     * bias the wide-head backward recomputes the probabilities from hidden_save (4 MFMAs per 32-channel block on idle
     * matrix cores) instead of streaming the [M, out_dim] output through twice; `out` may then be NULL. */
    const float *softmax_stats; const float *b_last;
    int dx1_accumulate;   /* XCD8 dx1 only: add this decoder's input gradient to what dx1 already holds (two heads on the
                             same panoptic features - saves the separate gradient-sum pass) */
    const float *dx1_col0_add;   /* optional f32 [M] (strided dx1, MFMA mode, out_dim <= 64): added to column 0 of dx1 - the
                                    gradient of the density that pc_nerf/panoptic_delta_nef.py:188 reads off column 0 of the
                                    density decoder's output, which is also this (colour) decoder's x1 */
    const float *dx1_col0_gate;  /* optional f32 [M] with dx1_col0_add: the addend is applied only where gate[m] > 0 (the relu of
                                    that column: pass the forward's x1_col0_relu) */
    const float *g_ray_scale;    /* optional f32 [N] with the rank-1 gradient: grad_out[m][c] = g_scale[m] * g_ray_scale[g_index[m]] *
                                    g_ray[g_index[m]][c] (g_scale = the compositing weights w_m, g_ray_scale = the rays' alpha) */
    /* Fused weight gradients (optional; pag_mlp_bwd_fused_supported() == 1).  With wgrad_workspace != NULL the launch also forms
     * dW[i] = dz_i^T . input_i (f32 [out_i, in_i], nn.Linear layout) and db[i] = column sums of dz_i for every layer, from the
     * tiles it holds anyway: no dz tensor is written (dz[] may be NULL) and no second pass re-reads [M,64] activations
     * (536 MB per 64 x 64 layer at M = 2.1 M - the separate pag_mlp_wgrad_batch ran at the HBM rate on exactly those bytes).
     * Needs the forward's layer-0 input: x1 (bf16; layout / levels / feats as above) and, if the forward had it, x2 / x2_index.
     * wgrad_workspace: device scratch of pag_mlp_bwd_fused_workspace_bytes(args, M) bytes (per-wave partial sums, reduced in a
     * fixed order by a second tiny launch: deterministic). */
    const void *x1; int x1_dtype; const float *x2; int k2p; const int32_t *x2_index;
    float *wgrad_workspace; int64_t wgrad_workspace_bytes;
    float *dW[3]; float *db[3];
    /* Fused mode RECOMPUTES the hidden activations from x1 (same MFMA sequence as pag_mlp_fwd: bit-identical) instead of reading
     * hidden_save - the forward then need not write them (pag_mlp_fwd_args.hidden_save = NULL): 268 MB less each way per hidden
     * layer at M = 2.1 M.  Needs the hidden layers' biases b[0 .. n_layers-2]; hidden_save[] may be NULL except, for the wide
     * softmax head, the LAST hidden layer's (the probabilities are rebuilt from it). */
    const float *b[3];
    /* Optional, wide softmax head with wgrad_workspace only: a second decoder on the SAME XCD8 input - a two-layer softmax head with
     * out_dim <= 8 (the semantic head next to the instance head), filled in as for its own pag_mlp_bwd call (fused workspace, dW, db,
     * b[0], rank-1 gradient, dx1 = this decoder's dx1 with dx1_accumulate = 1).  Its backward then runs inside this call, in the launch of
     * the layers below the wide output layer: one read of the input and one write of the summed input gradient for both decoders.
     * The caller does not call pag_mlp_bwd for it. */
    const struct pag_mlp_bwd_args *pair;
    /* Optional (ABI 11), colour-like decoder with wgrad_workspace and a per-ray x2 whose x2_index is NON-DECREASING (samples packed ray by ray): instead
     * of the [M,64] dz[0] tensor the launch writes one f32 [64] row per (32-sample tile, ray) - the column sums of dz_0 over that ray's samples of the
     * tile, formed on the matrix cores - at row tile + ray of dz0_slots (pag_mlp_dz0_slots_bytes(M, R) bytes, R = rows of x2); pag_mlp_dz0_slots_sum adds
     * a ray's rows: the per-ray sum of dz_0 (x W_0[:, k1:] = the gradient of x2) for 8 B per sample instead of 128 written and 128 read again. */
    float *dz0_slots;
} pag_mlp_bwd_args;
int pag_mlp_bwd(const pag_mlp_bwd_args *args, int64_t M, void *stream);
int64_t pag_mlp_dz0_slots_bytes(int64_t M, int64_t R);
/* out f32 [R,64] = per-ray sums of pag_mlp_bwd_args.dz0_slots; pack_start i64 [R+1] = the rays' sample ranges (one pack per ray).  (ABI 11) */
int pag_mlp_dz0_slots_sum(const int64_t *pack_start, int64_t R, const float *slots, float *out, void *stream);
/* 1 when pag_mlp_bwd has a fused weight-gradient kernel for these (fully filled in, wgrad_workspace aside) arguments.  Three
 * decoder shapes are covered - the narrow decoders of pc_nerf/panoptic_nef.py:114-164 on the bf16 path:
 *   density-like   XCD8 bf16 x1, dense bf16 grad_out, no output activation, out_dim % 4 == 0, XCD8 bf16 dx1
 *   colour-like    bf16 x1 [M,16] + f32 x2 [R,32] through x2_index, dense f32 grad_out, sigmoid, out_dim <= 4, bf16 dx1 [M,16] with
 *                  dx1_col0_add + dx1_col0_gate
 *   semantic-like  XCD8 bf16 x1, rank-1 gradient (g_ray, g_scale, g_index, g_ray_scale), softmax with the saved bf16 `out`,
 *                  out_dim <= 8, XCD8 bf16 dx1 (dx1_accumulate allowed)
 *   wide softmax   XCD8 bf16 x1, rank-1 gradient, softmax_stats + b_last (the instance head: 3 layers, 192 < out_dim <= 224), XCD8
 *                  bf16 dx1: two launches - the output layer with its weight gradient (the [M, out_dim] softmax gradient is never
 *                  written), then the two layers below it on the hidden gradient
 * the first three with 2 or 3 layers, out_dim <= 32, and input column 63 free (XCD8: staged position 63 is padding; it carries the
 * constant 1 whose weight gradient is the layer-0 bias gradient).  Anything else: dz[] + pag_mlp_wgrad_batch. */
int pag_mlp_bwd_fused_supported(const pag_mlp_bwd_args *args);
/* The wide softmax kernels address the [M,64] bf16 tensors with 32-bit byte offsets: pag_mlp_bwd refuses M above this on that path
 * (PAG_ERR_ARG; callers split the batch or leave wgrad_workspace NULL). */
#define PAG_MLP_FUSED_WIDE_MAX_M ((int64_t)1 << 24)
int64_t pag_mlp_bwd_fused_workspace_bytes(const pag_mlp_bwd_args *args, int64_t M);
/* 1 when `pair` (fully filled in) can ride in args' call as pag_mlp_bwd_args.pair: args is a wide softmax head, pair a two-layer narrow
 * softmax head on the same XCD8 input that accumulates into args->dx1. */
int pag_mlp_bwd_pair_supported(const pag_mlp_bwd_args *args, const pag_mlp_bwd_args *pair);

/* One affine map of the XCD8 features: the activation-free `decoder_delta_density` of pc_nerf/panoptic_dd_nef.py:49-56, :238
 * (its layers composed to one [n_out, in_dim] matrix by the caller; n_out <= 8).
 *   fwd     out f32 [M, n_out] = x . W^T + b        x: bf16 [8][M][8] (PAG_LAYOUT_XCD8 of x_levels x x_feats features), W f32 [n_out, in_dim]
 *   bwd_dx  dx bf16 [8][M][8] = grad_out [M, n_out] . W   (padding positions 0)
 * Weight gradients: pag_mlp_wgrad_batch with grad_out (bf16) as `dz` and x as `a1`. */
int pag_affine_xcd8_fwd(const void *x, int64_t M, int x_levels, int x_feats, const float *W, const float *b, int n_out, int in_dim,
                        float *out, void *stream);
int pag_affine_xcd8_bwd_dx(const float *grad_out, int64_t M, int x_levels, int x_feats, const float *W, int n_out, int in_dim, void *dx,
                           void *stream);

/* Wide softmax head fused with the per-ray weighted sum of tracers/panoptic_packed_rf_tracer.py:197-205:
 *   out[ray][c] = alpha[ray] * sum_{i in pack} weights[i] * softmax(W_last . hidden[i] + b_last)[c]
 * from the forward's saved last hidden layer (bf16 [M,64]) and softmax_stats (pag_mlp_fwd with out = NULL): the
 * [M, out_dim] probabilities are rebuilt tile by tile and never stored.  64 < out_dim <= 224; out f32 [N,out_dim]
 * (rows of rays that have a pack are overwritten).  n_samples = pack_start[P] as the host knows it (0 = unknown): short packs
 * (fewer than ~5 tiles of 32 samples on average: the voxel march after the first prune) are processed one per wave instead of
 * one per workgroup - same sums in the same order per pack, a speed hint only. */
int pag_head_composite_fwd(const int64_t *pack_start, const int32_t *ray_of_pack, int64_t P,
                           const void *hidden, const float *W_last, const float *b_last, int out_dim,
                           const float *softmax_stats, const float *weights, const float *alpha,
                           float *out, int64_t n_samples, void *stream);

/* Weight and bias gradients of one Linear layer of pag_mlp_fwd (MFMA mode):
 *   dW[o][i] = sum_m dz[m][o] * a[m][i],  db[o] = sum_m dz[m][o]
 * with a = the layer's input: [M,k1] (F32 or BF16) optionally followed by gathered per-ray columns
 * a2[a2_index[m]] (layer 0 of the colour decoder), n_in <= 64 columns used.
 *   dz      bf16 [M, dz_cols] (dz_cols >= n_out; the hidden layers' dz are [M,64])
 *   a1_layout PAG_LAYOUT_XCD8: a1 is the encoders' bf16 [8][M][8] tensor (k1 = n_in = 64); slab column p
 *           then holds the gradient of feature column level*F+f with p = 8*(level%8) + (level/8)*F + f.
 *   slabs   f32 [n_blocks][ceil(n_out/32)*32][96] per-workgroup partial sums written (not
 *           accumulated) by the kernel: columns 0..n_in-1 = dW rows, column 64 = db.  The caller sums
 *           over n_blocks (n_blocks = pag_mlp_wgrad_blocks(M)) - deterministic, no atomics. */
int pag_mlp_wgrad_blocks(int64_t M);
int pag_mlp_wgrad(const void *dz, int dz_cols, int n_out, const void *a1, int a1_dtype,
                  int a1_layout, int k1, const float *a2, int k2p, const int32_t *a2_index, int n_in,
                  float *slabs, int n_blocks, int64_t M, void *stream);

/* Deterministic sum of those slabs into the final gradients: dW f32 [n_out, n_in] (for XCD8 inputs the staged
 * positions are mapped back to feature columns level*F + f) and db f32 [n_out]. */
int pag_mlp_wgrad_finish(const float *slabs, int n_blocks, int n_out, int n_in, int a1_layout,
                         int a1_levels, int a1_feats, float *dW, float *db, void *stream);

/* Every weight gradient of one decoder in 2-3 launches: layers with the same kernel variant share one slab launch
 * (grid.y = layer), one finish launch sums all of them.  Same arithmetic (and bits) as pag_mlp_wgrad +
 * pag_mlp_wgrad_finish per layer.  Field meanings as in those two; n_layers <= 6; M >= 1. */
typedef struct pag_wgrad_layer {
    const void *dz;          /* bf16 [M, dz_cols] */
    int dz_cols, n_out;
    const void *a1;          /* layer input (a1_dtype, a1_layout, k1 columns) */
    int a1_dtype, a1_layout, k1;
    const float *a2;         /* gathered second input or NULL */
    int k2p;
    const int32_t *a2_index;
    int n_in;
    float *slabs;            /* f32 [n_blocks, round32(n_out), 96] */
    int n_blocks;
    int a1_levels, a1_feats; /* XCD8 inputs only */
    float *dW, *db;          /* f32 [n_out, n_in] (XCD8 inputs: [n_out, a1_levels * a1_feats]), f32 [n_out] */
} pag_wgrad_layer;
int pag_mlp_wgrad_batch(const pag_wgrad_layer *layers, int n_layers, int64_t M, void *stream);

/* ------------------------------------------------------------------------------------------
 * Ray march (wisp OctreeAS.raymarch, 'ray' mode) - tracers/panoptic_packed_rf_tracer.py:85-86
 * ------------------------------------------------------------------------------------------ */

/* Pass 1: per-ray number of surviving samples.
 *   origins, dirs f32 [N,3]; tvals f32 [S] = linspace(0,1,S); jitter f32 [N,S] in [0,1)
 *   occupancy_bits u32 [R^3/32] (bit (x*R+y)*R+z), R = 2^blas_level, or NULL for a dense grid
 *   counts i32 [N] */
int pag_raymarch_count(const float *origins, const float *dirs, int64_t N, int S,
                       const float *tvals, const float *jitter, float dist_min, float dist_max,
                       const uint32_t *occupancy_bits, int blas_level, int32_t *counts,
                       void *stream);
/* pack_start i64 [N+1]: exclusive prefix sums of counts i32 [N] (pack_start[N] = total number of samples) - the write
 * offsets pag_raymarch_pack takes and the per-ray pack table of the compositing kernels (kaolin's
 * mark_pack_boundaries / cumsum bookkeeping, tracers/panoptic_packed_rf_tracer.py:114).  One workgroup.
 * total_host (optional): device-accessible PINNED HOST memory that also receives pack_start[N] (system-scope release store):
 * a host that preset it to a negative value can poll it instead of issuing a stream-synchronising read-back. */
int pag_pack_offsets(const int32_t *counts, int64_t N, int64_t *pack_start, int64_t *total_host, void *stream);
/* Pad a packed batch to `capacity` samples (a multiple of samples_per_entry) WITHOUT the host knowing the sample count: the
 * M = pack_start[N] real samples are followed by filler samples that belong to no pack (coordinates 0, depth 0, delta 0, ray index
 * N - 1; pack_start is not modified).  Per-ray kernels never touch them; per-sample kernels compute on them and the results are
 * ignored; with the per-sample gradient tensors of the compositing backward zero-filled past M they carry zero gradient.  The step
 * after the march then has shapes that do not depend on device data and can be replayed as a HIP graph (pagnerf_amd/graphs.py - the
 * reference's boolean-mask indexing, wisp OctreeAS.raymarch, forces a host read-back instead).
 * M > capacity: no filler is written (the caller learns M from pag_pack_offsets' total_host, discards the step and falls back to
 * exact shapes).  pack_start_clamped i64 [N + 1] (optional, ABI 8) receives min(pack_start[r], capacity): the pack table to hand to
 * every launch that is queued on capacity-sized views BEFORE the host knows M - equal to pack_start when the batch fits, a
 * truncated batch otherwise, so that no per-ray kernel ever indexes a per-sample tensor past `capacity`.
 * ridx_sample i32 [capacity] / ridx_entry i32 [capacity / k] / ridx64 i64 [capacity / k] may be NULL; pidx i32 [capacity / k]. */
int pag_pad_packed(const int64_t *pack_start, int64_t N, int64_t capacity, int samples_per_entry, float *samples, float *depths,
                   float *deltas, int32_t *ridx_sample, int32_t *ridx_entry, int64_t *ridx64, int32_t *pidx,
                   uint8_t *boundary, int64_t *pack_start_clamped, void *stream);

/* pag_pack_offsets + pag_pad_packed + the copy of the ray directions (dirs_src f32 [N,3] -> dirs_dst, both may be NULL) as ONE
 * launch (16 workgroups: each repeats the scan for the total, the first writes the tables, all share the filler stores and the
 * copy): the head of a graph-replayed step (pagnerf_amd/graphs.py).  Arguments as the two entry points';
 * pack_start_clamped is required.  The fillers lie behind the samples the pack pass writes, so it may be queued before that pass. (ABI 9) */
int pag_pack_offsets_pad(const int32_t *counts, int64_t N, int64_t *pack_start, int64_t *total_host, int64_t capacity,
                         int samples_per_entry, float *samples, float *depths, float *deltas, int32_t *ridx_sample,
                         int32_t *ridx_entry, int64_t *ridx64, int32_t *pidx, uint8_t *boundary, int64_t *pack_start_clamped,
                         const float *dirs_src, float *dirs_dst, void *stream);

/* Up to 16 device-to-device copies in ONE launch (pagnerf_amd/graphs.py: the caller-owned copies of a graph replay's static
 * outputs, the upstream gradients into the backward graph's static inputs).  dst / src: host arrays of device pointers, nbytes[i]
 * bytes each (0 = skipped); 16-byte pieces where both pointers are 16-byte aligned.  (ABI 9) */
int pag_copy_batch(int n, void *const *dst, const void *const *src, const int64_t *nbytes, void *stream);

/* View-direction embedding of the colour decoder (wisp PositionalEmbedder on -ray_d, pc_nerf/panoptic_delta_nef.py:196-200):
 * out f32 [R, width] = (-d, sin(-d 2^k) for k < n_freq, cos(-d 2^k) for k < n_freq), frequency-major, zero padded;
 * dirs f32 [R,3], width >= 3 + 6 n_freq. */
int pag_view_embed(const float *dirs, int64_t R, int n_freq, int width, float *out, void *stream);

/* Pass 2: pack.  offsets i64 [N] = exclusive prefix sum of counts.
 *   ridx i32 [M], pidx i32 [M] (linear cell id), samples f32 [M,3], depths f32 [M],
 *   deltas f32 [M], boundary u8 [M] (1 at the first sample of each ray);
 *   ridx64 i64 [M] or NULL: the ray ids once more in the int64 form wisp's raymarch returns */
int pag_raymarch_pack(const float *origins, const float *dirs, int64_t N, int S,
                      const float *tvals, const float *jitter, float dist_min, float dist_max,
                      const uint32_t *occupancy_bits, int blas_level, const int64_t *offsets,
                      int32_t *ridx, int32_t *pidx, float *samples, float *depths, float *deltas,
                      uint8_t *boundary, int64_t *ridx64, void *stream);

/* 'voxel' mode (wisp OctreeAS.raymarch after pc_nerf/trainer.py:362-366 switches the tracer): every ray is walked
 * through the 2^blas_level occupancy grid (3-D DDA); each occupied cell it crosses (a "nugget") receives
 * samples_per_voxel samples.  ONE walk per ray: _count_nuggets records every kept nugget (t_in, t_out) and its cell and
 * counts them; _pack_nuggets (offsets = pag_pack_offsets() of the counts) turns them into the packed arrays in parallel
 * (one wave per ray):
 *   ridx i32 [M'], pidx i32 [M'] per nugget; samples f32 [M',k,3], depths f32 [M',k], deltas f32 [M'*k],
 *   boundary u8 [M'*k] (1 at the first sample of a ray's first nugget) - the shapes
 *   tracers/panoptic_packed_rf_tracer.py:88-108 indexes.
 * counts (out, i32 [N]) are in SAMPLES (nuggets * samples_per_voxel): pag_pack_offsets() of them is at once the pack
 * pass's offset table and the compositing kernels' pack_start (one pack per ray, empty packs allowed).
 *   max_travel   the travel filter of tracers/panoptic_packed_rf_tracer.py:88-108 applied inside the march: a nugget is kept
 *                iff (depth of its first sample) - (depth of the ray's first sample) < max_travel (strict; fp32 subtraction
 *                as in the tensor expression :91-92).  INFINITY disables it (plain OctreeAS.raymarch 'voxel' output).
 *   nugget_t     f32 [2][cap][N][2], nugget_cell i32 [2][cap][N]  caller-allocated scratch, cap = pag_raymarch_voxel_nugget_capacity(blas_level)
 *                (3 * 2^blas_level + 3: the most cells a ray can cross).  First half: the walk's candidates, [step][ray]; second half (ABI 11): the
 *                kept nuggets ray-major, [ray][slot] - what _pack_nuggets (which takes blas_level for `cap`) reads
 *   ridx_sample  optional i32 [M'*k]: the ray of every SAMPLE (the decoders' per-sample ray index); ridx64 optional
 *                i64 [M'] copy of ridx (wisp hands out int64 ray ids). */
int64_t pag_raymarch_voxel_nugget_capacity(int blas_level);
int pag_raymarch_voxel_count_nuggets(const float *origins, const float *dirs, int64_t N, int samples_per_voxel,
                                     float dist_min, float dist_max, const uint32_t *occupancy_bits, int blas_level,
                                     float max_travel, int32_t *counts, float *nugget_t, int32_t *nugget_cell, void *stream);
int pag_raymarch_voxel_pack_nuggets(const float *origins, const float *dirs, int64_t N, int samples_per_voxel,
                                    const int64_t *offsets, const float *nugget_t, const int32_t *nugget_cell, int blas_level,
                                    int32_t *ridx, int32_t *pidx, float *samples, float *depths, float *deltas,
                                    uint8_t *boundary, int32_t *ridx_sample, int64_t *ridx64, void *stream);

/* Occupancy update of pc_nerf/panoptic_delta_nef.py:63-104 (prune), one launch:
 *   occupancy[i] <- max(density[i * density_stride], occupancy[i] * decay)     (:74, :90)
 *   bit i of occupancy_bits <- occupancy[i] > min_density                      (:75, :98-104)
 * density f32 (one value per dense cell, x slowest), occupancy f32 [num_cells] (in/out),
 * occupancy_bits u32 [ceil(num_cells/32)] (out) - the bitfield pag_raymarch_* consume. */
int pag_occupancy_update(const float *density, int64_t density_stride, float *occupancy,
                         uint32_t *occupancy_bits, int64_t num_cells, float decay,
                         float min_density, void *stream);

/* Occupancy carving from depth images (csrc/carve.hip; the tensor-op definitions are carve_reference / carve_finish_reference of pagnerf_amd/carve.py).
 * Additive to ABI 15.  An addition of this package: the reference has no such step.
 * pag_carve_rays: ray i = (origins[i], dirs[i]) f32 [N,3] in the world frame, t_hit f32 [N] the measured surface distance ALONG the ray in scene
 *   units.  The ray is walked through the 2^blas_level lattice exactly as pag_raymarch_voxel_count_nuggets walks it (the same clip to
 *   [dist_min, dist_max], first cell, DDA and fp32 roundings: the same candidates (t_in, t_out, cell), t_out > t_in).  A ray is valid iff t_hit is
 *   finite and > 0; an invalid ray writes nothing.  With lo = t_hit - margin and hi = t_hit + margin (one fp32 rounding each) a candidate of a valid
 *   ray is SURFACE iff t_in <= hi && t_out >= lo, else FREE iff t_out <= lo, else untouched (it lies behind the surface).  The bit (x*R + y)*R + z of
 *   the cell is OR-ed into surface_bits / free_bits, u32 [max(1, R^3/32)] each, which the caller zeroes before the first call; calls accumulate.
 *   One launch; integer atomic ORs, issued only where the bit is still clear.  The result is a set: it does not depend on the order of the rays or
 *   on scheduling, so the same input gives the same bits.
 * pag_carve_finish: D = surface_bits dilated `dilate` times by the 26-neighbourhood (Chebyshev radius `dilate`, no wrap-around at the cube's faces);
 *   out_bits = ~free_bits | D (PAG_CARVE_HULL: a cell that no ray observed stays occupied) or D (PAG_CARVE_BAND: only the neighbourhood of measured
 *   surfaces is kept).  Bits past R^3 in the last word are 0.  One launch, no atomics.  out_bits must not alias the inputs.
 * Refused (PAG_ERR_ARG) before any launch: N < 0, NULL buffers (pag_carve_rays: with N > 0), blas_level outside [0, 10] (what
 * pag_raymarch_voxel_nugget_capacity's march accepts), a negative or NaN margin, dilate outside [0, PAG_CARVE_MAX_DILATE], an unknown mode.
 * N == 0 is a no-op. */
#define PAG_CARVE_MAX_DILATE 4
enum { PAG_CARVE_HULL = 0, PAG_CARVE_BAND = 1 };
int pag_carve_rays(const float *origins, const float *dirs, const float *t_hit, int64_t N, float dist_min, float dist_max, float margin,
                   int blas_level, uint32_t *free_bits, uint32_t *surface_bits, void *stream);
int pag_carve_finish(const uint32_t *free_bits, const uint32_t *surface_bits, int blas_level, int dilate, int mode, uint32_t *out_bits,
                     void *stream);

/* ------------------------------------------------------------------------------------------
 * Alpha compositing - kaolin spc_render.exponential_integration / sum_reduce as used at
 * tracers/panoptic_packed_rf_tracer.py:134-182,197-205
 * ------------------------------------------------------------------------------------------ */

/* Segmented exclusive scan + per-ray sums for the base channels.
 *   pack_start i64 [P+1] first packed sample of each non-empty ray (pack), ray_of_pack i32 [P]
 *   sigma f32 [M] (density, already ReLU'd), deltas f32 [M], depths f32 [M] or NULL,
 *   rgb f32 [M,3] or NULL
 *   weights f32 [M] (out): w_i = exp(-sum_{j<i} tau_j) (1 - exp(-tau_i)), tau = sigma*delta
 *   out_alpha f32 [N], out_rgb f32 [N,3], out_depth f32 [N], out_hit u8 [N]: rows of rays that
 *   have a pack are overwritten; the caller pre-fills the rest with the background.
 *   n_samples (ABI 9): 0, or the length of `weights` when the batch carries filler samples past pack_start[P]
 *   (pag_pad_packed): weights[pack_start[P] .. n_samples) is zeroed by the same launch. */
int pag_composite_fwd(const int64_t *pack_start, const int32_t *ray_of_pack, int64_t P,
                      const float *sigma, const float *deltas, const float *depths,
                      const float *rgb, int bg_color, float *weights, float *out_alpha,
                      float *out_rgb, float *out_depth, uint8_t *out_hit, int64_t n_samples, void *stream);

/* Gradients of pag_composite_fwd w.r.t. sigma and rgb.
 *   g_rgb f32 [N,3] / g_depth f32 [N] / g_alpha f32 [N]: upstream gradients (any may be NULL)
 *   d_sigma f32 [M], d_rgb f32 [M,3] (NULL allowed when rgb is NULL)
 *   n_samples (ABI 9): 0, or the length of d_sigma / d_rgb of a padded batch: the rows of the filler samples
 *   [pack_start[P], n_samples) are zeroed by the same launch (they carry no gradient). */
int pag_composite_bwd(const int64_t *pack_start, const int32_t *ray_of_pack, int64_t P,
                      const float *sigma, const float *deltas, const float *depths,
                      const float *rgb, int bg_color, const float *weights,
                      const float *out_alpha, const float *g_rgb, const float *g_depth,
                      const float *g_alpha, float *d_sigma, float *d_rgb, int64_t n_samples, void *stream);

/* Pose optimisation (pc_nerf/ba_pipeline.py:85-92): gradients of samples[m] = origins[ray] + dirs[ray] * depths[m] with respect to the rays -
 * out f32 [N,6], row r = (sum of grad_samples over ray r's pack | sum of grad_samples * depth); rows of rays without a pack are NOT written
 * (the caller zero-fills when packs do not cover every ray).  One pass over grad_samples f32 [M,3] and depths f32 [M].  (ABI 7) */
int pag_ray_sample_grad(const int64_t *pack_start, const int32_t *ray_of_pack, int64_t P, const float *grad_samples, const float *depths,
                        float *out, void *stream);

/* Per-ray weighted feature sums (tracer :197-205): out[ray, c] = alpha[ray] * sum_i w_i f[i, c].
 *   feats [M,C] row-major (feat_dtype F32 or BF16); out f32 [N,C] (rows of rays with a pack) */
int pag_composite_feats_fwd(const int64_t *pack_start, const int32_t *ray_of_pack, int64_t P,
                            const float *weights, const float *alpha, const void *feats,
                            int feat_dtype, int C, float *out, void *stream);
/* d feats[i, c] = alpha[ray] * w_i * g_out[ray, c]   (weights and alpha are detached, :148-155);
 * d_feats [M,C] in feat_dtype (F32 or BF16). */
int pag_composite_feats_bwd(const int64_t *pack_start, const int32_t *ray_of_pack, int64_t P,
                            const float *weights, const float *alpha, const float *g_out, int C,
                            void *d_feats, int feat_dtype, void *stream);

/* ------------------------------------------------------------------------------------------
 * Linear-assignment instance loss, device half (loss/lin_assignment_things.py:23-54,
 * loss/lin_assignment.py:16-26, utils/outlier_rejection.py:56-71)
 * ------------------------------------------------------------------------------------------ */

/* sums[k, c] = sum over rays p with labels_gt[p] == label_list[k] (and row_mask[p] != 0 when given)
 *              of values[p, col0 + c];   counts[k] = number of such rays.
 *   values [P, row_stride] (PAG_F32 or PAG_BF16), labels_gt i64 [P], row_mask u8 [P] or NULL,
 *   label_list i64 [K] (device), sums f32 [K, C], counts i32 [K].
 * fp32 accumulation in ray order (the order of a sequential sum over dim 0); the caller forms
 * cost = -(sums / (counts + 1e-4)) (:33) and runs the Hungarian solver on the host. */
int pag_label_sums(const void *values, int value_dtype, int64_t P, int64_t row_stride, int col0, int C,
                   const int64_t *labels_gt, const uint8_t *row_mask, const int64_t *label_list, int K,
                   float *sums, int32_t *counts, void *stream);

/* The same loss with ONE host synchronisation per step (ABI 10; loss/lin_assignment_things.py:23-82).
 *
 * All three take a BATCH of B images in one set of launches (the reference loops over the images of a step, :58): prob is
 * [B][P] rows of n_cols floats with element strides image_stride / row_stride, every other array is contiguous with the image as its
 * leading dimension (labels_gt [B,P], stuff_mask [B,P], info [B,2], labels / targets [B,max_rows], cost [B,max_rows,n_cols-col0],
 * sums_ws [B,max_rows,n_cols-col0], counts_ws [B,max_rows], virt / loss / valid / grad [B,P], wrong [B], d_prob [B,P,n_cols]).
 * Per image:
 * pag_assign_cost (three launches):
 *   labels i64 [max_rows]          the distinct positive gt ids of the image, ascending: `sorted(torch.unique(things_gt))[:max_rows]`
 *                                  (:29); entries past info[0] hold a sentinel no ray carries.  max_rows <= 1024.
 *   cost   f32 [max_rows, n_cols - col0]   row r = -(sum of prob[p, col0:] over the rays with gt == labels[r]) / (count + 1e-4)
 *                                  (:31-33: fp32 sums in ray order, int64 count + python float -> fp32, fp32 division); rows past info[0] untouched
 *   info   i32 [2]                 info[0] = number of labels, info[1] = 1 if the image carries more than 1024 distinct ids (take the
 *                                  general path: pag_label_sums with an explicit list)
 * so that ONE fixed-size device-to-host copy carries everything SciPy needs.  sums_ws f32 [max_rows, n_cols - col0] and counts_ws i32
 * [max_rows] are scratch.
 *
 *   points f32 [B,P,3] or NULL (outlier rejection, :38-43 + utils/outlier_rejection.py:8-51,56-71): the per-id centres of the same labels and
 *                                  id_lo_hi i32 [B,max_rows,2] = the id range [lo, hi] each may take (id_slope = (max_num_inst_at_x + id_margin) /
 *                                  frame_min_length and id_x_limit = (n_ids - id_margin) / id_slope as fp32, n_ids = n_cols - col0); every id outside
 *                                  costs 10000 - applied by the caller on the host.  psums_ws f32 [B,max_rows,3], pcounts_ws i32 [B,max_rows]: scratch.
 *
 * pag_assign_nll_fwd: per ray  valid = stuff_mask | gt > 0 (:60; stuff_mask u8 [P] or NULL),
 *   virt = gt > 0 ? (gt == labels[r] for some r < info[0] ? targets[r] : default_label) : 0   - targets i64 [max_rows] holds the assignment
 *   (:47-53: assigned column + 1; default_label = 1 for ids that got none), arg-max of the ray's n_cols probabilities,
 *   loss[ray] = -log(prob[ray, virt] + 1e-27) (:80) for valid rays when ANY valid ray of the image has virt != arg-max (:79), else 0;
 *   wrong i32 [1] (zeroed by the caller) receives that flag, virt / valid are kept for the backward.
 * pag_assign_nll_bwd: d_prob f32 [P, n_cols] (contiguous, every element written) from grad f32 [P]. */
int pag_assign_cost(const float *prob, int B, int64_t P, int64_t image_stride, int64_t row_stride, int n_cols, int col0,
                    const int64_t *labels_gt, int max_rows, float *sums_ws, int32_t *counts_ws, int32_t *info, int64_t *labels,
                    float *cost, const float *points, float id_slope, float id_x_limit, int id_margin, float *psums_ws,
                    int32_t *pcounts_ws, int32_t *id_lo_hi, void *stream);
/* The Hungarian step itself on the device (ABI 13): replaces `rows, cols = scipy.optimize.linear_sum_assignment(np.nan_to_num(cost))` of
 * loss/lin_assignment_things.py:45 (loss/lin_assignment.py:22) for the batch pag_assign_cost prepared - no device-to-host copy, no host wait, the train step
 * stays one uninterrupted stream of launches.  One wave per image runs SciPy's algorithm (rectangular_lsap.cpp: shortest augmenting paths, Crouse 2016) in
 * float64 in SciPy's operation order and tie rule, so the assigned columns are the same integers (oracle/lin_assign.py::lsap_jv is the sequential
 * restatement, pinned against the installed SciPy; tests/test_gpu_loss.py compares the kernel with SciPy itself on random, tie-heavy and masked matrices).
 *   cost f32 [B,max_rows,n_ids] (pag_assign_cost's output; rows >= info[b][0] are not read), widened to float64; id_lo_hi i32 [B,max_rows,2] or NULL: columns
 *   outside [lo, hi] of a row cost 10000 (utils/outlier_rejection.py:8-51); NaN -> 0, +-inf -> +-DBL_MAX (np.nan_to_num).
 *   targets i64 [B,max_rows]: assigned column + 1 for the rows < info[b][0], 1 elsewhere (:47-53) - what pag_assign_nll_fwd reads.
 *   status i32 [B]: 0 solved; 1 not attempted (info[b][1] set: more distinct ids than pag_assign_cost holds; targets all 1); 2 infeasible matrix (SciPy raises).
 * max_rows, n_ids <= 256. */
int pag_assign_solve(const float *cost, int B, int max_rows, int n_ids, const int32_t *info, const int32_t *id_lo_hi, int64_t *targets, int32_t *status,
                     void *stream);
int pag_assign_nll_fwd(const float *prob, int B, int64_t P, int64_t image_stride, int64_t row_stride, int n_cols,
                       const int64_t *labels_gt, const uint8_t *stuff_mask, const int64_t *labels, const int64_t *targets,
                       const int32_t *info, int max_rows, int64_t default_label, int64_t *virt, float *loss, uint8_t *valid,
                       int32_t *wrong, void *stream);
int pag_assign_nll_bwd(const float *prob, int B, int64_t P, int64_t image_stride, int64_t row_stride, int n_cols,
                       const int64_t *virt, const uint8_t *valid, const int32_t *wrong, const float *grad, float *d_prob,
                       void *stream);

/* segment_consistency_regularizer (ABI 12; loss/regularizers.py:5-35, called at pc_nerf/trainer.py:525-527 on `inst_embedding + 1e-27`) over a batch of B images
 * without a host synchronisation.  prob f32: [B][P] rows of n_cols probabilities (element strides image_stride / row_stride), eps is added to every
 * probability read (the caller's `+ 1e-27`), labels i64 [B,P] contiguous.  Per image every distinct value of labels is a segment (at most 2048 per image and
 * never INT64_MIN - otherwise out is NaN and the gradient 0); per segment: histogram of its rays' first arg-max column (:22), skipped when every ray predicts
 * column 0 (:24-25), label = first most frequent column among 1.. (:27) or 0 when bins[0] * 0.5 > bins[label] (:29-30), term = mean over its rays of
 * -log(prob[ray, label] + eps) (:32); the running total is divided by each image's segment count in turn (:33) and finally by B (:35) -> out f32 [1].
 * workspace (pag_segment_reg_workspace_bytes(B, P) bytes) keeps what the backward needs; pag_segment_reg_bwd writes EVERY element of d_prob f32 [B,P,n_cols]
 * (contiguous) from grad f32 [1].  Sums are lane-strided with a fixed butterfly: bitwise reproducible. */
int64_t pag_segment_reg_workspace_bytes(int B, int64_t P);
int pag_segment_reg_fwd(const float *prob, int B, int64_t P, int64_t image_stride, int64_t row_stride, int n_cols, float eps,
                        const int64_t *labels, void *workspace, int64_t workspace_bytes, float *out, void *stream);
int pag_segment_reg_bwd(const float *prob, int B, int64_t P, int64_t image_stride, int64_t row_stride, int n_cols, float eps,
                        const void *workspace, int64_t workspace_bytes, const float *grad, float *d_prob, void *stream);

/* ------------------------------------------------------------------------------------------
 * Supervised-contrastive instance loss (loss/sup_contrastive.py::SupConLoss as pc_nerf/trainer.py:499-503 and :477-480 call it) - three launches
 * forward, two backward, no [n, n] matrix in memory, no host synchronisation.  Additive to ABI 14.
 * ------------------------------------------------------------------------------------------ */

/* Per image b of features [B, P, D] (f32 or bf16 `dtype`, element (b, p, k) at b*image_stride + p*row_stride + k) and labels i64 [B,P] (contiguous):
 * the anchors S are the rows with anchor_mask u8 [B,P] != 0, in row order (anchor_mask NULL: every row).  f = x / max(||x||, 1e-12);
 * A_ij = f_i.f_j / temperature for i, j in S; m_i = max_j A_ij (j = i included, treated as a constant); LSE_i = log Sum_{j != i} exp(A_ij - m_i);
 * M_ij = [label_i == label_j][j != i], cnt_i = Sum_j M_ij;
 * loss_i = -(temperature / base_temperature) * (Sum_j M_ij (pos_weight (A_ij - m_i) - neg_weight LSE_i)) / (cnt_i + 1e-16).
 * An image with anchor_mask given whose anchor set is empty or holds a single label value is skipped.  loss f32 [B,P] (contiguous) gets loss_i at each
 * anchor's row and 0 at every other row and in skipped images.  The workspace (pag_supcon_workspace_bytes(B, P, D) bytes) keeps the normalised anchors
 * and the row statistics for pag_supcon_bwd, which writes EVERY element of d_features [B,P,D] (contiguous, `dtype`) from grad_loss f32 [B,P]
 * (contiguous): zero rows for non-anchors and skipped images.  1 <= D <= 512, P <= 2^24; sums run in a fixed order (bitwise reproducible). */
int64_t pag_supcon_workspace_bytes(int B, int64_t P, int D);
int pag_supcon_fwd(const void *features, int dtype, int B, int64_t P, int D, int64_t image_stride, int64_t row_stride, const int64_t *labels,
                   const uint8_t *anchor_mask, float temperature, float base_temperature, float pos_weight, float neg_weight, void *workspace,
                   int64_t workspace_bytes, float *loss, void *stream);
int pag_supcon_bwd(int dtype, int B, int64_t P, int D, float temperature, float base_temperature, float pos_weight, float neg_weight, void *workspace,
                   int64_t workspace_bytes, const float *grad_loss, void *d_features, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mean-shift clustering of the instance embedding (utils/clustering/mean_shift.py::MeanShift with utils/embedding.py::mean_class_embedding and sklearn's
 * estimate_bandwidth / MeanShift / predict; pc_nerf/clustering_nef.py, called at pc_nerf/trainer.py:948-970 and :737-738) - every pass on the device,
 * no K x K matrix in memory, no float atomics, bitwise reproducible.  Additive to ABI 14.
 * ------------------------------------------------------------------------------------------ */

/* Workspace of pag_meanshift_fit for B*P rows of D dimensions (0 for sizes past the limits: B*P <= 2^24, 1 <= D <= 512); O(B*P + K*D) bytes. */
int64_t pag_meanshift_workspace_bytes(int B, int64_t P, int D);

/* features [B, P, D] (f32 or bf16 `dtype`, element (b, p, k) at b*image_stride + p*row_stride + k), labels i64 [B,P] contiguous.
 * Stage 1 (utils/embedding.py:3-27, mean_class_embedding): one class mean per (image, distinct label), images in order and labels ascending within an
 *   image, negative labels included; each is the fp32 sum of its rows divided by the count -> means f32 [Kcap, D] rows 0 .. K-1, Kcap = min(B*P, 32768).
 *   labels NULL: every row is its own class (K = B*P <= 32768; the rows are copied), which is how the centres of estimate_bandwidth are passed in.
 * Stage 2 (mean_shift.py:22, sklearn estimate_bandwidth(centres, quantile)): k = max(1, int(K quantile)); per centre the exact k-th smallest Euclidean
 *   distance to all centres (itself included, at 0), from the fp32 values with fp64 accumulation; bandwidth f64 [1] = their mean.  For K < 1/quantile
 *   k = 1 and the bandwidth is exactly 0, and stage 3 makes every distinct centre its own cluster.  This differs from the reference there: sklearn's
 *   ~1e-9 bandwidth is at the size of its rounding of a centre's distance to itself, so it drops some seeds, and for a bandwidth of exactly 0 (K = 1,
 *   identical centres) its MeanShift raises instead of fitting.
 * Stage 3 (mean_shift.py:24, sklearn MeanShift(bandwidth, bin_seeding=False, cluster_all=True, max_iter).fit): every centre seeds
 *   m <- mean of the centres with ||c - m|| <= bw, summed in ascending index order in fp64 and rounded to fp32, until ||m_new - m_old|| <= 1e-3 bw or
 *   max_iter iterations; intensity = the neighbour count of the last iteration (a seed whose neighbourhood empties is dropped).  Equal converged means
 *   are one entry (sklearn's dict) with the last such seed's intensity; the entries are ordered by (intensity, coordinates lexicographically)
 *   descending and each kept entry removes every later one within bw -> centers f32 [Kcap, D] rows 0 .. C-1 = cluster_centers_.
 * info i32 [4] = {K, C, n_iter (the largest completed-iteration count of any seed), flags}; flags bit 0: K > 32768 (the fit stops after counting; K
 * then reads 32769).  Nothing is read back to the host: the caller reads info once at the end.  stages 1, 2, 3 run the passes up to that stage. */
int pag_meanshift_fit(const void *features, int dtype, int B, int64_t P, int D, int64_t image_stride, int64_t row_stride, const int64_t *labels,
                      double quantile, int max_iter, int stages, void *workspace, int64_t workspace_bytes, float *means, double *bandwidth,
                      float *centers, int32_t *info, void *stream);

/* mean_shift.py:34-42 (sklearn MeanShift.predict = pairwise_distances_argmin): labels_out i64 [N] = argmin_c ||x_n - c|| over centers f32 [C, D]
 * (contiguous), exact ties to the lowest index.  x: N rows (f32 or bf16 `dtype`) of D elements, row n at n*row_stride.  Scores ||c||^2 - 2 x.c on the
 * f32-input MFMA; a row whose two best scores are closer than the bound of their rounding error is recomputed in fp64, so the result equals the fp64
 * argmin.  1 <= D <= 512, 1 <= C <= 32768, any N (0: no-op); no host synchronisation (capturable in a graph). */
int pag_meanshift_predict(const void *x, int dtype, int64_t N, int D, int64_t row_stride, const float *centers, int C, int64_t *labels_out,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Panoptic evaluation of a validation image (pc_nerf/trainer.py:651-941 evaluate_metrics): the instance cleanup of :750-772, the panoptic quality
 * update of utils/metrics/panoptic_quality{,_func}.py and the confusion matrix of the semantic IoU (:670-671, :720).  Every pass on the device, no
 * [K, H, W] masks, no float atomics, integer sums only (bitwise reproducible), no host synchronisation (capturable in a graph).  Additive to ABI 14.
 * ------------------------------------------------------------------------------------------ */
enum { PAG_I32 = 3, PAG_I64 = 4 };          /* id / label dtypes of the panoptic evaluation */

/* Workspace of pag_panoptic_pq_update (0 past the limits: B*H*W <= 2^28, 2 <= n_cat <= 1024); O(B*H*W) bytes. */
int64_t pag_panoptic_pq_workspace_bytes(int B, int64_t H, int64_t W, int n_cat);

/* One PanopticQuality.update(preds, target): both [B, 2, H, W] (int32 / int64 `*_dtype`, element (b, c, y, x) at the dot product with the host arrays
 * `*_strides` [4]); never written.  cat_ids i64 [n_cat] (device) = things and stuff ids in ascending order, cat_cont i32 [n_cat] (device) = their
 * continuous ids (things in set iteration order first: 0 .. n_things-1, then stuff).
 * Preprocessing (_prepocess_image): instance ids of image b get the cumulative offset sum_{b' < b} max(raw instance channel of b'); stuff pixels get
 *   instance 0; categories outside cat_ids become the void colour.  Segments are the distinct (category, instance) colours.
 * Matching (_panoptic_quality_update): a (pred, target) pair with a non-void target of the same category matches when the f32 quotient of the int64
 *   intersection and union = pred_area - pred_void_area + target_area - void_target_area - intersection is > 0.5; every such pair adds 1 to tp and
 *   its IoU to iou_sum.  An unmatched non-void target (pred) segment adds 1 to fn (fp) unless its void area over its area (f32) is > 0.5.
 * The call's sums are added to the state iou_sum f64 [n_cat], true_positives / false_positives / false_negatives i32 [n_cat] (device).  The IoUs of
 * a call are exact multiples of 2^-24 in (0.5, 1] and summed exactly as integers, so iou_sum equals the reference's f64 sum in any order.
 * The first 4 bytes of the workspace receive this call's flags: bit 0 an unknown pred category (then, with allow_unknown == 0, the state is left
 * unchanged and the caller raises); bit 1 a thing instance id outside int32 after the offsets, which is also OR-ed into state_flags i32 [1]. */
int pag_panoptic_pq_update(const void *preds, int preds_dtype, const int64_t *preds_strides, const void *target, int target_dtype,
                           const int64_t *target_strides, int B, int64_t H, int64_t W, const int64_t *cat_ids, const int32_t *cat_cont, int n_cat,
                           int n_things, int allow_unknown, void *workspace, int64_t workspace_bytes, double *iou_sum, int32_t *true_positives,
                           int32_t *false_positives, int32_t *false_negatives, int32_t *state_flags, void *stream);

/* Workspace of pag_panoptic_clean (0 past the limits: H, W <= 32768, H*W <= 2^28); O(H*W) bytes. */
int64_t pag_panoptic_clean_workspace_bytes(int64_t H, int64_t W);

/* trainer.py:750-772 on an id image [H, W] (int32 / int64 `dtype`, element (y, x) at y*stride_y + x*stride_x; never written) -> out [H, W]
 * (contiguous, same dtype).  The background is the smallest id.  Every other id's mask gets a flat 3x3 opening when num_openings > 0 (opening is
 * idempotent; erosion counts pixels outside the image as inside, dilation as outside), then with outlier_rejection its pixels farther from the
 * mask's centre of mass than mean + std_threshold * std of the mask's distances (population std) are dropped, then masks of fewer than min_area
 * pixels are dropped.  Dropped pixels get the background id.  Moments are exact integers, distances fp64, their sums 2^-20 fixed point. */
int pag_panoptic_clean(const void *ids, int dtype, int64_t H, int64_t W, int64_t stride_y, int64_t stride_x, int num_openings, int outlier_rejection,
                       int64_t min_area, double std_threshold, void *workspace, int64_t workspace_bytes, void *out, void *stream);

/* confmat i64 [C, C] (device, contiguous) += counts of (target, pred) over shape[4] elements (host array; element (i0..i3) of preds at the dot
 * product with preds_strides [4], likewise target); pairs with a value outside [0, C) are ignored.  1 <= C <= 65536. */
int pag_confusion_matrix(const void *preds, int preds_dtype, const int64_t *preds_strides, const void *target, int target_dtype,
                         const int64_t *target_strides, const int64_t *shape, int C, int64_t *confmat, void *stream);

/* Workspace of pag_mask_ap_update (0 past the limits: 1 <= H*W <= 2^28, 1 <= max_detections <= 4096): two 8192-slot id tables and a dense
 * [max_detections, 4096] count array, whatever the image size - nothing of it grows with ids * H * W. */
int64_t pag_mask_ap_workspace_bytes(int64_t H, int64_t W, int max_detections);

/* One image of the mask mAP of pc_nerf/trainer.py:674-675, :794-798, :839-843 (MeanAveragePrecision(iou_type="segm") with one class and every score
 * 1.0), from label images instead of [K, H, W] mask stacks.  pred, pred_raw, target: [H, W] id images (int32 / int64 `*_dtype`, element (y, x) at
 * y*stride_y + x*stride_x; never written).
 * Detections: the distinct ids of pred_raw in ascending order without the smallest (mask_ids[1:], :753-755), the first max_detections of them; the
 *   mask of one is the pixels of pred with its id (possibly none: :766-767 keeps zeroed masks).  With empty_detection_if_single_id, a pred_raw of
 *   one distinct id gives one empty detection (:780-781).  Ground truths: the distinct ids of target without the smallest (gt_ids[1:], :791-792).
 * IoU = double(i) / double(a_d + a_g - i) of the exact integer counts when i > 0, else 0.  Matching, per threshold of the host array thresholds
 *   f64 [10] (passed to the launch by value), detections in order: the not yet matched ground truth of the largest IoU >= min(t, 1 - 1e-10), the
 *   later one on a tie (COCOeval's greedy rule).
 * slots i32 [max_detections] (device) receives one word per detection - bit 0 present, bit 1 + k matched at threshold k - and 0 in the slots past
 * the last detection; *npig i64 (device) += the number of ground truths.  More than 4096 distinct ids in pred_raw or in target, the id INT64_MIN,
 * or an id of pred that pred_raw lacks: the bit (1, 1, 2) is OR-ed into *state_flags i32 (device) and slots and npig are left untouched.
 * Six launches, no host synchronisation, integer sums only (bitwise reproducible), every probe and id loop bounded by the table capacity. */
int pag_mask_ap_update(const void *pred, int pred_dtype, int64_t pred_stride_y, int64_t pred_stride_x, const void *pred_raw, int raw_dtype,
                       int64_t raw_stride_y, int64_t raw_stride_x, const void *target, int target_dtype, int64_t target_stride_y,
                       int64_t target_stride_x, int64_t H, int64_t W, int max_detections, int empty_detection_if_single_id,
                       const double *thresholds, void *workspace, int64_t workspace_bytes, int32_t *slots, int64_t *npig, int32_t *state_flags,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * Panoptic point-cloud map export (utils/render_map.py; main_interactive.py:109-129 `--save-map-only`): the reduction of rendered rays / dense lattice
 * rows to the kept map points as an ORDERED APPEND behind a running device counter.  Kept rows land in row order behind *count (i64 [1], device),
 * which the call advances by the number kept; a row whose slot is at or past `cap` is counted and not written, so an overflow shows in the counter
 * and nothing is written out of bounds.  Output order and bits do not depend on how the rows are split over calls.  Three launches (four with the
 * `argmax != 0` predicate), no host synchronisation, no float atomics, capturable in a graph.  n = 0 is a no-op; n <= 2^31.  Additive to ABI 14.
 * Instance ids are torch.argmax's over inst f32 [n, I] (row i at i*inst_stride elements, 1 <= I <= 1024): the first index of the maximum, a NaN
 * counting as the maximum; or they are copied from ids_in i64 [n] (give one of the two).
 * ------------------------------------------------------------------------------------------ */

/* Workspace of one call over n rows (0 for n outside (0, 2^31]); about 4 n bytes. */
int64_t pag_map_workspace_bytes(int64_t n);

/* render_points_at_depth :107-120 on one rendered chunk of n rays, global ray index ray0 + i: depth, alpha, density f32 [n] (the [n,1] buffers),
 * hit u8 / bool [n], rgb f32 [n,3].  Kept iff density > min_density && alpha > min_alpha && hit && depth < depth_max && depth > depth_min (all
 * strict).  point = sum_k (o_c - t + d_c depth)[k] R[k] (the arithmetic and op order of pag_pose_points; utils/outlier_rejection.py:89-97) with
 * the camera cam[(ray0 + i) / rays_per_camera] (cam i32 [n_cam], rows of params f32 [C,9], clamped as in pag_pose_rays_fwd) and the camera-frame
 * base ray (ray0 + i) % rays_per_camera of origins_c / dirs_c f32 [rays_per_camera,3] (the reference stacks the same base rays once per camera,
 * :98).  -> points f32 [cap,3], color f32 [cap,3] (the rgb bits), ids_out i64 [cap]. */
int pag_map_points(const float *params, int64_t C, const int32_t *cam, int64_t n_cam, int64_t rays_per_camera, const float *origins_c,
                   const float *dirs_c, int64_t ray0, int64_t n, const float *depth, const float *alpha, const uint8_t *hit,
                   const float *density, const float *rgb, const float *inst, int I, int64_t inst_stride, const int64_t *ids_in,
                   float min_density, float min_alpha, float depth_min, float depth_max, float *points, float *color, int64_t *ids_out,
                   int64_t cap, int64_t *count, void *workspace, int64_t workspace_bytes, void *stream);

/* get_dense_occupied_points :77-79 / generate_pc_map :160-165: rows of points_in f32 [n,3] kept iff value[i] > threshold (value f32 [n], strict)
 * or, with value NULL, iff their instance id != 0.  -> points f32 [cap,3] and, with ids_out i64 [cap] not NULL and ids given, the kept rows' ids. */
int pag_map_select(const float *points_in, int64_t n, const float *value, float threshold, const float *inst, int I, int64_t inst_stride,
                   const int64_t *ids_in, float *points, int64_t *ids_out, int64_t cap, int64_t *count, void *workspace,
                   int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Panoptic surface-mesh export: surface nets on the density lattice (csrc/mesh.hip; beyond the reference, which exports points only).  Additive to
 * ABI 14.  field f32 [nx, ny, nz] (z fastest, device): a lattice point is INSIDE when v >= iso (a NaN is outside), a cell (i, j, k) with the corners
 * (i + bx, j + by, k + bz) ACTIVE when its 8 corners are finite and neither all inside nor all outside.  Every active cell owns one vertex, every
 * lattice edge whose ends differ in `inside` and whose four cells own a vertex one quad.  Both calls are ordered appends with the contract of the
 * map export above: kept rows land in row order behind *count (i64 [1], device), a slot at or past the capacity is counted and not written, three
 * launches, no host synchronisation, no atomics; the order of vertices and faces does not depend on the launch geometry.  Every axis needs 2 points;
 * fewer than 2^31 cells (vertex ids are i32) and fewer than 2^32 / 3 points (one thread per edge row).
 * ------------------------------------------------------------------------------------------ */

/* Workspace of either call on an nx x ny x nz lattice (0 for a lattice the calls refuse); about points / 21 bytes. */
int64_t pag_mesh_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);

/* A row is a cell in linear order (x slowest).  The vertex of an active cell, all in fp32 and in this order: over the 12 cell edges taken axis-major
 * (axis a = 0, 1, 2; the two other axes in increasing order with bits (bu, bv) = 00, 01, 10, 11, the lower axis's bit slower; the edge runs from
 * corner A with bit 0 on axis a to corner B with bit 1) every edge whose ends differ in `inside` adds the point p = A's bits with
 * p[a] = (iso - vA) / (vB - vA) to S and 1 to n;  local = S / n;  vertex = ((float)(index0 + cell index) + local) * h + lo per axis (two roundings after
 * the add).  Normal: g[a] = the chain sum of (vB - vA) over the axis's four edges, m = sqrt((g0 g0 + g1 g1) + g2 g2), normal = -g / m, 0 when
 * m == 0 (towards falling density).  lo_host f32 [3], index0_host i32 [3] (the global index of field[0,0,0], >= 0) are host arrays.
 * -> vertices, normals f32 [cap, 3]; cell_vertex i32 [(nx-1)(ny-1)(nz-1)] receives EVERY cell's slot (the vertex id when *count was 0), -1 for a
 * cell without vertex, also for slots at or past cap. */
int pag_mesh_vertices(const float *field, int64_t nx, int64_t ny, int64_t nz, float iso, const float *lo_host, float h, const int32_t *index0_host,
                      float *vertices, float *normals, int64_t cap, int32_t *cell_vertex, int64_t *count, void *workspace, int64_t workspace_bytes,
                      void *stream);

/* A row is r = ((i ny + j) nz + k) 3 + a: the lattice edge from P = (i, j, k) to P + e_a (no edge when P[a] + 1 leaves the lattice).  It gives a quad
 * when its ends differ in `inside` and the four cells at P with the offsets (du, dv) = (-1,-1), (0,-1), (0,0), (-1,0) on the axes u = (a + 1) % 3,
 * v = (a + 2) % 3 exist and have a vertex in cell_vertex (as pag_mesh_vertices wrote it): q0..q3, reversed when P is outside.  The s-th kept row
 * writes the triangles (q0, q1, q2), (q0, q2, q3) to rows 2s, 2s + 1 of faces i32 [cap, 3]; *count counts QUADS, and a quad whose two rows do not
 * both fit below cap is counted and not written.  Face normals point from inside to outside. */
int pag_mesh_faces(const float *field, int64_t nx, int64_t ny, int64_t nz, float iso, const int32_t *cell_vertex, int32_t *faces, int64_t cap,
                   int64_t *count, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused panoptic voxel map: the exported points of all views reduced to one row per occupied voxel, and the per-instance table of that map
 * (csrc/voxelmap.hip).  Additive to ABI 14.  The two reductions are ordered appends behind a device counter with the contract of the map export
 * above: kept runs land in row order behind *count (i64 [1], device), a slot at or past `cap` is counted and not written, three launches, no host
 * synchronisation, no float atomics.  Every sum is taken in an order fixed by the sorted row sequence and a compile-time group width (16 lanes per
 * voxel run, 256 threads per label run), so the results are bit-identical from run to run and however the points were chunked before the sort.
 * n = 0 is a no-op; n <= 2^31.
 * ------------------------------------------------------------------------------------------ */

/* Workspace of one fuse / table call over n rows (0 for n outside (0, 2^31]); about n / 21 bytes. */
int64_t pag_voxel_workspace_bytes(int64_t n);

/* points f32 [n,3] -> keys i64 [n]: per axis i = floorf((p - origin) / voxel_size), both roundings in fp32 and in that order, a true division;
 * key = iz | iy << 21 | ix << 42 (x slowest).  INT64_MAX when a coordinate is not finite, an index is < 0 or >= 2^21, or - limits_host f32 [2,3]
 * = [[min], [max]] given - the point is not strictly inside the box.  origin_host f32 [3] and limits_host are host arrays.  One launch. */
int pag_voxel_keys(const float *points, int64_t n, const float *origin_host, float voxel_size, const float *limits_host, int64_t *keys,
                   void *stream);

/* Rows ordered by (key, id): keys i64 [n] ascending (the INT64_MAX rows last), ids i64 [n] ascending inside a run of equal keys, points f32 [n,3]
 * and color f32 [n,3] (or NULL) permuted alike.  Every run of equal keys with at least min_votes (>= 1) rows gives one output row, in key order:
 * points / color f32 [cap,3] the mean of the members (fp32 sum / (float) rows), ids_out i64 [cap] the most frequent id of the run (on equal counts
 * the smaller id, signed), count_out i32 [cap] the rows, agreement f32 [cap] = (float) winner's rows / (float) rows, voxels i32 [cap,3] = (ix, iy, iz). */
int pag_voxel_fuse(const int64_t *keys, const int64_t *ids, const float *points, const float *color, int64_t n, int64_t min_votes,
                   float *points_out, float *color_out, int64_t *ids_out, int32_t *count_out, float *agreement, int32_t *voxels,
                   int64_t cap, int64_t *count, void *workspace, int64_t workspace_bytes, void *stream);

/* Voxel rows ordered by label (labels i64 [n] ascending; points f32 [n,3], color f32 [n,3] or NULL, voxel_count i32 [n] permuted alike).  Every run
 * of a label that is not one of the n_ignore (<= 8) labels of ignore_host (host array) gives one row, in label order: ids_out i64 [cap], voxels_out
 * i64 [cap] the rows, observations i64 [cap] the sum of voxel_count, centroid f32 [cap,3] the mean of the points, bbox_min / bbox_max f32 [cap,3],
 * color_out f32 [cap,3] the mean colour (untouched without color). */
int pag_label_table(const int64_t *labels, const float *points, const float *color, const int32_t *voxel_count, int64_t n,
                    const int64_t *ignore_host, int n_ignore, int64_t *ids_out, int64_t *voxels_out, int64_t *observations,
                    float *centroid, float *bbox_min, float *bbox_max, float *color_out, int64_t cap, int64_t *count, void *workspace,
                    int64_t workspace_bytes, void *stream);

/* Connected components of a fused map (additive to ABI 14; pagnerf_amd.map_export.connected_components_reference is the definition).
 *   voxels i32 [n,3] = (ix, iy, iz), rows STRICTLY ascending by key iz | iy << 21 | ix << 42 (what pag_voxel_fuse writes); ids i64 [n]
 *   connectivity 6 / 18 / 26: rows are linked when their indices differ by an offset with at most 1 / 2 / 3 non-zero components, each -1 or +1; an
 *   index outside [0, 2^21) does not exist (nothing is borrowed across an axis of the key).  same_id != 0: linked rows must also carry equal ids.
 *   Rows whose id is one of the n_ignore (<= 8) ids of ignore_host (host array) link nothing and get component 0.
 *   component i64 [n]: 1 .. C, the components numbered by their first row; count i64 [1] = C; status i32 [1]: 0, or bit 0 a row's key is not greater
 *   than the row's before, bit 1 an index outside [0, 2^21), bit 2 a loop cap of n + 1 rounds exceeded (the result is then undefined, nothing is
 *   accessed out of range).  count and status are device words, OVERWRITTEN.
 * A lock-free union-find over int32 parent[n] (the larger root is hooked under the smaller with a compare-and-swap: a component's root is its first
 * row in any interleaving, so the same input gives the same output), then the ordered append above over the root rows.  Seven launches and two
 * memsets, no host synchronisation, no thread waits on another.  workspace: pag_voxel_components_workspace_bytes(n) bytes (16 n and the append's
 * tables; 0 for n outside (0, 2^31)).  n = 0 is a no-op; n < 2^31. */
int64_t pag_voxel_components_workspace_bytes(int64_t n);
int pag_voxel_components(const int32_t *voxels, const int64_t *ids, int64_t n, int connectivity, int same_id, const int64_t *ignore_host,
                         int n_ignore, void *workspace, int64_t workspace_bytes, int64_t *component, int64_t *count, int32_t *status, void *stream);

/* Two fused maps on one lattice: the shared voxels per pair of ids, the IoU / cost of the id association, and the merged map (additive to ABI 14;
 * pagnerf_amd.map_export.overlap_table_reference / associate_maps_reference / merge_maps_reference are the definitions).  Each map: voxels i32
 * [n,3] with rows STRICTLY ascending by key as above, ids i64 [n], uniq i64 [T] the map's distinct ids ascending (signed).
 *
 * pag_voxel_overlap: keys i64 [n] (-1: an index outside [0, 2^21)) and slot i32 [n] (the position of the row's id in uniq; -1: not in it) of both
 *   maps, and table i32 [Ta,Tb] (ZEROED BY THE CALLER): table[slot_a, slot_b] += 1 for every key both maps hold (a lower-bound search per row of a
 *   in b's keys).  Integer atomics, combined per wave before they leave it when combine != 0 (equal results either way).  status i32 [1], OVERWRITTEN: bits 0 / 1 as in pag_voxel_components (either map), bit 3 an id
 *   that is missing from its list.  A map that breaks the contract is read as data: nothing is accessed out of range.  One memset, three launches,
 *   no host synchronisation, no thread waits on another.  na + nb < 2^31, Ta * Tb < 2^31; an empty map is allowed (T = 0, NULL columns).
 * pag_overlap_cost: iou f32 [Ta,Tb] = (float) t / (float) (row_sum[i] + col_sum[j] - t), 0 where that denominator is 0 (row_sum i64 [Ta], col_sum
 *   i64 [Tb]: the table's sums); cost f32 [R,C] = 1.0f - iou over the active ids act_a i32 [n_a] / act_b i32 [n_b] (positions in uniq), oriented
 *   for pag_assign_solve: R = min(n_a, n_b) rows, the rows being b's ids when n_a > n_b.  No contraction; one launch.
 * pag_voxel_merge: keys i64 [na + nb] = both maps' keys sorted stably (a's rows first) and order i64 [na + nb] = that sort's permutation.  Every
 *   run of equal keys gives one row in key order behind *count (i64 [1], device, zeroed by the caller; a slot at or past cap is counted and not
 *   written).  b's id is mapping[slot_b] (mapping i64 [Tb]).  A run of one row is copied bit for bit.  A run of a's row and b's row: count = cA + cB
 *   (saturating), points / color = (pA * (float) cA + pB * (float) cB) / (float) count in that order without contraction, votes v = rintf(agreement *
 *   (float) c); equal ids: that id with vA + vB votes, else the id with more votes (ties: the smaller id) and its own votes; agreement = (float) votes
 *   / (float) count.  color_out NULL: no colour.  status i32 [1] is ORed into: bit 4 a run of three or more rows, or of two rows of one map (its first
 *   row is copied).  workspace: pag_voxel_workspace_bytes(na + nb).  Three launches, no host synchronisation. */
int pag_voxel_overlap(const int32_t *voxels_a, const int64_t *ids_a, int64_t na, const int64_t *uniq_a, int Ta, const int32_t *voxels_b,
                      const int64_t *ids_b, int64_t nb, const int64_t *uniq_b, int Tb, int combine, int64_t *keys_a, int32_t *slot_a, int64_t *keys_b,
                      int32_t *slot_b, int32_t *table, int32_t *status, void *stream);
int pag_overlap_cost(const int32_t *table, const int64_t *row_sum, const int64_t *col_sum, int Ta, int Tb, const int32_t *act_a, int n_a,
                     const int32_t *act_b, int n_b, float *iou, float *cost, void *stream);
int pag_voxel_merge(const int64_t *keys, const int64_t *order, int64_t na, int64_t nb, const float *points_a, const float *color_a,
                    const int64_t *ids_a, const int32_t *count_a, const float *agreement_a, const int32_t *voxels_a, const float *points_b,
                    const float *color_b, const int32_t *slot_b, const int64_t *mapping, int Tb, const int32_t *count_b, const float *agreement_b,
                    const int32_t *voxels_b, float *points_out, float *color_out, int64_t *ids_out, int32_t *count_out, float *agreement_out,
                    int32_t *voxels_out, int64_t cap, int64_t *count, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Per-ray training loss of the rendered buffers (pc_nerf/trainer.py:443-446 rgb, :459-465 semantics,
 * loss/lin_assignment_things.py:80 instance term after the assignment) - one launch forward, one backward
 * ------------------------------------------------------------------------------------------ */

/* loss = rgb_weight * mean|rgb - rgb_gt|
 *      + sum over the (up to two) NLL terms t of  weight_t * sum_n l_tn / denom_t,
 *        l_tn = -log(prob_t[n, target_t[n]] + eps) * inv_temp_t * (conf_t[n] if conf_t else 1)
 *        for rows with 0 <= target < C_t (others - F.nll_loss's ignore_index included - contribute nothing);
 *        denom_t = N if all_t (reduction 'none' then .mean(), trainer.py:459-465) else the number of valid rows
 *        (F.nll_loss reduction 'mean').
 *   rgb, rgb_gt f32 [N,3] (both NULL: no rgb term); prob_t f32 [N, C_t] contiguous (NULL: term absent);
 *   target_t i64 [N]; conf_t f32 [N] or NULL.
 *   workspace: pag_render_loss_workspace_bytes() bytes, ZEROED ONCE by the caller and then reused as is.
 *   out f32 [6]: total, rgb term, term A, term B, denom A, denom B.
 * Deterministic (fixed-order block partials, the last block adds them in block order). */
int64_t pag_render_loss_workspace_bytes(void);
int pag_render_loss_fwd(const float *rgb, const float *rgb_gt, int64_t N, float rgb_weight,
                        const float *prob_a, int C_a, const int64_t *target_a, const float *conf_a, float weight_a,
                        float inv_temp_a, int all_a,
                        const float *prob_b, int C_b, const int64_t *target_b, const float *conf_b, float weight_b,
                        float inv_temp_b, int all_b,
                        float eps, void *workspace, float *out, void *stream);

/* Gradients of the above times the upstream scalar *g (device pointer; NULL = 1): d_rgb [N,3] = g rgb_weight sgn(rgb-gt)/(3N),
 * d_t [N, C_t] dense: -g weight_t inv_temp_t conf / (denom_t (p + eps)) in the target column of valid rows, 0 elsewhere
 * (every element is written).  fwd_out = the forward's `out`.  Any of d_rgb / d_a / d_b may be NULL. */
int pag_render_loss_bwd(const float *g, const float *fwd_out, const float *rgb, const float *rgb_gt, int64_t N,
                        float rgb_weight,
                        const float *prob_a, int C_a, const int64_t *target_a, const float *conf_a, float weight_a,
                        float inv_temp_a, int all_a,
                        const float *prob_b, int C_b, const int64_t *target_b, const float *conf_b, float weight_b,
                        float inv_temp_b, int all_b,
                        float eps, float *d_rgb, float *d_a, float *d_b, void *stream);

/* ---- optimiser step of the train step's caller (round 4, ABI 9) ------------------------------------------------------------------
 * torch.optim.Adam(params, lr, betas, eps, weight_decay) as the reference builds it (config_parser.py:667-673: eps = 1e-15;
 * pc_nerf/trainer.py:268-286 parameter groups; :583 scaler.step(optimizer)) for fp32 tensors, op for op the single-tensor formula
 * of torch/optim/adam.py (maximize / amsgrad off):  g += weight_decay p ; m += (g - m)(1 - beta1) ; v = v beta2 + (1 - beta2) g g ;
 * p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps).   `step` = the step count AFTER this update (>= 1).
 * n_tensors host arrays of device pointers (f32, contiguous, numel[i] elements each); ONE launch per 48 tensors (704 MB per step
 * for the two 50.3 MB tables: the update is a pure stream; a tensor gets one block per 4096 elements, at most 4096). */
int pag_adam_step(int n_tensors, float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                  const int64_t *numel, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                  void *stream);

/* ---- pose optimisation: the per-ray camera transform (round 5, ABI 11) -------------------------------------------------------------
 * pc_nerf/ba_pipeline.py:85-92 `transform_rays` (kaolin `inv_transform_rays` on the 'matrix_6dof_rotation' camera parameters registered at
 * :49-51, then re-normalised directions) - what configs/bup20/best.yaml runs at the head of EVERY train step (optimize_extrinsics with
 * extrinsics_epoch_end 900 > epochs 800, pc_nerf/trainer.py:308) - and its gradient.
 *   params f32 [C,9] = (a1, a2, t) per camera:  b1 = a1/|a1|, b2 = normalise(a2 - (b1.a2) b1), b3 = b1 x b2,  R rows = (b1, b2, b3)
 *   cam i32 [ceil(N / rays_per_entry)]: ray i belongs to camera cam[i / rays_per_entry] (rays_per_entry = 1: one index per ray; = rays per
 *   image: one per image, the layout of `transform_rays`).  Indices must lie in [0, C); one outside is clamped to 0 / C - 1 in the forward AND the backward
 *   (the ray renders through that camera and sends its gradient there) - the tensor-op form would raise or wrap instead.
 *   origins_w[i] = sum_k (origins_c[i] - t)[k] R[k]        dirs_w[i] = normalise(sum_k dirs_c[i][k] R[k])          all f32 [N,3]
 * _bwd: d_params f32 [C,9] = d loss / d params from g_origins / g_dirs f32 [N,3] (either may be NULL = zero); EVERY row is written (zeros
 * for cameras without a ray in the batch); two launches (per-(camera, ray slice) partial sums into `workspace`, >= pag_pose_rays_bwd_workspace_bytes(C)
 * bytes; then one thread per camera), fixed summation order (bitwise reproducible). */
int pag_pose_rays_fwd(const float *params, int64_t C, const int32_t *cam, int64_t rays_per_entry, const float *origins_c, const float *dirs_c,
                      int64_t N, float *origins_w, float *dirs_w, void *stream);
int64_t pag_pose_rays_bwd_workspace_bytes(int64_t C);
int pag_pose_rays_bwd(const float *params, int64_t C, const int32_t *cam, int64_t rays_per_entry, const float *origins_c, const float *dirs_c,
                      int64_t N, const float *g_origins, const float *g_dirs, float *d_params, void *workspace, int64_t workspace_bytes, void *stream);

/* The position gradient of pag_*_encode_bwd_xyz reduced PER RAY inside the gather pass (pose optimisation, pc_nerf/ba_pipeline.py:85-92: the packed samples
 * are origin[ray] + dir[ray] * depth, so what is wanted of d loss / d xyz is its per-ray sum and its per-ray sum weighted by depth):
 *   out f32 [N,6], row r = (sum of d xyz over ray r's samples | sum of d xyz * depth); rays without samples get zeros.
 *   ridx i32 [M] = ray of each packed sample (non-decreasing), depths f32 [M], pack_start i64 [N+1] (one pack per ray, empty packs allowed);
 *   workspace >= pag_encode_bwd_rays_workspace_bytes(M, N) (6 floats per (XCD group, wave of 64 samples, ray) instead of 8 x 3 floats per sample).
 * Replaces pag_*_encode_bwd_xyz + pag_ray_sample_grad where the samples come straight from the ray march (fixed summation order: bitwise reproducible;
 * the sums are formed in a different order than by those two calls, so the values agree to fp32 rounding, not bit for bit).  Other arguments as
 * pag_*_encode_bwd_xyz.  (ABI 11) */
int64_t pag_encode_bwd_rays_workspace_bytes(int64_t M, int64_t N);
int pag_hash_encode_bwd_rays(const float *xyz, int64_t M, const void *tables, int table_dtype, const void *grad_out, int grad_dtype,
                             int64_t g_stride_m, int64_t g_stride_c, int layout, int n_levels, int n_feat, int log2_T,
                             const float *resolutions_host, const float *feat_scale_host, const int32_t *ridx, const float *depths,
                             const int64_t *pack_start, int64_t N, float *out, void *workspace, int64_t workspace_bytes, int flags, void *stream);
int pag_permuto_encode_bwd_rays(const float *xyz, int64_t M, const void *tables, int table_dtype, const void *grad_out, int grad_dtype,
                                int64_t g_stride_m, int64_t g_stride_c, int layout, int n_levels, int n_feat, uint32_t capacity,
                                const float *scale_factor_host, const float *shift_host, const float *feat_scale_host, const int32_t *ridx,
                                const float *depths, const int64_t *pack_start, int64_t N, float *out, void *workspace, int64_t workspace_bytes,
                                int flags, void *stream);

/* utils/outlier_rejection.py:74-97 `rays_to_3d_points` as pc_nerf/trainer.py:508-518 calls it (ABI 12): points f32 [N,3] = the camera-frame base rays
 * unprojected by depth f32 [N] and mapped to the world by the cameras' current extrinsics - sum_k (o_c - t + d_c depth)[k] R[k] with params / cam /
 * rays_per_entry as in pag_pose_rays_fwd.  No gradient (the trainer wraps the call in torch.no_grad()). */
int pag_pose_points(const float *params, int64_t C, const int32_t *cam, int64_t rays_per_entry, const float *origins_c, const float *dirs_c,
                    const float *depth, int64_t N, float *points, void *stream);

/* Gradient of pag_view_embed with respect to the directions (the view direction depends on the camera rotation: pc_nerf/ba_pipeline.py:89-90
 * -> pc_nerf/panoptic_delta_nef.py:196-200): d_dirs f32 [R,3] from g_out f32 [R, width].  (ABI 11) */
int pag_view_embed_bwd(const float *dirs, int64_t R, int n_freq, int width, const float *g_out, float *d_dirs, void *stream);

/* Touched-rows exchange of a table gradient (ABI 14; this build's multi-GPU addition, pagnerf_amd/shard.py::SparseRows - the reference is single-GPU): the four passes
 * around the collective.  After the first prune (configs/bup20/best.yaml:187, pc_nerf/trainer.py:362-366) the coarse and middle lattice levels touch few of their rows and
 * pag_*_encode_bwd_set leaves exact zeros elsewhere, so only the UNION over the ranks of the non-zero rows has to travel.
 *   pag_sparse_rows_mask    grad f32 [L][T][F] -> bits u32 [L][W], W = ceil(T / 32): bit r of word w = any(grad[l][32 w + r][:] != 0)
 *                           (the caller all_gathers the ranks' bits and ORs them)
 *   pag_sparse_rows_plan    union bits, caps i32 [L] (slots per level; caps[l] >= T: the level travels whole) -> word_prefix i32 [L][W] (union rows of the level before
 *                           word w; 32 w for a whole level), counts i64 [L + 1] (union rows per level; [L] = rows that do not fit their level's slots)
 *   pag_sparse_rows_pack    member rows in row order -> buf f32 [sum of slots][F] at offs[l] + rank while rank < caps[l] (offs i64 [L]); the caller zero-fills buf
 *   pag_sparse_rows_unpack  EVERY row of grad rewritten: a member with rank < caps[l] takes buf[offs[l] + rank], any other row 0
 * 1 <= F <= 64, T <= 2^31. */
int pag_sparse_rows_mask(const float *grad, int L, int64_t T, int F, uint32_t *bits, void *stream);
int pag_sparse_rows_plan(const uint32_t *bits, int L, int64_t T, const int32_t *caps, int32_t *word_prefix, int64_t *counts, void *stream);
int pag_sparse_rows_pack(const float *grad, int L, int64_t T, int F, const uint32_t *bits, const int32_t *word_prefix, const int32_t *caps, const int64_t *offs,
                         float *buf, void *stream);
int pag_sparse_rows_unpack(const float *buf, int L, int64_t T, int F, const uint32_t *bits, const int32_t *word_prefix, const int32_t *caps, const int64_t *offs,
                           float *grad, void *stream);

/* Semantic-NeRF decoder (pc_nerf/semantic_nerf.py:43-76, :188-224; additive, ABI 14): the whole network in one launch (mlp_deep.hip).
 *   e = PE10(coords) (63 wide, SURVEY Appendix A2 order); trunk: 8 x (Linear + ReLU) at width 256, layer 0 reads e, layer 5 reads cat([e, h]) (e in the
 *   first 63 columns), then lout 256 -> 256 without activation = feats; density = relu(Linear(256,1)(feats)); rgb = sigmoid(Linear(128,3)(relu(
 *   Linear(319,128)(cat([feats, PE10(-ray_d)]))))); semantics = Linear(128,C)(relu(Linear(256,128)(feats))), raw logits.
 * Rounding points: every Linear's input and weight are rounded to bf16 (round to nearest even), sums and biases are f32, sin / cos are the accurate ones.
 * W[i] / b[i] are the f32 nn.Linear tensors ([out,in] row major): 0..7 trunk layers, 8 lout, 9 density, 10 / 11 colour layers[0] / lout, 12 / 13 semantics
 * layers[0] / lout.  `channels` is a mask of PAG_DEEP_*; an output pointer is needed only for a requested channel; ray_d (f32 [M,3], per sample) only with
 * PAG_DEEP_RGB.  save = 0: nothing but the outputs is written (validation render, prune).  save = 1 (training forward): every Linear's bf16 input is kept
 * in the workspace for pag_deep_mlp_bwd; all three channels must then be requested.
 *   pag_deep_mlp_supported        1 when the fused path takes (hidden, num_classes): hidden == 256, 1 <= num_classes <= 16
 *   pag_deep_mlp_workspace_bytes  mode 0: forward with save = 0, 1: forward with save = 1, 2: backward (bwd_workspace); -1 on bad sizes
 *   pag_deep_mlp_fwd              density f32 [M], rgb f32 [M,3], semantics f32 [M,C]
 *   pag_deep_mlp_bwd              dW[i] / db[i] (f32, shapes of W[i] / b[i], overwritten) from the upstream gradients g_density [M], g_rgb [M,3],
 *                                 g_semantics [M,C] (f32; NULL = zero), the forward's density / rgb outputs and its save = 1 workspace.  Gradient operands
 *                                 (every layer's dz) are rounded to bf16 before both of their products; weight and bias gradients are per-workgroup
 *                                 partial sums added in a fixed order by a finish pass (no atomics: two runs give the same bits).  No gradient with
 *                                 respect to coords or ray_d.
 * Bad sizes, NULL buffers and short workspaces are refused before any launch; M == 0 is a no-op (nothing is written). */
enum { PAG_DEEP_DENSITY = 1, PAG_DEEP_RGB = 2, PAG_DEEP_SEMANTICS = 4 };
typedef struct pag_deep_mlp_args {
    const void *coords, *ray_d;
    int hidden, num_classes, channels, save;
    const void *W[14], *b[14];
    void *density, *rgb, *semantics;
    void *workspace;
    int64_t workspace_bytes;
    const void *g_density, *g_rgb, *g_semantics;
    void *dW[14], *db[14];
    void *bwd_workspace;
    int64_t bwd_workspace_bytes;
} pag_deep_mlp_args;
int pag_deep_mlp_supported(int hidden, int num_classes);
int64_t pag_deep_mlp_workspace_bytes(int64_t M, int hidden, int num_classes, int mode);
int pag_deep_mlp_fwd(const pag_deep_mlp_args *args, int64_t M, void *stream);
int pag_deep_mlp_bwd(const pag_deep_mlp_args *args, int64_t M, void *stream);

/* 128-wide decoders (additive, ABI 14; mlp_h128.hip): one wisp BasicDecoder at hidden width 128 per call - decoder_density / decoder_color /
 * decoder_semantics / decoder_inst of pc_nerf/panoptic_nef.py:114-164 with hidden_dim / sem_hidden_dim / inst_hidden_dim = 128 (config_parser.py:149's
 * default, main_hp_tunning.py:84-87's grid).  n_hidden (1 .. 3) Linear + ReLU layers of width `hidden` = 128, then lout: W[i] / b[i] are the f32 nn.Linear
 * tensors of layers[i] (i < n_hidden) and lout (i = n_hidden); out_dim <= 224, in_dim <= 64.  bf16 operands, f32 accumulate on the matrix cores: the
 * layer-0 input, every weight and every hidden activation are rounded to bf16 (round to nearest even), sums, biases and the output activation are f32.
 *   x1        PAG_LAYOUT_XCD8: the encoders' bf16 [8][M][8] tensor of x1_levels x x1_feats features (k1 = 64, in_dim = levels * feats, no x2), or
 *             PAG_LAYOUT_STRIDED: [M, k1] row-major, bf16 or f32, k1 % 8 == 0
 *   x2        f32 [R, k2p] or NULL, k2p % 8 == 0, rows gathered per sample through x2_index i32 [M]; k1 + k2p <= 64; input columns >= in_dim are ignored
 *   out       [M, out_dim] row-major, f32 or bf16, after out_act (PAG_ACT_*)
 *   workspace NULL (nothing but `out` is written: validation, prune) or pag_mlp128_workspace_bytes(M, n_hidden, out_dim, 1) bytes, 256-B aligned: the
 *             layer-0 input and every hidden layer's post-ReLU output, bf16, kept for pag_mlp128_bwd.  Plane layout ("native"): samples are padded to
 *             Mp = ceil(M / 256) * 256; the plane of columns [c0, c0 + 32 nb) starts at bf16 element Mp * c0 and holds, per 32-sample tile t and 32-column
 *             block blk, 64 x 4 chunks of 4 values: chunk (g, lane) = columns 32 blk + 8 g + 4 (lane >> 5) + 0..3 of sample 32 t + (lane & 31), at element
 *             ((t * nb + blk) * 4 + g) * 256 + 4 lane.  Planes: the input (64 positions) at column 0, h_l at 64 + 128 l.
 * pag_mlp128_bwd: data and weight gradients.  grad_out [M, out_dim] in out's dtype, `out` the forward's output (sigmoid / softmax).  Writes
 *   bwd_workspace  pag_mlp128_workspace_bytes(M, n_hidden, out_dim, 2) bytes: first the pre-activation gradients dz_l as bf16 native planes (dz_l at column
 *             128 l, the output layer's after them) - dz_0, the first plane, is what the caller sums per ray for the gradient of x2 -, then the weight
 *             gradients' partial sums
 *   dx1       NULL or the gradient of x1 in x1's form: bf16 [8][M][8] with padding positions zero (dx1_accumulate = 1: added to what is there), or
 *             [M, k1] (dx1_dtype bf16 / f32), columns >= in_dim zero
 *   dW[i], db[i]   f32, shapes of W[i] / b[i], overwritten: per-workgroup partial sums added in a fixed order by a finish launch (no atomics: two runs give
 *             the same bits)
 * pag_mlp128_workspace_bytes(M, n_hidden, out_dim, mode), with Mp as above, ob = 1 (out_dim <= 32), 4 (<= 128) or 7, align = round up to 256:
 *   mode 0 (forward, nothing saved)  0
 *   mode 1 (forward, saving)         align(Mp * (64 + 128 n_hidden) * 2)
 *   mode 2 (backward)                align(Mp * (128 n_hidden + 32 ob) * 2) + align(128 * (128 n_hidden + 32 ob) * 129 * 4)
 *   -1 for M < 0, M > PAG_MLP128_MAX_M or an unsupported shape; 0 for M == 0.
 * pag_mlp128_supported: 1 when (n_hidden, hidden, in_dim, out_dim) is a shape these kernels take.
 * The forward launches min(ceil(M / 256), 256) workgroups of 256 samples each and grid-strides.  Every sample offset is 64-bit; M above PAG_MLP128_MAX_M is
 * refused (PAG_ERR_ARG).  Bad sizes, NULL buffers and short workspaces are refused before any launch, the message naming the field; M == 0 is a no-op. */
#define PAG_MLP128_MAX_M ((int64_t)1 << 26)
typedef struct pag_mlp128_fwd_args {
    const void *x1; int x1_dtype; int k1;
    int x1_layout; int x1_levels; int x1_feats;
    const float *x2; int k2p; const int32_t *x2_index;
    int in_dim; int n_hidden; int hidden; int out_dim;
    const float *W[4]; const float *b[4];
    int out_act;
    void *out; int out_dtype;
    void *workspace; int64_t workspace_bytes;
} pag_mlp128_fwd_args;
typedef struct pag_mlp128_bwd_args {
    const void *grad_out; const void *out; int out_dtype; int out_act;
    int k1; int k2p; int in_dim; int n_hidden; int hidden; int out_dim;
    int x1_layout; int x1_levels; int x1_feats;
    const float *W[4];
    const void *workspace; int64_t workspace_bytes;       /* the forward's */
    void *bwd_workspace; int64_t bwd_workspace_bytes;
    void *dx1; int dx1_dtype; int dx1_accumulate;
    float *dW[4]; float *db[4];
} pag_mlp128_bwd_args;
int pag_mlp128_supported(int n_hidden, int hidden, int in_dim, int out_dim);
int64_t pag_mlp128_workspace_bytes(int64_t M, int n_hidden, int out_dim, int mode);
int pag_mlp128_fwd(const pag_mlp128_fwd_args *args, int64_t M, void *stream);
int pag_mlp128_bwd(const pag_mlp128_bwd_args *args, int64_t M, void *stream);

/* TensoRF vector-matrix grid (grids/tensorf.py::VMSplitFeatureVolume; additive, ABI 14): vm.hip.  f32 tables, f32 arithmetic.
 * Tables are CHANNEL-LAST: plane i is f32 [R][R][C] (row = the pair's second coordinate, column = its first: matMode [[0,1],[0,2],[1,2]]), line i is
 * f32 [R][C] along coordinate vecMode[i] = 2 - i; C = 16 for the density set, 48 for the appearance set; basis is the Linear(144, 27) weight [27][144]
 * (column = plane * 48 + component).  Sampling is grid_sample's bilinear / align_corners / zero padding: pixel = ((c + 1) / 2) * (R - 1), taps outside
 * the table contribute 0.
 *   sigma[m] = sum_i sum_c plane_i,c(m) * line_i,c(m)          (density set)
 *   app[m]   = basis . cat_i(plane_i(m) * line_i(m))           (appearance set; the 144-wide product stays on chip)
 *   pag_vm_supported            1 for density_n_comp == 16, app_n_comp == 48, app_dim == 27, 2 <= res <= 2048; 0 otherwise
 *   pag_vm_bwd_workspace_bytes  bytes of `workspace` pag_vm_bwd needs for M samples (the basis gradient's per-workgroup partial sums); -1 for M < 0
 *   pag_vm_fwd                  xyz f32 [M,3] -> sigma f32 [M] and / or app f32 [M,27]; either output may be NULL (not both)
 *   pag_vm_bwd                  g_sigma f32 [M] and / or g_app f32 [M,27] (NULL = zero, not both) -> the table gradients, ADDED with float atomics into
 *                               g_* (same layouts as the tables; the caller zero-fills them; a set whose upstream gradient is NULL may have NULL
 *                               gradient tables), and g_basis f32 [27][144], OVERWRITTEN from partial sums added in a fixed order (needed with g_app).
 *                               The taps are recomputed from xyz.  A sample whose upstream gradients are all exactly zero writes nothing.  No gradient
 *                               with respect to xyz (the reference detaches the coordinates).
 * Bad sizes, NULL buffers and a short workspace are refused before any launch; M == 0 is a no-op (nothing is written). */
typedef struct pag_vm_args {
    const float *density_plane[3], *density_line[3], *app_plane[3], *app_line[3], *basis;
    int density_n_comp, app_n_comp, app_dim, res;
    const float *xyz;
    float *sigma, *app;
    const float *g_sigma, *g_app;
    float *g_density_plane[3], *g_density_line[3], *g_app_plane[3], *g_app_line[3], *g_basis;
    void *workspace;
    int64_t workspace_bytes;
} pag_vm_args;
int pag_vm_supported(int density_n_comp, int app_n_comp, int app_dim, int res);
int64_t pag_vm_bwd_workspace_bytes(int64_t M);
int pag_vm_fwd(const pag_vm_args *args, int64_t M, void *stream);
int pag_vm_bwd(const pag_vm_args *args, int64_t M, void *stream);

/* Tri-plane feature grid (wisp TriplanarGrid, selected by configs/bup20/mean_shift_contrastive_app.yaml:137-144; additive, ABI 14): triplanar.hip.
 * Replaces the tensor-op form of pagnerf_amd/triplanar.py (per level three torch grid_sample calls and their sum).  f32 tables, f32 arithmetic.
 * Level l has resolution res_host[l] (a HOST array of n_levels ints, 2 <= res <= 8193) and three planes fmx, fmy, fmz; `tables` is ONE flat f32 buffer, 16-byte
 * aligned, level after level, each level [3][R][R][F] channel-last (plane, row, column, feature).  Plane fmx reads (y, z), fmy (x, z), fmz (x, y): the
 * pair's first coordinate indexes the columns, the second the rows.  Sampling is grid_sample's bilinear / align_corners / reflection padding:
 *   pixel = ((c + 1) / 2) * (R - 1), reflected about [0, R - 1], clipped; the taps nw, ne, sw, se; the tap at index R is skipped.
 *   out[m, l*F + f] = ((fmx_l + fmy_l) + fmz_l)[f] * feat_scale_host[l*F + f]   (a HOST array of n_levels * n_feat floats, or NULL = 1)
 * n_levels in [1, 8], n_feat in {2, 4, 8}.
 *   pag_triplanar_fwd          xyz f32 [M,3] -> out [M, L*F] via strides, PAG_F32 or PAG_BF16 (the f32 result rounded once)
 *   pag_triplanar_bwd_tables   grad_out [M, L*F] via strides (PAG_F32 or PAG_BF16) -> grad_tables f32 (the flat layout), ADDED with float atomics (the
 *                              caller zero-fills it).  The taps are recomputed from xyz; a sample whose upstream gradient row is exactly zero adds nothing.
 *   pag_triplanar_bwd_xyz      d loss / d xyz f32 [M,3], OVERWRITTEN, from grad_out and the tables: d pixel / d c = +-(R - 1) / 2 by the parity of the
 *                              reflection, 0 where the clip is active (grid_sample's backward).  No atomics: fixed bits.
 * Bad sizes and NULL buffers are refused before any launch; M == 0 is a no-op (nothing is written). */
int pag_triplanar_fwd(const float *xyz, int64_t M, const float *tables, int n_levels, int n_feat, const int *res_host, const float *feat_scale_host,
                      void *out, int out_dtype, int64_t stride_m, int64_t stride_c, void *stream);
int pag_triplanar_bwd_tables(const float *xyz, int64_t M, const void *grad_out, int grad_dtype, int64_t stride_m, int64_t stride_c, int n_levels, int n_feat,
                             const int *res_host, const float *feat_scale_host, float *grad_tables, void *stream);
int pag_triplanar_bwd_xyz(const float *xyz, int64_t M, const float *tables, const void *grad_out, int grad_dtype, int64_t stride_m, int64_t stride_c,
                          int n_levels, int n_feat, const int *res_host, const float *feat_scale_host, float *d_xyz, void *stream);

/* Lattice total variation (loss/regularizers.py:41-54, the grid TV terms of pc_nerf/trainer.py:556-574; additive, ABI 14): regularizer.hip.
 * `values` is channel-last and contiguous, viewed as [d0, d1, d2, C] (the lattice extents of the input padded with trailing 1s, then the channels), dtype
 * PAG_F32 / PAG_F16 / PAG_BF16; every difference, product and partial sum is f32, the final combine f64, every element offset 64-bit.
 *   out[0] = (1 / d0) * sum over the axes and over the points p with a +1 neighbour of phi(v[p + e_axis] - v[p]),   phi = |.| (power 1) or (.)^2 (power 2)
 * - EVERY axis is divided by d0, the reference's `values.shape[0]` (:43, :47).  An axis of extent 1 contributes nothing.
 *   grad[p] = (upstream[0] / d0) * sum over the axes of [phi'(v[p] - v[p - e]) - phi'(v[p + e] - v[p])], a face without a neighbour has no term;
 *   phi'(t) = sign(t) with sign(0) = 0 (power 1), 2 t (power 2).  grad has the dtype of values (the f32 result rounded once); upstream is DEVICE f32 [1].
 *   Every term is scaled by s = upstream[0] * (1 / d0) on its own and the terms are added in the order of the tensor-op form's backward (an axis's two
 *   faces first, then the axes last to first), so that a half gradient is the form's f32 gradient rounded.
 * Sums: f32 per thread, a fixed butterfly per wave, the waves in order, one partial per workgroup in `workspace` (pag_tv_workspace_bytes bytes, a function
 * of the sizes only), then one workgroup adds the partials in f64 in a fixed order.  No floating-point atomics: the same input gives the same bits.
 * 16-byte channel vectors are used when C is a multiple of 4 (f32) / 8 (f16, bf16) and the buffers are 16-byte aligned, single elements otherwise.
 * Extents < 1, C outside [1, 2^24], more than 2^46 elements, a power other than 1 or 2, a bad dtype, NULL buffers and a short workspace are refused
 * (PAG_ERR_ARG) before any launch; pag_tv_workspace_bytes returns 0 for sizes that would be refused. */
int64_t pag_tv_workspace_bytes(int64_t d0, int64_t d1, int64_t d2, int64_t C);
int pag_tv_fwd(const void *values, int dtype, int64_t d0, int64_t d1, int64_t d2, int64_t C, int power, void *workspace, int64_t workspace_bytes,
               float *out, void *stream);
int pag_tv_bwd(const void *values, int dtype, int64_t d0, int64_t d1, int64_t d2, int64_t C, int power, const float *upstream, void *grad, void *stream);

/* Ray sampling of a device-resident multiview dataset (datasets/transforms/ray_sampler.py:17-40, the per-image indexing and collation of
 * datasets/multiview_dataset.py:177-192; additive, ABI 14): sample.hip.  One launch draws slot_count pixels without replacement for each of B views and
 * gathers the pixels' rows of up to PAG_SAMPLE_MAX_MODES modes into the collated batch.
 *   state   DEVICE int64 [2] = {seed, draw}, read by the kernel (a captured graph replays with the draw that is there at replay time)
 *   views   DEVICE int32 [B], the view of each batch row; repeats allowed; a view outside [0, num_views) yields zero rows and ray_idx -1
 *   pixel of output row (b, j) = slot slot_begin + j of the first min(k, n) entries of the keyed permutation of [0, n) with key (seed, draw, views[b]):
 *           pagnerf_amd.dataset.sample_indices is the definition (6-round balanced Feistel network on the smallest even bit width >= max(2,
 *           bit_length(n - 1)), murmur3-finaliser round function and key schedule, cycle-walked into [0, n); uint32 arithmetic only), reproduced exactly.
 *           Slot j depends on (seed, draw, view, n, j) alone - not on k, the slice or the launch shape.
 *   mode    src is [num_views, n, row] (per_view != 0) or [n, row] (shared); dst is [B, slot_count, row_bytes]; row_bytes counts a DESTINATION row.
 *           PAG_SAMPLE_COPY copies row_bytes bytes (any dtype); PAG_SAMPLE_U8_TO_F32 reads row_bytes / 4 uint8 and writes (float)u / 255.0f
 *           (IEEE division, torch's CPU `x.float() / 255`), so row_bytes must be a multiple of 4.  Rows move at the widest of 16 / 8 / 4 / 2 / 1 bytes that
 *           divides row_bytes and both base addresses (pag_sample_copy_width returns it; 4 or 1 source bytes per step for a conversion; 0 = refused).
 *   ray_idx int64 [B, slot_count] or NULL: the pixel.   cam_idx int32 [B * slot_count] or NULL: views[b] of the row, the per-ray camera row that
 *           pc_nerf/ba_pipeline.py:85-92 in its per-ray form takes.
 * Source offsets are 64-bit.  No atomics, no workspace.  Refused (PAG_ERR_ARG) before any launch: n outside [1, 2^30], k < 1, B outside [0, 65535],
 * num_views < 1, more than PAG_SAMPLE_MAX_MODES modes, row_bytes outside [1, 2^20], an unknown conversion or one that does not fit row_bytes, slot_begin < 0,
 * slot_count < 0 or slot_begin + slot_count > min(k, n), NULL pointers.  B == 0 or slot_count == 0 is a no-op.
 * pag_sample_advance: state[1] += 1 as a one-thread launch; inside a captured step the sequence is sample, ..., advance. */
#define PAG_SAMPLE_MAX_MODES 12
enum { PAG_SAMPLE_COPY = 0, PAG_SAMPLE_U8_TO_F32 = 1 };
typedef struct pag_sample_mode {
    const void *src;
    void *dst;
    int64_t row_bytes;
    int32_t per_view;
    int32_t convert;
} pag_sample_mode;
int pag_sample_copy_width(const void *src, const void *dst, int64_t row_bytes, int convert);
int pag_sample_batch(const int64_t *state, const int32_t *views, int B, int num_views, int64_t n, int64_t k, int64_t slot_begin, int64_t slot_count,
                     const pag_sample_mode *modes, int n_modes, int64_t *ray_idx, int32_t *cam_idx, void *stream);
int pag_sample_advance(int64_t *state, void *stream);

/* Validation pictures (pc_nerf/trainer.py:710-829 and :855-896: the imgviz label_colormap / label2rgb / depth2rgb, torchvision masks_to_boxes /
 * draw_bounding_boxes and 0.7-blend chain of evaluate_metrics, per image; additive, ABI 14): visualize.hip.  Two launches for one H x W image:
 * pag_vis_stats, then pag_vis_paint, which writes every requested uint8 [H,W,3] picture once.  pagnerf_amd/visualize.py holds the tensor-op forms
 * (`*_reference`) that define every picture bit for bit; the file is built without FMA contraction.
 *   rgb      f32 (rgb_is_u8 == 0: the picture is trunc(clamp(x, 0, 1) * 255), NaN -> 0) or uint8 (taken as it is), rgb_stride elements per pixel (>= 3)
 *   gt       f32, gt_stride floats per pixel;   depth f32 [H,W];   conf[2] f32 [H,W] (inst_conf, inst_conf_pred)
 *   labels   PAG_VIS_L_*: int64 / int32 / uint8 (label_bytes 8 / 4 / 1) [H,W], NULL = absent
 *   table    uint8 [256,3], the colour map of the depth and confidence pictures
 *   out      PAG_VIS_*: the plane of each picture, NULL = not painted and not touched.  A requested picture whose inputs are absent is refused.
 * Label colour: the PASCAL-VOC bit procedure on the id's low 24 bits (for j = 0..7: r |= bit0 << (7-j), g |= bit1 << (7-j), b |= bit2 << (7-j),
 * id >>= 3); a negative id is black.  *_RGB of the semantic pictures: grey = rint(0.299f R + 0.587f G + 0.114f B) of the rgb picture,
 * rint(blend_keep * grey + blend_alpha * colour).  Depth: t = (d - min) / (max - min) over the finite minimum / maximum, index min(255, floor(t * 256)),
 * non-finite d black, max == min index 0; the confidences the same with the fixed range [conf_min, conf_max] and t clamped to [0, 1].
 * INST_RGB / INST_PRED_RGB: the rgb picture, then the outline (box_width pixels inward, the highest id on top) of the inclusive pixel box of every id
 * in [1, max_id] of labels[L_INST] / labels[L_INST_PRED] in the id's colour, then per channel where the label colour's channel is non-zero
 * trunc(overlay_keep * base + overlay_alpha * colour).
 * Workspace: int32, two halves of 4 + 8 * (max_id + 1) words each: {min key, max key, 0, 0}, then the box tables (x0, y0, x1, y1) of L_INST and
 * L_INST_PRED.  The caller initialises BOTH halves once to {-1, 0, 0, 0} and (INT32_MAX, INT32_MAX, -1, -1) per id; pag_vis_stats reduces into half
 * `phase` (LDS per workgroup, then integer min / max atomics: order-independent, the same input gives the same bits; an absent id keeps x0 > x1) -
 * the depth range when `depth` is given, a box table when its label image is given - and pag_vis_paint reads half `phase` and re-initialises half
 * `phase ^ 1`, so a caller that alternates `phase` never launches a fill.  Keys: the f32 bits made monotone (sign bit flipped / all bits flipped).
 * Refused (PAG_ERR_ARG) before any launch: H, W < 1 or H * W * 3 >= 2^31, max_id outside [1, 1023], box_width < 1, a label_bytes other than 8 / 4 / 1,
 * strides < 3, phase outside {0, 1}, a short or NULL workspace, a requested picture without its inputs. */
#define PAG_VIS_PICTURES 15
#define PAG_VIS_LABELS 6
#define PAG_VIS_MAX_ID 1023
enum { PAG_VIS_RGB = 0, PAG_VIS_GT, PAG_VIS_DEPTH, PAG_VIS_SEM, PAG_VIS_SEM_RGB, PAG_VIS_SEM_GT, PAG_VIS_SEM_PRED, PAG_VIS_SEM_PRED_RGB, PAG_VIS_INST,
       PAG_VIS_INST_CONF, PAG_VIS_INST_RGB, PAG_VIS_INST_GT, PAG_VIS_INST_PRED, PAG_VIS_INST_PRED_RGB, PAG_VIS_INST_CONF_PRED };
enum { PAG_VIS_L_SEM = 0, PAG_VIS_L_INST, PAG_VIS_L_SEM_GT, PAG_VIS_L_INST_GT, PAG_VIS_L_SEM_PRED, PAG_VIS_L_INST_PRED };
typedef struct pag_vis_args {
    int32_t H, W;
    const void *rgb;
    int32_t rgb_is_u8, rgb_stride;
    const float *gt;
    int32_t gt_stride, phase;
    const float *depth;
    const void *labels[PAG_VIS_LABELS];
    int32_t label_bytes[PAG_VIS_LABELS];
    const float *conf[2];
    const unsigned char *table;
    int32_t max_id, box_width;
    float blend_keep, blend_alpha, overlay_keep, overlay_alpha, conf_min, conf_max;
    int32_t *workspace;
    int64_t workspace_bytes;
    unsigned char *out[PAG_VIS_PICTURES];
} pag_vis_args;
int64_t pag_vis_workspace_bytes(int max_id);
int pag_vis_stats(const pag_vis_args *args, void *stream);
int pag_vis_paint(const pag_vis_args *args, void *stream);

/* View preparation of a NeRF-standard dataset (datasets/formats/nerf_standard.py:57-60 img_as_float32 + resize_mip, :239-267 the per-view ray grid,
 * :269-282 masks and the alpha composite; datasets/formats/bup20.py:203-229 the nearest label resample; additive, ABI 14): prepare.hip.
 * pagnerf_amd/formats.py holds the tensor-op forms (`prepare_views_reference`, `prepare_labels_reference`, `rays_reference`) that define the results.
 *   src      DEVICE uint8 [B, H0, W0, C0], C0 = 3 or 4: the decoded frames of a chunk.  f = 2^mip must divide H0 and W0; h = H0 / f, w = W0 / f.
 *   imgs     f32 [V, h, w, 3]: per channel (float)S / (float)(255 f f), S the integer sum of the f x f block, one IEEE division; with C0 = 4 composited
 *            onto the background with a = the fourth channel: PAG_BG_WHITE clamp((v * a) + (1 - a), 0, 1), PAG_BG_BLACK clamp(v - (1 - a), 0, 1), three
 *            roundings in that order (built without FMA contraction): bit for bit the definition.
 *   masks    uint8 [V, h, w, 1]: a > 0.5 (1 with C0 = 3)
 *   origins  f32 [V, h, w, 3]: c2w[v][:, 3], a copy.    c2w: DEVICE f32 [V, 3, 4], camera -> world, indexed by the DESTINATION view
 *   dirs     f32 [V, h, w, 3]: normalise(R d_cam), R = c2w[v][:, :3], d_cam = ((x + 0.5 - w/2 - x0) / fx, -(y + 0.5 - h/2 - y0) / fy, -1)
 * Chunk view b is written to view view_offset + b of every destination; any subset of the four outputs may be NULL (not written; src is needed for imgs /
 * masks only, c2w for origins / dirs only).  One launch; a thread per output pixel, an RGBA pixel read as one word (8- and 16-byte vectors along a block
 * row where f and the address of src allow), RGB and sources that are not word-aligned by bytes; the destinations need their dtype's alignment only.
 * No atomics, no workspace.  Refused (PAG_ERR_ARG) before any launch: mip outside [0, 8], B outside
 * [0, 65535], C0 other than 3 / 4, sizes < 1 or not divisible by f, more than 2^30 output pixels, view_offset < 0 or view_offset + B > V, an unknown
 * background, a NULL src / c2w that a requested output needs, a zero or NaN focal length with dirs.  B == 0 or no output is a no-op.
 * pag_prepare_labels: all label planes of a chunk in one launch: dst[view_offset + b][y][x] = src[b][y f][x f] for each plane (src DEVICE uint8
 * [B, H0, W0], dst int64 [V, h, w, 1]); at most PAG_PREPARE_MAX_PLANES planes, the same size checks, NULL planes refused. */
#define PAG_PREPARE_MAX_PLANES 8
typedef struct pag_label_plane {
    const void *src;
    int64_t *dst;
} pag_label_plane;
int pag_prepare_views(const void *src, int B, int H0, int W0, int C0, int mip, int bg, const float *c2w, float fx, float fy, float x0, float y0,
                      int64_t view_offset, int64_t V, float *imgs, unsigned char *masks, float *origins, float *dirs, void *stream);
int pag_prepare_labels(const pag_label_plane *planes, int n_planes, int B, int H0, int W0, int mip, int64_t view_offset, int64_t V, void *stream);

/* The BUP20 loader's device work (datasets/formats/bup20.py:189-234 on agrobot_base.py:442-461 the depth filter of the detector's instance masks and
 * :524-547 the label planes from COCO annotations; additive, ABI 14): bup20.hip.  pagnerf_amd/bup20.py holds the tensor-op / NumPy forms that define the
 * results (`polygon_keys_reference`, `coco_labels_reference`, `pred_stats_reference`, `prepare_frames_reference`) and builds the tables (`coco_tables`);
 * every output is bit for bit the definition.
 *
 * Ground-truth labels.  All tables are DEVICE int32 arrays for the B frames of a chunk (n_* are host numbers):
 *   verts [n_verts, 2]        the rounded vertices trunc(5 v + 0.5) of every polygon part, ring not closed
 *   part_vert_begin [n_parts+1]   a part's vertices; an RLE part has none
 *   point_begin [n_verts+1]   prefix sums of the per-edge boundary point counts max(|dX|, |dY|) + 1 (edge e starts at vertex e)
 *   part_key_begin [n_parts+1]    a part's slice of `keys`: an upper bound of its key count (polygon) or its count (RLE)
 *   part_key_count [n_parts]  keys in the slice: written per polygon part, given for an RLE part, whose keys are in `keys` already
 *   ann_part_begin [n_anns+1], ann_label [n_anns]    an annotation's parts and its class index
 *   ann_cover [n_anns]        H0 W0 for an annotation known to cover the image, else 0; the counting pass adds the covered pixels of the annotations
 *                             in cand [n_cand] (so one pag_coco_labels call per set of tables)
 *   frame_ann_begin [B+1], frame_labelled [B]        a frame's annotations; a frame with frame_labelled 0 becomes -1 everywhere
 *   max_part_keys             the largest polygon part's key bound, computed by the host from the vertices
 * pag_coco_keys: one workgroup per polygon part walks its boundary points (a lane per consecutive pair, the points from their edge's closed form with
 * one fp64 line each), keeps the pairs that cross a pixel column, and sorts the part's keys X H0 + Y in LDS.  pag_coco_labels: a thread per output pixel
 * (y, x) of the h x w = H0 / 2^mip x W0 / 2^mip plane reads source pixel (y 2^mip, x 2^mip): covered by a part iff the number of its keys <= x H0 + y is
 * odd, by an annotation iff by any of its parts; semantics = min(max_label, sum of the covering annotations' labels, starting again from zero at an
 * annotation that covers all H0 W0 pixels), instance = 1 + the index within the frame of the last covering annotation, else 0; int64 [V, h, w, 1] each,
 * written at view view_offset + b, either may be NULL.  With n_cand > 0 a counting launch precedes it (integer atomics, one per wave).
 * Refused (PAG_ERR_ARG) before any launch: max_part_keys above PAG_COCO_MAX_PART_KEYS (that image takes the tensor-op form), (W0 + 1) H0 >= 2^31, B or
 * n_cand outside [0, 65535], negative counts, NULL tables that a count says are read, mip outside [0, 8], sizes not divisible by 2^mip, views outside
 * [0, V). */
#define PAG_COCO_MAX_PART_KEYS 4096
typedef struct pag_coco_tables {
    const int32_t *verts, *part_vert_begin, *point_begin, *part_key_begin;
    int32_t *part_key_count, *keys;
    const int32_t *ann_part_begin, *ann_label;
    int32_t *ann_cover;
    const int32_t *cand, *frame_ann_begin, *frame_labelled;
    int32_t n_verts, n_parts, n_anns, n_cand, B, max_part_keys;
} pag_coco_tables;
int pag_coco_keys(const pag_coco_tables *tables, int H0, int W0, void *stream);
int pag_coco_labels(const pag_coco_tables *tables, int H0, int W0, int mip, int max_label, int64_t view_offset, int64_t V, int64_t *semantics,
                    int64_t *instance, void *stream);
/* pag_bup20_pred_stats: counts int32 [B, n_ids, 2], ZEROED by the caller, += per view and instance id (pixels, pixels whose depth d = (float)raw * 0.001f
 * has 0 < d <= max_depth); inst DEVICE int32 [B, H0, W0] with ids in [0, n_ids), depth DEVICE uint16 [B, H0, W0].  Integer atomics (a workgroup
 * histogram in LDS up to 2048 ids).  Refused: B outside [0, 65535], H0 W0 outside [1, 2^24), n_ids outside [1, 2^24], max_depth <= 0, NULL buffers.
 * pag_bup20_prepare: one launch per chunk, a thread per output pixel, every destination may be NULL, chunk view b goes to view view_offset + b:
 *   kept(id) = 2 valid > total from counts (NULL: everything is kept); inst' = inst if kept else 0; sem' = 0 where inst' = 0 (with counts only)
 *   semantics_pred, instance_pred int64 [V, h, w, 1]: sem', inst' at source pixel (y f, x f), f = 2^mip
 *   imgs f32 [V, h, w, 3], depths, sem_conf_out, inst_conf_out f32 [V, h, w, 1]: f = 1 the source value, else ((0.25 a + 0.25 b) + 0.25 c) + 0.25 d of
 *   the source pixels at offsets f/2 - 1 and f/2 in each axis (a top-left, b top-right, c bottom-left, d bottom-right), fp32, not contracted; an image
 *   value is (float)u8 / 255f, a depth (float)raw * 0.001f, a confidence 1 where the filter removed the pixel's instance.  masks uint8 [V, h, w, 1]: 1
 *   with C0 = 3; with C0 = 4 alpha > 0.5 and the image composited as pag_prepare_views does.
 * Refused before any launch: mip outside [0, 8], B outside [0, 65535], sizes < 1, not divisible by f or above 2^30 pixels, views outside [0, V), C0
 * other than 3 / 4, an unknown background, a destination without its source, counts without inst or with 2^24 pixels or more. */
typedef struct pag_bup20_prepare_args {
    const unsigned char *img;          /* [B, H0, W0, C0] */
    const uint16_t *depth;             /* [B, H0, W0] */
    const int32_t *sem, *inst;         /* [B, H0, W0] */
    const float *sem_conf, *inst_conf; /* [B, H0, W0] */
    const int32_t *counts;             /* [B, n_ids, 2] or NULL */
    int32_t B, H0, W0, C0, mip, bg, n_ids;
    int64_t view_offset, V;
    float *imgs;
    unsigned char *masks;
    float *depths;
    int64_t *semantics_pred, *instance_pred;
    float *sem_conf_out, *inst_conf_out;
} pag_bup20_prepare_args;
int pag_bup20_pred_stats(const int32_t *inst, const void *depth_u16, int B, int H0, int W0, float max_depth, int n_ids, int32_t *counts, void *stream);
int pag_bup20_prepare(const pag_bup20_prepare_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PAGNERF_HIP_H */
