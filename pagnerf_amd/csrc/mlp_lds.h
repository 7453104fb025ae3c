// Dynamic-LDS layouts of the decoder kernels in mlp.hip (the file itself and its headers mlp_generic.h and mlp_f32.h hold them; mlp_tile.h takes the
// constants) and mlp_wgrad.hip - nothing else includes this: ONE description per kernel serves the
// carve-up inside the kernel (lds_at<T>(smem, L.region)) and the byte count its launcher asks for (L.bytes), so the two cannot drift apart.
// Constants and constexpr code only - a plain host program can include this file and print every size.
// Conventions: every member is an offset in BYTES from the start of the dynamic segment; regions follow each other in declaration order; a
// wave-private region is its wave-0 offset plus `wave * <name>_stride`; `bytes` is the total.
// The kernels are pinned instruction for instruction (scripts/kernel_digest.py), which decides how a kernel may WRITE the use of its layout:
// the per-wave term is added in the kernel body (inside a helper the schedule moves), and where the layout depends on a run-time block count
// absolute offsets compile differently from the pointer chain (the compiler no longer shares OB * 32 with the loop bounds).  mlp_bwd_wide_mfma
// therefore chains differences of its layout's offsets; mlp_fwd_mfma and head_composite_fwd_kernel, where that changes the code as well, keep
// the chain written out beside a comment naming their layout - only their launchers use it.
#pragma once

namespace pagmlp {

constexpr int LDS_MAX_BYTES = 160 * 1024;       // gfx950: LDS per workgroup (kernels above 64 KiB opt in: raise_lds_limit)
constexpr int OB_MAX = 7;                       // 32-row blocks of the widest output layer (out_dim <= 224)
constexpr int HID = 64;
constexpr int RS = 72;                          // LDS row stride (bf16 elements) of a 64-wide weight row: 144 B
constexpr int ST_RS = 72;                       // staging row stride in bf16 (144 B: conflict-light for b64 and b128)
constexpr int ST_BYTES = 32 * ST_RS * 2;        // 4608 B per wave
constexpr int TW_ELEMS = 32 * 64;               // bf16 elements of a swizzled 32-sample tile (4 KiB)
constexpr int WR_RS = 256;                      // floats per staged gradient row
constexpr int WB_RMAX = 4;                      // rays whose gradient rows are staged per tile; tiles spanning more read their rows from global
constexpr int WIDE_BWD_WAVES = 8;               // waves per workgroup of mlp_bwd_wide_mfma (one workgroup per CU; 16 would not fit the LDS at 7 blocks)
constexpr int PT = 128;                        // threads per block on the FP32 path
constexpr int WG_RS = 72;                       // LDS row stride (bf16) of the transposed weight-gradient tiles: 64 samples + 8 pad

constexpr int W64 = 64 * RS * 2, W32 = 32 * RS * 2;      // bytes of a [64][RS] / [32][RS] bf16 weight image
constexpr int TW_BYTES = TW_ELEMS * 2;

// mlp_fwd_mfma, mlp_fwd_fast (ob = 1), mlp_fwd_wide_stats and head_fwd_once_kernel (n_layers = 3, ob = 7): the forward weight images
// (W0 natural k, the others permuted k), PAIR's companion head, the biases, head_fwd_once_kernel's per-wave ray sums [4][ob*32], staging tiles
struct FwdLds {
    int W0, W1, WL, W0p, WLp, b0, b1, bL, b0p, bLp, red, stg, stg_stride, bytes;
    constexpr FwdLds(int n_layers, int ob, int waves = 4, bool pair = false, bool ray_sums = false)
        : W0(0), W1(W0 + W64), WL(W1 + (n_layers == 3 ? W64 : 0)), W0p(WL + ob * W32), WLp(W0p + (pair ? W64 : 0)), b0(WLp + (pair ? W32 : 0)),
          b1(b0 + 64 * 4), bL(b1 + 64 * 4), b0p(bL + ob * 32 * 4), bLp(b0p + (pair ? 64 * 4 : 0)), red(bLp + (pair ? 32 * 4 : 0)),
          stg(red + (ray_sums ? 4 * ob * 32 * 4 : 0)), stg_stride(ST_BYTES), bytes(stg + waves * stg_stride) {}
};
// mlp_fwd_density_colour: density decoder (W0 natural k, WL permuted k), colour decoder (W0 natural, W1 and WL permuted), their biases; no staging
struct DensityColourLds {
    int W0d = 0, WLd = W0d + W64, W0c = WLd + W32, W1c = W0c + W64, WLc = W1c + W64, b0d = WLc + W32, bLd = b0d + 64 * 4, b0c = bLd + 32 * 4,
        b1c = b0c + 64 * 4, bLc = b1c + 64 * 4, bytes = bLc + 32 * 4;
};
// mlp_bwd_mfma: W_L^T [64][rsl] (k = output channel, permuted), W_1^T (n_layers = 3), W_0^T [64][RS], staging tiles
struct BwdLds {
    int rsl, WLt, W1t, W0t, stg, stg_stride, bytes;
    constexpr BwdLds(int n_layers, int ob)
        : rsl(ob * 32 + 8), WLt(0), W1t(WLt + 64 * rsl * 2), W0t(W1t + (n_layers == 3 ? W64 : 0)), stg(W0t + W64), stg_stride(ST_BYTES), bytes(stg + 4 * stg_stride) {}
};
// mlp_bwd_fused: the transposed images as in BwdLds, the forward's images W0s / W1s and hidden biases (the activations are recomputed), per wave
// the swizzled tiles Tx | Th0 | Th1 (n_layers = 3; else Th1 = Th0) | Tz, and for DZ0 == 2 per wave lray[32] | rid[32] (int)
struct FusedLds {
    int rsl, WLt, W1t, W0t, W0s, W1s, b0, b1, Tx, Th0, Th1, Tz, tile_stride, rays, rays_stride, bytes;
    constexpr FusedLds(int n_layers, int obl, int dz0)
        : rsl(obl * 32 + 8), WLt(0), W1t(WLt + 64 * rsl * 2), W0t(W1t + (n_layers == 3 ? W64 : 0)), W0s(W0t + W64), W1s(W0s + W64),
          b0(W1s + (n_layers == 3 ? W64 : 0)), b1(b0 + 64 * 4), Tx(b1 + 64 * 4), Th0(Tx + TW_BYTES), Th1(Th0 + (n_layers == 3 ? TW_BYTES : 0)), Tz(Th1 + TW_BYTES),
          tile_stride((n_layers + 1) * TW_BYTES), rays(Tx + 4 * tile_stride), rays_stride(64 * 4), bytes(rays + (dz0 == 2 ? 4 * rays_stride : 0)) {}
};
// mlp_bwd_pair: the images of FusedLds for .i (64-wide upper layer: [64][rslI]) and .s (output layer [64][rslS]), two layers each; per wave Tx | ThI | ThS | Tz
struct PairLds {
    int rslI = 72, rslS = 40, WLtI = 0, W0tI = WLtI + 64 * rslI * 2, W0sI = W0tI + W64, WLtS = W0sI + W64, W0tS = WLtS + 64 * rslS * 2, W0sS = W0tS + W64, b0I = W0sS + W64, b0S = b0I + 64 * 4,
        Tx = b0S + 64 * 4, ThI = Tx + TW_BYTES, ThS = ThI + TW_BYTES, Tz = ThS + TW_BYTES, tile_stride = 4 * TW_BYTES, bytes = Tx + 4 * tile_stride;
};
// mlp_bwd_wide_blocks<OB>: W_L both ways (WLt [64][rsl], WLs [ob*32][RS] permuted k), its bias, the activation ring Th [4][tile], the helper's transpose
// tile Tp, one dz tile per block wave (Tz + wave * Tz_stride), gradient rows grow [2][WB_RMAX][WR_RS] f32, partial dots dot [2][ob][64] f32,
// dz fragments zbuf [2][ob][2][64] x 16 B
struct WideBlocksLds {
    int rsl, WLt, WLs, bL, Th, Tp, Tz, Tz_stride, grow, dot, zbuf, bytes;
    constexpr WideBlocksLds(int ob)
        : rsl(ob * 32 + 8), WLt(0), WLs(WLt + 64 * rsl * 2), bL(WLs + ob * W32), Th(bL + ob * 32 * 4), Tp(Th + 4 * TW_BYTES), Tz(Tp + TW_BYTES), Tz_stride(TW_BYTES),
          grow(Tz + ob * Tz_stride), dot(grow + 2 * WB_RMAX * WR_RS * 4), zbuf(dot + 2 * ob * 64 * 4), bytes(zbuf + 2 * ob * 2 * 64 * 16) {}
};
// mlp_bwd_wide_mfma: W_L both ways, W_1^T (n_layers = 3), W_0^T, the last bias, per wave a staging tile and the tile's gradient row [ob*32] f32
struct WideMfmaLds {
    int rsl, WLt, WLs, W1t, W0t, bL, stg, stg_stride, grow, grow_stride, bytes;
    constexpr WideMfmaLds(int n_layers, int ob, int waves)
        : rsl(ob * 32 + 8), WLt(0), WLs(WLt + 64 * rsl * 2), W1t(WLs + ob * W32), W0t(W1t + (n_layers == 3 ? W64 : 0)), bL(W0t + W64), stg(bL + ob * 32 * 4),
          stg_stride(ST_BYTES), grow(stg + waves * stg_stride), grow_stride(ob * 32 * 4), bytes(grow + waves * grow_stride) {}
};
// head_composite_fwd_kernel: W_L [ob*32][RS] permuted k, its bias, the waves' partial ray sums red [4][ob*32] f32, staging tiles
struct HeadCompLds {
    int WL, bL, red, stg, stg_stride, bytes;
    constexpr HeadCompLds(int ob) : WL(0), bL(WL + ob * W32), red(bL + ob * 32 * 4), stg(red + 4 * ob * 32 * 4), stg_stride(ST_BYTES), bytes(stg + 4 * stg_stride) {}
};
// mlp_fwd_f32 / mlp_bwd_f32: the per-sample columns [rows][PT] f32 (64 activations / 224 dz) and the current weight chunk [64][64] f32
struct F32Lds {
    int cols, wt, bytes;
    constexpr F32Lds(int rows) : cols(0), wt(cols + rows * PT * 4), bytes(wt + 64 * 64 * 4) {}
};
// mlp_wgrad_kernel: the transposed dz tile Zt [ob*32][WG_RS] and input tile At [ib*32][WG_RS], bf16
struct WgradLds {
    int Zt, At, bytes;
    constexpr WgradLds(int ob, int ib) : Zt(0), At(Zt + ob * 32 * WG_RS * 2), bytes(At + ib * 32 * WG_RS * 2) {}
};

// the largest instance of every layout fits a workgroup
static_assert(FwdLds(3, OB_MAX, 16, true).bytes <= LDS_MAX_BYTES && FwdLds(3, OB_MAX, 4, true, true).bytes <= LDS_MAX_BYTES, "FwdLds");
static_assert(DensityColourLds{}.bytes <= LDS_MAX_BYTES, "DensityColourLds");
static_assert(BwdLds(3, OB_MAX).bytes <= LDS_MAX_BYTES, "BwdLds");
static_assert(FusedLds(3, 1, 2).bytes <= LDS_MAX_BYTES && FusedLds(2, 2, 0).bytes <= LDS_MAX_BYTES, "FusedLds");
static_assert(PairLds{}.bytes <= LDS_MAX_BYTES, "PairLds");
static_assert(WideBlocksLds(OB_MAX).bytes <= LDS_MAX_BYTES, "WideBlocksLds");
static_assert(WideMfmaLds(3, OB_MAX, WIDE_BWD_WAVES).bytes <= LDS_MAX_BYTES, "WideMfmaLds");
static_assert(HeadCompLds(OB_MAX).bytes <= LDS_MAX_BYTES, "HeadCompLds");
static_assert(F32Lds(224).bytes <= LDS_MAX_BYTES, "F32Lds");
static_assert(WgradLds(OB_MAX, 2).bytes <= LDS_MAX_BYTES, "WgradLds");

}  // namespace pagmlp
