// Dynamic-LDS layouts of the 128-wide decoder kernels in mlp_h128.hip (nothing else includes this), in the idiom of mlp_lds.h: ONE description per
// kernel serves the carve-up inside the kernel (lds_at<T>(smem, L.region)) and the byte count its launcher asks for (L.bytes).
// Constants and constexpr code only; WT is mlp_common.h's (pagmlp), which mlp_h128.hip includes first.  Every member is an offset in BYTES from the
// start of the dynamic segment.
#pragma once

namespace pagmlp128 {

constexpr int LDS_MAX_BYTES = 160 * 1024;       // gfx950: LDS per workgroup
constexpr int WH = 128;                         // hidden width
constexpr int K0 = 64;                          // layer-0 input positions (in_dim <= 64, zero padded)
constexpr int S128 = 136, S64 = 72;             // LDS row strides (bf16 elements): width + 16 B, an odd number of 16-B granules (ds_read_b128 conflict-free)
constexpr int MAX_HIDDEN = 3;                   // Linear + ReLU layers
constexpr int OB_MAX = 7;                       // 32-row blocks of the widest output layer (out_dim <= 224)
using pagmlp::WT;                               // mlp_common.h, included first: row stride of the weight-gradient kernel's transposed images

// h128_fwd_kernel: every layer's image is resident for the whole launch.  W0 [128][S64], W1 / W2 [128][S128] (n_hidden - 1 of them), WL [ob*32][S128],
// all with the input index permuted (swap23); then the f32 biases b0 .. b(n_hidden-1) [128] each and bL [ob*32]
struct FwdLds {
    int W0, Wh, WL, b, bL, bytes;
    constexpr FwdLds(int n_hidden, int ob)
        : W0(0), Wh(W0 + WH * S64 * 2), WL(Wh + (n_hidden - 1) * WH * S128 * 2), b(WL + ob * 32 * S128 * 2), bL(b + n_hidden * WH * 4), bytes(bL + ob * 32 * 4) {}
    constexpr int hidden_image(int l) const { return Wh + (l - 1) * WH * S128 * 2; }      // l = 1 .. n_hidden - 1
};
// h128_bwd_kernel: the transposed images.  WLt [128][rsl] (k = output channel, permuted), W1t / W2t [128][S128], W0t [64][S128]
struct BwdLds {
    int rsl, WLt, Wht, W0t, bytes;
    constexpr BwdLds(int n_hidden, int ob)
        : rsl(ob * 32 + 8), WLt(0), Wht(WLt + WH * rsl * 2), W0t(Wht + (n_hidden - 1) * WH * S128 * 2), bytes(W0t + K0 * S128 * 2) {}
    constexpr int hidden_image(int l) const { return Wht + (l - 1) * WH * S128 * 2; }
};
// h128_wgrad_kernel: the transposed dz tile zT [256][WT] (8 waves x 32 rows) and input tile aT [128][WT], bf16
struct WgradLds {
    int zT = 0, aT = zT + 256 * WT * 2, bytes = aT + WH * WT * 2;
};

static_assert(FwdLds(MAX_HIDDEN, OB_MAX).bytes <= LDS_MAX_BYTES, "FwdLds");
static_assert(BwdLds(MAX_HIDDEN, OB_MAX).bytes <= LDS_MAX_BYTES, "BwdLds");
static_assert(WgradLds{}.bytes <= 64 * 1024, "WgradLds");

}  // namespace pagmlp128
