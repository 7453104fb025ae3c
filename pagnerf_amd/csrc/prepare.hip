// View preparation of a NeRF-standard dataset (pagnerf_amd/formats.py; datasets/formats/nerf_standard.py:57-60 and :239-282, the nearest label resample
// of datasets/formats/bup20.py:203-229): decoded uint8 frames of a chunk in, the dataset's final float image, mask and world rays out, one launch.
//
// Thread (b, p) owns output pixel p = y * w + x of chunk view b, so that the lanes of a wave walk the contiguous output axis:
//   image   S_c = the integer sum of channel c over the f x f source block (f = 2^mip);  v_c = (float)S_c / (float)(255 f f), one IEEE division;
//           RGBA: a = v_3, mask = a > 0.5, white: clamp((v_c * a) + (1 - a), 0, 1), black: clamp(v_c - (1 - a), 0, 1) - three roundings in that order
//           (the file is built without FMA contraction);  RGB: v_c itself, mask true.  pagnerf_amd.formats.prepare_views_reference is the definition.
//   rays    origin = c2w[:, 3] (a copy);  d_cam = ((x + 0.5 - w/2 - x0) / fx, -(y + 0.5 - h/2 - y0) / fy, -1);  dir = normalise(R d_cam), R = c2w[:, :3]
// An RGBA pixel is read as one 32-bit word and the f words of a block row as 8- or 16-byte vectors where f and the base address allow (a block row starts
// at a multiple of 4 f bytes because W0 is a multiple of f); RGB and unaligned sources take the byte path.  Every output is written once, at view
// view_offset + b of a destination with [V, h, w, ...] strides.  No atomics, no LDS, no workspace.  Bytes moved per output pixel: 4 f f read (RGBA),
// 37 written (12 image, 1 mask, 12 origin, 12 direction).
// A variant with four consecutive pixels per thread, 16-byte loads and stores and the four mask bytes as one word was built and measured: it was 8 - 11 %
// SLOWER on 100 x 800 x 800 RGBA at mip 0 and 1 and is not here.
#include "common.h"

namespace {

struct PrepareViews {
    const unsigned char *src;
    const float *c2w;                  // [V, 3, 4]
    float *imgs, *origins, *dirs;      // [V, h, w, 3]
    unsigned char *masks;              // [V, h, w, 1]
    int64_t view_offset;
    int32_t H0, W0, h, w, f, bg;
    float half_w, half_h, fx, fy, x0, y0;
};

struct Float3 {
    float x, y, z;
};

// the block sums of one output pixel; VW = 32-bit words per load of an RGBA block row (1, 2 or 4), 0 = the byte path of C0 channels
template <int VW, int C0>
__device__ __forceinline__ void block_sums(const unsigned char *__restrict__ row0, int64_t row_bytes, int f, uint32_t (&S)[4]) {
    S[0] = S[1] = S[2] = S[3] = 0u;
    for (int dy = 0; dy < f; ++dy) {
        const unsigned char *r = row0 + dy * row_bytes;
        if constexpr (VW == 0) {
            for (int dx = 0; dx < f; ++dx)
#pragma unroll
                for (int c = 0; c < C0; ++c) S[c] += r[dx * C0 + c];
        } else {
            for (int dx = 0; dx < f; dx += VW) {
                uint32_t wds[VW];
                if constexpr (VW == 4) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(r + 4 * dx);
                    wds[0] = v.x, wds[1] = v.y, wds[2] = v.z, wds[3] = v.w;
                } else if constexpr (VW == 2) {
                    const uint2 v = *reinterpret_cast<const uint2 *>(r + 4 * dx);
                    wds[0] = v.x, wds[1] = v.y;
                } else {
                    wds[0] = *reinterpret_cast<const uint32_t *>(r + 4 * dx);
                }
#pragma unroll
                for (int i = 0; i < VW; ++i) {
                    S[0] += wds[i] & 0xffu;
                    S[1] += (wds[i] >> 8) & 0xffu;
                    S[2] += (wds[i] >> 16) & 0xffu;
                    S[3] += wds[i] >> 24;
                }
            }
        }
    }
}

// the colour of one output pixel from its block sums: the definition's op order
template <int C0>
__device__ __forceinline__ Float3 pixel_colour(const uint32_t (&S)[4], float den, int bg, bool &mask) {
    float r = (float)S[0] / den, g = (float)S[1] / den, bl = (float)S[2] / den;
    mask = true;
    if (C0 == 4) {
        const float al = (float)S[3] / den;
        const float rest = 1.0f - al;
        mask = al > 0.5f;
        if (bg == PAG_BG_WHITE) {
            r = r * al + rest;
            g = g * al + rest;
            bl = bl * al + rest;
        } else {
            r = r - rest;
            g = g - rest;
            bl = bl - rest;
        }
        r = fminf(fmaxf(r, 0.0f), 1.0f);
        g = fminf(fmaxf(g, 0.0f), 1.0f);
        bl = fminf(fmaxf(bl, 0.0f), 1.0f);
    }
    return Float3{r, g, bl};
}

// the world direction of pixel (x, y) of the view with camera-to-world rows m[0..11]
__device__ __forceinline__ Float3 pixel_dir(const float *__restrict__ m, int x, int y, const PrepareViews &a) {
    const float dx = (((float)x + 0.5f) - a.half_w - a.x0) / a.fx;
    const float dy = -((((float)y + 0.5f) - a.half_h - a.y0) / a.fy);
    const float wx = (m[0] * dx + m[1] * dy) - m[2];            // R d_cam with d_cam.z = -1
    const float wy = (m[4] * dx + m[5] * dy) - m[6];
    const float wz = (m[8] * dx + m[9] * dy) - m[10];
    const float len = sqrtf((wx * wx + wy * wy) + wz * wz);     // >= |d_cam| (1 - eps) >= 1 for a rotation: never 0
    return Float3{wx / len, wy / len, wz / len};
}

template <int VW, int C0>
__global__ __launch_bounds__(256) void prepare_views_kernel(PrepareViews a) {
    const int64_t n = (int64_t)a.h * a.w;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int b = blockIdx.y;
    const int y = (int)(p / a.w), x = (int)(p - (int64_t)y * a.w);
    const int64_t out = (a.view_offset + b) * n + p;                    // 64-bit: V * h * w * 3 passes 2^31 for a real dataset
    if (a.imgs || a.masks) {
        const int64_t row_bytes = (int64_t)a.W0 * C0;
        const unsigned char *row0 = a.src + ((int64_t)b * a.H0 + (int64_t)y * a.f) * row_bytes + (int64_t)x * a.f * C0;
        uint32_t S[4];
        block_sums<VW, C0>(row0, row_bytes, a.f, S);
        bool mask;
        const Float3 c = pixel_colour<C0>(S, (float)(255 * a.f * a.f), a.bg, mask);      // 255 f f <= 255 * 2^16 < 2^24: exact, as is every S
        if (a.imgs) *reinterpret_cast<Float3 *>(a.imgs + out * 3) = c;
        if (a.masks) a.masks[out] = mask ? 1 : 0;
    }
    if (a.origins || a.dirs) {
        const float *m = a.c2w + (a.view_offset + b) * 12;              // wave-uniform: twelve scalar loads
        if (a.origins) *reinterpret_cast<Float3 *>(a.origins + out * 3) = Float3{m[3], m[7], m[11]};
        if (a.dirs) *reinterpret_cast<Float3 *>(a.dirs + out * 3) = pixel_dir(m, x, y, a);
    }
}

struct LabelPlanes {
    const unsigned char *src[PAG_PREPARE_MAX_PLANES];
    int64_t *dst[PAG_PREPARE_MAX_PLANES];
};

__global__ __launch_bounds__(256) void prepare_labels_kernel(LabelPlanes planes, int H0, int W0, int h, int w, int f, int64_t view_offset) {
    const int64_t n = (int64_t)h * w;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int b = blockIdx.y, k = blockIdx.z;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    const unsigned char *s = planes.src[k] + ((int64_t)b * H0 + (int64_t)y * f) * W0 + (int64_t)x * f;
    planes.dst[k][(view_offset + b) * n + p] = (int64_t)*s;
}

// the sizes both entry points share: -> PAG_OK with h, w, f set
int check_sizes(const char *who, int B, int H0, int W0, int mip, int64_t view_offset, int64_t V, int *h, int *w, int *f) {
    PAG_CHECK_ARG(mip >= 0 && mip <= 8, "%s: mip %d not in [0,8]", who, mip);
    PAG_CHECK_ARG(B >= 0 && B <= 65535, "%s: B %d not in [0,65535]", who, B);
    PAG_CHECK_ARG(H0 >= 1 && W0 >= 1, "%s: source size %d x %d < 1", who, H0, W0);
    *f = 1 << mip;
    PAG_CHECK_ARG(H0 % *f == 0 && W0 % *f == 0, "%s: source size %d x %d is not divisible by 2^mip = %d", who, H0, W0, *f);
    *h = H0 / *f;
    *w = W0 / *f;
    PAG_CHECK_ARG((int64_t)*h * *w <= ((int64_t)1 << 30), "%s: %lld output pixels per view, more than 2^30", who, (long long)*h * *w);
    PAG_CHECK_ARG(view_offset >= 0 && V >= 1 && view_offset + B <= V, "%s: views [%lld, %lld) outside the destination's [0, %lld)", who, (long long)view_offset,
                  (long long)(view_offset + B), (long long)V);
    return PAG_OK;
}

}  // namespace

extern "C" int pag_prepare_views(const void *src, int B, int H0, int W0, int C0, int mip, int bg, const float *c2w, float fx, float fy, float x0, float y0,
                                 int64_t view_offset, int64_t V, float *imgs, unsigned char *masks, float *origins, float *dirs, void *stream) {
    int h, w, f;
    const int rc = check_sizes("pag_prepare_views", B, H0, W0, mip, view_offset, V, &h, &w, &f);
    if (rc != PAG_OK) return rc;
    PAG_CHECK_ARG(C0 == 3 || C0 == 4, "pag_prepare_views: C0 %d is neither 3 nor 4", C0);
    PAG_CHECK_ARG(bg == PAG_BG_BLACK || bg == PAG_BG_WHITE, "pag_prepare_views: background code %d", bg);
    const bool pixels = imgs || masks, rays = origins || dirs;
    if (B == 0 || !(pixels || rays)) return PAG_OK;
    PAG_CHECK_ARG(!pixels || src, "pag_prepare_views: NULL src");
    PAG_CHECK_ARG(!rays || c2w, "pag_prepare_views: NULL c2w");
    PAG_CHECK_ARG(!dirs || (fx != 0.0f && fy != 0.0f && fx == fx && fy == fy), "pag_prepare_views: focal lengths %g, %g", (double)fx, (double)fy);
    PrepareViews a = {};
    a.src = static_cast<const unsigned char *>(src);
    a.c2w = c2w;
    a.imgs = imgs, a.masks = masks, a.origins = origins, a.dirs = dirs;
    a.view_offset = view_offset;
    a.H0 = H0, a.W0 = W0, a.h = h, a.w = w, a.f = f, a.bg = bg;
    a.half_w = 0.5f * (float)w, a.half_h = 0.5f * (float)h;
    a.fx = fx, a.fy = fy, a.x0 = x0, a.y0 = y0;
    const dim3 grid((unsigned)(((int64_t)h * w + 255) / 256), (unsigned)B), block(256);
    hipStream_t s = (hipStream_t)stream;
    // words per load of a block row: the widest of 4 / 2 / 1 that divides f and whose bytes divide the base address (rows are 4 W0 bytes, W0 = w f)
    const uintptr_t addr = (uintptr_t)src;
    if (C0 == 3) {
        hipLaunchKernelGGL((prepare_views_kernel<0, 3>), grid, block, 0, s, a);
    } else if (!pixels || (addr & 3)) {
        hipLaunchKernelGGL((prepare_views_kernel<0, 4>), grid, block, 0, s, a);
    } else if (f % 4 == 0 && (addr & 15) == 0) {
        hipLaunchKernelGGL((prepare_views_kernel<4, 4>), grid, block, 0, s, a);
    } else if (f % 2 == 0 && (addr & 7) == 0) {
        hipLaunchKernelGGL((prepare_views_kernel<2, 4>), grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((prepare_views_kernel<1, 4>), grid, block, 0, s, a);
    }
    PAG_CHECK_LAUNCH("pag_prepare_views");
    return PAG_OK;
}

extern "C" int pag_prepare_labels(const pag_label_plane *planes, int n_planes, int B, int H0, int W0, int mip, int64_t view_offset, int64_t V, void *stream) {
    int h, w, f;
    const int rc = check_sizes("pag_prepare_labels", B, H0, W0, mip, view_offset, V, &h, &w, &f);
    if (rc != PAG_OK) return rc;
    PAG_CHECK_ARG(n_planes >= 0 && n_planes <= PAG_PREPARE_MAX_PLANES, "pag_prepare_labels: n_planes %d not in [0,%d]", n_planes, PAG_PREPARE_MAX_PLANES);
    PAG_CHECK_ARG(n_planes == 0 || planes, "pag_prepare_labels: NULL planes");
    LabelPlanes k = {};
    for (int i = 0; i < n_planes; ++i) {
        PAG_CHECK_ARG(planes[i].src && planes[i].dst, "pag_prepare_labels: plane %d: NULL src / dst", i);
        k.src[i] = static_cast<const unsigned char *>(planes[i].src);
        k.dst[i] = planes[i].dst;
    }
    if (B == 0 || n_planes == 0) return PAG_OK;
    hipLaunchKernelGGL(prepare_labels_kernel, dim3((unsigned)(((int64_t)h * w + 255) / 256), (unsigned)B, (unsigned)n_planes), dim3(256), 0, (hipStream_t)stream, k,
                       H0, W0, h, w, f, view_offset);
    PAG_CHECK_LAUNCH("pag_prepare_labels");
    return PAG_OK;
}
