// Host-side image preparation and depth read-out of the raw model's infer_image, on the device (reference RAW/dpt.py:186-221,
// RAW/util/transform.py:5-158).  The reference prepares a decoded photo with OpenCV on the host: BGR -> RGB, / 255 (float64),
// cv2.resize INTER_CUBIC to the network size, ImageNet normalisation; after the forward it resizes the depth map back to the photo
// with F.interpolate(bilinear, align_corners=True).  Neither kernel is on the benchmark path: each is one memory-bound pass.
// The second half of the file is the host preparation of the two-model infer.py on the device (reference infer.py:17-18, 77, 83-91, 113): the
// photo resized twice (cv2's 8-bit INTER_LINEAR for the base network, ATen's nearest for the amodal one) in one pass, the amodal masks, and the
// cv2 INTER_NEAREST resize of a result back to the photo.  Same launch shape, same rule: one thread per output pixel, no scratch.
// The last kernel is the rendering of infer.py:106-119 (colour map, highlight_target, the nearest resize to the photo's size, the channel flip) in one
// pass over the output grid: uint8 pixels out, optionally the 16-bit map beside them.
#include "ada_common.h"

namespace {

// cv2's interpolateCubic (imgproc/src/resize.cpp), A = -0.75, in fp32 with every operation rounded on its own as in the host build
// (no contraction into FMAs): the coefficients are bit-identical to OpenCV's.
ADA_DEV void cubic_coeffs(float x, float c[4]) {
#pragma clang fp contract(off)
    const float A = -0.75f;
    c[0] = ((A * (x + 1.f) - 5.f * A) * (x + 1.f) + 8.f * A) * (x + 1.f) - 4.f * A;
    c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    c[2] = ((A + 2.f) * (1.f - x) - (A + 3.f)) * (1.f - x) * (1.f - x) + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// source position of output pixel d as cv2.resize computes it: fx = (float)((d + 0.5) * scale - 0.5) in double, sx = floor(fx), fx -= sx.
// Cubic keeps fx at the borders; the taps sx - 1 .. sx + 2 are clamped to the image (replicate) by the caller.
ADA_DEV int cubic_src(int d, double scale, float& frac) {
#pragma clang fp contract(off)
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const int s = (int)__builtin_floorf(f);
    frac = f - (float)s;
    return s;
}

ADA_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct PrepArgs {
    const uint8_t* src;
    long pitch, istride;     // bytes between rows / images
    int hi, wi, cn;          // cn = 3 (BGR) or 4 (BGRA, alpha ignored)
    int ho, wo;
    double sy, sx;           // 1 / ((double)ho / hi), 1 / ((double)wo / wi): cv2's scale_y / scale_x
    float mean[3], stdv[3];  // RGB order
    float* out;              // [B, 3, ho, wo]
};

// block (64, 4): one output pixel per thread, all three channels.  A wave covers 64 consecutive x of one output row, so the four source rows
// of its vertical taps are shared and each of the three plane stores is one contiguous 256-byte segment.  The 4 x 4 taps are byte gathers
// through the caches (the photo is read about once: its rows are visited by at most ~4 / scale output rows each).
__global__ __launch_bounds__(256) void image_prep_kernel(PrepArgs a) {
    const int dx = blockIdx.x * 64 + threadIdx.x;
    const int dy = blockIdx.y * 4 + threadIdx.y;
    const int b = blockIdx.z;
    if (dx >= a.wo || dy >= a.ho) return;
    float fx, fy, cx[4], cy[4];
    const int sx = cubic_src(dx, a.sx, fx);
    const int sy = cubic_src(dy, a.sy, fy);
    cubic_coeffs(fx, cx);
    cubic_coeffs(fy, cy);
    long xo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xo[j] = (long)clampi(sx - 1 + j, 0, a.wi - 1) * a.cn;
    const uint8_t* img = a.src + (long)b * a.istride;
    // horizontal pass on each of the four source rows, then the vertical pass (cv2's order); u8 / 255 is applied last -- the sums are linear
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint8_t* row = img + (long)clampi(sy - 1 + k, 0, a.hi - 1) * a.pitch;
        float h[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int c = 0; c < 3; ++c) h[c] += (float)row[xo[j] + 2 - c] * cx[j];   // byte 2 - c of a BGR(A) pixel is RGB channel c
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += h[c] * cy[k];
    }
    const long plane = (long)a.ho * a.wo;
    float* o = a.out + (long)b * 3 * plane + (long)dy * a.wo + dx;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = (acc[c] * (1.f / 255.f) - a.mean[c]) / a.stdv[c];   // not clamped: cubic overshoots at edges, as cv2's float path does
}

struct DepthResizeArgs {
    const float* in;
    float* out;
    int hi, wi, ho, wo;
    float ry, rx;            // (in - 1) / (out - 1), 0 when out == 1
};

// ATen's upsample_bilinear2d (align_corners=True) on one channel: src = r * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), lambda = src - i0,
// out = h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11).  Block (64, 4), one output pixel per thread: stores are coalesced along x.
__global__ __launch_bounds__(256) void depth_resize_kernel(DepthResizeArgs a) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    const int b = blockIdx.z;
    if (x >= a.wo || y >= a.ho) return;
    const float syf = a.ry * (float)y, sxf = a.rx * (float)x;
    const int y0 = (int)syf, x0 = (int)sxf;
    const int y1 = y0 + (y0 < a.hi - 1 ? 1 : 0), x1 = x0 + (x0 < a.wi - 1 ? 1 : 0);
    const float h1 = syf - (float)y0, h0 = 1.f - h1;
    const float w1 = sxf - (float)x0, w0 = 1.f - w1;
    const float* p = a.in + (long)b * a.hi * a.wi;
    const float* r0 = p + (long)y0 * a.wi;
    const float* r1 = p + (long)y1 * a.wi;
    a.out[((long)b * a.ho + y) * a.wo + x] = h0 * (w0 * r0[x0] + w1 * r0[x1]) + h1 * (w0 * r1[x0] + w1 * r1[x1]);
}

// One axis of cv2.resize's 8-bit INTER_LINEAR (imgproc/src/resize.cpp, resizeGeneric_ with HResizeLinear / VResizeLinear<uchar, int, short>):
// fx = (float)((d + 0.5) * scale - 0.5) in double, s = floor(fx), fx -= s; at the borders the tap is pinned and fx = 0; the two coefficients are
// shorts on an 11-bit scale, cvRound (half to even) of the fp32 products.  Returns s; the second tap is min(s + 1, n_in - 1).
ADA_DEV int linear_src(int d, double scale, int n_in, int& a0, int& a1) {
#pragma clang fp contract(off)
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)__builtin_floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_in - 1) { s = n_in - 1; f = 0.f; }
    a0 = (int)__builtin_rintf((1.f - f) * 2048.f);
    a1 = (int)__builtin_rintf(f * 2048.f);
    return s;
}

// ATen's nearest rule (UpSample.h nearest_idx): scale = (float)n_in / n_out, src = min((int)floorf(dst * scale), n_in - 1), all in fp32
ADA_DEV int aten_nearest(int d, float scale, int n_in) {
    const int s = (int)__builtin_floorf((float)d * scale);
    return s < n_in - 1 ? s : n_in - 1;
}

struct PhotoArgs {
    const uint8_t* src;
    long pitch;              // bytes between rows
    int hi, wi, cn;          // cn = 3 (BGR) or 4 (BGRA, alpha ignored)
    int ho, wo;
    double sy, sx;           // 1 / ((double)ho / hi), 1 / ((double)wo / wi): cv2's scale_y / scale_x
    float ny, nx;            // (float)hi / ho, (float)wi / wo: ATen's nearest scales
    int area;                // hi == 2 ho && wi == 2 wo: cv2 turns INTER_LINEAR into the 2 x 2 area mean
    float* raw;              // [3, ho, wo] or NULL
    float* near;             // [3, ho, wo] or NULL
};

// block (64, 4) as image_prep_kernel: one output pixel per thread, the three channels of both planes; a wave covers 64 consecutive x of one
// output row, so it shares its two source rows and each plane store is one contiguous 256-byte segment.  The channel order of the source
// is KEPT (plane c = byte c of a pixel): the reference feeds B, G, R planes to both networks on this path (infer.py:17-18, 83).
// v / 255.f is IEEE division (the build does not relax it): the correctly rounded quotient torch computes for `tensor / 255`.
__global__ __launch_bounds__(256) void photo_prep_kernel(PhotoArgs a) {
    const int dx = blockIdx.x * 64 + threadIdx.x;
    const int dy = blockIdx.y * 4 + threadIdx.y;
    if (dx >= a.wo || dy >= a.ho) return;
    const long plane = (long)a.ho * a.wo;
    const long o = (long)dy * a.wo + dx;
    if (a.raw) {
        int v[3];
        if (a.area) {
            const uint8_t* r0 = a.src + (long)(2 * dy) * a.pitch + (long)(2 * dx) * a.cn;
            const uint8_t* r1 = r0 + a.pitch;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = ((int)r0[c] + (int)r0[a.cn + c] + (int)r1[c] + (int)r1[a.cn + c] + 2) >> 2;
        } else {
            int ax0, ax1, ay0, ay1;
            const int x0 = linear_src(dx, a.sx, a.wi, ax0, ax1);
            const int y0 = linear_src(dy, a.sy, a.hi, ay0, ay1);
            const int x1 = x0 + 1 < a.wi ? x0 + 1 : a.wi - 1;
            const int y1 = y0 + 1 < a.hi ? y0 + 1 : a.hi - 1;
            const uint8_t* r0 = a.src + (long)y0 * a.pitch;
            const uint8_t* r1 = a.src + (long)y1 * a.pitch;
            const long o0 = (long)x0 * a.cn, o1 = (long)x1 * a.cn;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // horizontal pass on the two source rows, then cv2's vertical pass with its intermediate shifts; all int32:
                // 255 * 2048 >> 4 = 32640 and 32640 * 2048 < 2^31
                const int h0 = (int)r0[o0 + c] * ax0 + (int)r0[o1 + c] * ax1;
                const int h1 = (int)r1[o0 + c] * ax0 + (int)r1[o1 + c] * ax1;
                const int t = (((ay0 * (h0 >> 4)) >> 16) + ((ay1 * (h1 >> 4)) >> 16) + 2) >> 2;
                v[c] = t > 255 ? 255 : t;   // saturate_cast<uchar>; never negative
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) a.raw[c * plane + o] = (float)v[c] / 255.f;
    }
    if (a.near) {
        const uint8_t* p = a.src + (long)aten_nearest(dy, a.ny, a.hi) * a.pitch + (long)aten_nearest(dx, a.nx, a.wi) * a.cn;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.near[c * plane + o] = (float)p[c] / 255.f;
    }
}

struct MaskArgs {
    const uint8_t* src;
    long pitch, istride;     // bytes between rows / masks
    int hi, wi, ho, wo;
    float ny, nx;            // ATen's nearest scales
    float* out01;            // [K, 1, ho, wo]
    float* out_pm1;          // [K, 1, ho, wo] or NULL
};

// block (64, 4), grid z = mask: m = src != 0 at ATen's nearest source pixel; out01 = m, out_pm1 = 2 m - 1
__global__ __launch_bounds__(256) void mask_prep_kernel(MaskArgs a) {
    const int dx = blockIdx.x * 64 + threadIdx.x;
    const int dy = blockIdx.y * 4 + threadIdx.y;
    const int k = blockIdx.z;
    if (dx >= a.wo || dy >= a.ho) return;
    const uint8_t s = a.src[(long)k * a.istride + (long)aten_nearest(dy, a.ny, a.hi) * a.pitch + aten_nearest(dx, a.nx, a.wi)];
    const long o = ((long)k * a.ho + dy) * a.wo + dx;
    a.out01[o] = s ? 1.f : 0.f;
    if (a.out_pm1) a.out_pm1[o] = s ? 1.f : -1.f;
}

struct NearestArgs {
    const float* in;
    float* out;
    int hi, wi, ho, wo;
    double ify, ifx;         // 1 / ((double)ho / hi), 1 / ((double)wo / wi)
};

// cv2.resize(INTER_NEAREST)'s source index (resizeNN): min((int)floor(d * inv), n_in - 1) in double, inv = 1 / ((double)n_out / n_in)
ADA_DEV int cv2_nearest_src(int d, double inv, int n_in) {
    const int s = (int)__builtin_floor((double)d * inv);
    return s < n_in - 1 ? s : n_in - 1;
}

// cv2.resize(INTER_NEAREST): cv2_nearest_src on both axes.  Block (64, 4), grid z = image.
__global__ __launch_bounds__(256) void nearest_resize_kernel(NearestArgs a) {
    const int dx = blockIdx.x * 64 + threadIdx.x;
    const int dy = blockIdx.y * 4 + threadIdx.y;
    const int b = blockIdx.z;
    if (dx >= a.wo || dy >= a.ho) return;
    const int sx = cv2_nearest_src(dx, a.ifx, a.wi);
    const int sy = cv2_nearest_src(dy, a.ify, a.hi);
    a.out[((long)b * a.ho + dy) * a.wo + dx] = a.in[((long)b * a.hi + sy) * a.wi + sx];
}

struct RenderArgs {
    const float* depth;      // [B, hi, wi]
    const float* minmax;     // [B, 2] or NULL
    const uint8_t* lut;      // [256][3], R, G, B
    const float* mask;       // [B, hi, wi] or NULL
    uint8_t* out;            // [B, ho, wo, 3] or NULL
    uint16_t* out_u16;       // [B, ho, wo] or NULL
    int hi, wi, ho, wo;
    double ify, ifx;         // 1 / ((double)ho / hi), 1 / ((double)wo / wi)
    float lo, span;          // used when minmax == NULL
    double keep, fg;         // 1.0 - alpha, alpha * 200.0
    int overlay;             // mask != NULL && alpha != 0
    int radius;              // thickness - 1
    uint32_t outline;        // packed as a pixel below
    int bgr;
};

// a pixel in a register: R | G << 8 | B << 16, the order of the bytes in memory
ADA_DEV uint32_t pack_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

// highlight_target's overlay of one byte (infer.py:50): (uint8)((1 - alpha) * c + alpha * 200) in double, both products rounded before the sum
ADA_DEV uint32_t overlay_byte(uint32_t c, double keep, double fg) {
#pragma clang fp contract(off)
    return (uint32_t)(keep * (double)c + fg);
}

ADA_DEV bool inside(float m) { return m > 0.f; }

// draw_mask_outline's edge: an inside pixel with a 4-neighbour outside; neighbours past the image take the border pixel's value
ADA_DEV bool mask_edge(const float* m, int v, int u, int hi, int wi) {
    const float* row = m + (long)v * wi;
    if (!inside(row[u])) return false;
    const float* up = m + (long)(v > 0 ? v - 1 : 0) * wi;
    const float* dn = m + (long)(v < hi - 1 ? v + 1 : hi - 1) * wi;
    return !(inside(up[u]) && inside(dn[u]) && inside(row[u > 0 ? u - 1 : 0]) && inside(row[u < wi - 1 ? u + 1 : wi - 1]));
}

// ... dilated thickness - 1 times with a zero-padded cross: some in-image edge pixel within L1 distance `radius`
ADA_DEV bool near_edge(const float* m, int sy, int sx, int hi, int wi, int radius) {
    for (int dv = -radius; dv <= radius; ++dv) {
        const int v = sy + dv;
        if (v < 0 || v >= hi) continue;
        const int w = radius - (dv < 0 ? -dv : dv);
        const int u0 = sx - w > 0 ? sx - w : 0, u1 = sx + w < wi - 1 ? sx + w : wi - 1;
        for (int u = u0; u <= u1; ++u)
            if (mask_edge(m, v, u, hi, wi)) return true;
    }
    return false;
}

// Block (64, 4), grid z = image; a thread renders PPT consecutive pixels of one output row.  PPT = 1 stores three bytes (and one u16) per thread and
// takes any width and any pointer; PPT = 4 stores the twelve bytes of its four pixels as three dwords (and the four u16 as two), which needs
// wo % 4 == 0 and aligned pointers (the launcher picks).  Everything but the store is a function of the SOURCE pixel -- nearest resize is a pure
// gather, so rendering what was gathered is the reference's render-then-resize -- and neighbouring outputs of an up-sampling share it: a pixel
// whose source column is its left neighbour's reuses that result.  The colour table sits in LDS twice, plain and with the overlay applied
// (the overlay acts on table colours only: the outline is painted over it), so the double arithmetic is done 768 times per block, not per pixel.
template <int PPT>
__global__ __launch_bounds__(256) void depth_render_kernel(RenderArgs a) {
    __shared__ uint32_t lut[2][256];
    {
        const int i = threadIdx.y * 64 + threadIdx.x;
        const uint32_t r = a.lut[3 * i], g = a.lut[3 * i + 1], b = a.lut[3 * i + 2];
        lut[0][i] = pack_rgb(r, g, b);
        lut[1][i] = a.overlay ? pack_rgb(overlay_byte(r, a.keep, a.fg), overlay_byte(g, a.keep, a.fg), overlay_byte(b, a.keep, a.fg)) : pack_rgb(r, g, b);
    }
    __syncthreads();
    const int dx0 = (blockIdx.x * 64 + threadIdx.x) * PPT;
    const int dy = blockIdx.y * 4 + threadIdx.y;
    const int b = blockIdx.z;
    if (dx0 >= a.wo || dy >= a.ho) return;
    float lo = a.lo, span = a.span;
    if (a.minmax) {
        lo = a.minmax[2 * b];
        span = a.minmax[2 * b + 1] - lo;
    }
    const uint32_t nan_ov = a.overlay ? overlay_byte(0, a.keep, a.fg) * 0x010101u : 0u;   // a NaN pixel is black before the overlay
    const int sy = cv2_nearest_src(dy, a.ify, a.hi);
    const float* drow = a.depth + ((long)b * a.hi + sy) * a.wi;
    const float* mimg = a.mask ? a.mask + (long)b * a.hi * a.wi : nullptr;
    uint32_t px[PPT], t16[PPT];
    int prev = -1;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int sx = cv2_nearest_src(dx0 + j, a.ifx, a.wi);
        if (j > 0 && sx == prev) {
            px[j] = px[j - 1];
            t16[j] = t16[j - 1];
            continue;
        }
        prev = sx;
        float t = (drow[sx] - lo) / span;          // two roundings, IEEE division: numpy's (d - lo) / span
        t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);   // np.clip: NaN passes through
        const bool nan = t != t;
        int idx = nan ? 0 : (int)(t * 256.f);
        idx = idx < 255 ? idx : 255;
        bool ov = false, paint = false;
        if (mimg) {
            ov = mimg[(long)sy * a.wi + sx] == 0.f;
            paint = near_edge(mimg, sy, sx, a.hi, a.wi, a.radius);
        }
        uint32_t c = nan ? (ov ? nan_ov : 0u) : lut[ov ? 1 : 0][idx];
        if (paint) c = a.outline;
        if (a.bgr) c = (c & 0x00ff00u) | (c >> 16) | ((c & 0xffu) << 16);
        px[j] = c;
        t16[j] = nan ? 0u : (uint32_t)(t * 65535.f);
    }
    const long o = ((long)b * a.ho + dy) * a.wo + dx0;
    if (PPT == 1) {
        if (a.out) {
            uint8_t* p = a.out + o * 3;
            p[0] = (uint8_t)px[0];
            p[1] = (uint8_t)(px[0] >> 8);
            p[2] = (uint8_t)(px[0] >> 16);
        }
        if (a.out_u16) a.out_u16[o] = (uint16_t)t16[0];
    } else {
        if (a.out) {
            uint32_t* p = reinterpret_cast<uint32_t*>(a.out + o * 3);      // o % 4 == 0: 12-byte steps from an aligned base
            p[0] = px[0] | (px[PPT > 1 ? 1 : 0] << 24);
            p[1] = (px[PPT > 1 ? 1 : 0] >> 8) | (px[PPT > 2 ? 2 : 0] << 16);
            p[2] = (px[PPT > 2 ? 2 : 0] >> 16) | (px[PPT > 3 ? 3 : 0] << 8);
        }
        if (a.out_u16) {
            uint32_t* q = reinterpret_cast<uint32_t*>(a.out_u16 + o);
            q[0] = t16[0] | (t16[PPT > 1 ? 1 : 0] << 16);
            q[1] = t16[PPT > 2 ? 2 : 0] | (t16[PPT > 3 ? 3 : 0] << 16);
        }
    }
}

}  // namespace

extern "C" int ada_image_prep_fwd(const uint8_t* src, int32_t batch, int32_t hi, int32_t wi, int32_t channels, int64_t row_pitch_bytes,
                                  int64_t image_stride_bytes, int32_t ho, int32_t wo, const float* mean, const float* std, float* out,
                                  void* stream) {
    ADA_REQUIRE(src && mean && std && out, ADA_EINVAL, "ada_image_prep_fwd: null pointer");
    ADA_REQUIRE(batch > 0 && hi > 0 && wi > 0 && ho > 0 && wo > 0, ADA_EINVAL, "ada_image_prep_fwd: bad shape batch=%d %dx%d -> %dx%d", batch, hi, wi, ho, wo);
    ADA_REQUIRE(channels == 3 || channels == 4, ADA_EINVAL, "ada_image_prep_fwd: %d channels (3 = BGR, 4 = BGRA)", channels);
    ADA_REQUIRE(row_pitch_bytes >= (int64_t)wi * channels, ADA_EINVAL, "ada_image_prep_fwd: row pitch %ld < %d pixels x %d bytes", (long)row_pitch_bytes, wi, channels);
    ADA_REQUIRE(batch == 1 || image_stride_bytes >= (int64_t)(hi - 1) * row_pitch_bytes + (int64_t)wi * channels, ADA_EINVAL,
                "ada_image_prep_fwd: image stride %ld overlaps the previous image", (long)image_stride_bytes);
    ADA_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, ADA_EINVAL, "ada_image_prep_fwd: zero std");
    ADA_REQUIRE((ho + 3) / 4 <= 65535 && batch <= 65535, ADA_EUNSUPPORTED, "ada_image_prep_fwd: ho / batch exceed the grid limits");
    PrepArgs a;
    a.src = src; a.pitch = row_pitch_bytes; a.istride = image_stride_bytes;
    a.hi = hi; a.wi = wi; a.cn = channels; a.ho = ho; a.wo = wo;
    a.sy = 1.0 / ((double)ho / hi);
    a.sx = 1.0 / ((double)wo / wi);
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.stdv[c] = std[c]; }   // host pointers
    a.out = out;
    hipLaunchKernelGGL(image_prep_kernel, dim3((unsigned)((wo + 63) / 64), (unsigned)((ho + 3) / 4), (unsigned)batch), dim3(64, 4), 0,
                       (hipStream_t)stream, a);
    return ada_check_launch("ada_image_prep_fwd");
}

extern "C" int ada_depth_resize_fwd(const float* in, int32_t batch, int32_t hi, int32_t wi, int32_t ho, int32_t wo, float* out, void* stream) {
    ADA_REQUIRE(in && out, ADA_EINVAL, "ada_depth_resize_fwd: null pointer");
    ADA_REQUIRE(batch > 0 && hi > 0 && wi > 0 && ho > 0 && wo > 0, ADA_EINVAL, "ada_depth_resize_fwd: bad shape batch=%d %dx%d -> %dx%d", batch, hi, wi, ho, wo);
    ADA_REQUIRE((ho + 3) / 4 <= 65535 && batch <= 65535, ADA_EUNSUPPORTED, "ada_depth_resize_fwd: ho / batch exceed the grid limits");
    DepthResizeArgs a;
    a.in = in; a.out = out; a.hi = hi; a.wi = wi; a.ho = ho; a.wo = wo;
    a.ry = ho > 1 ? (float)(hi - 1) / (float)(ho - 1) : 0.0f;
    a.rx = wo > 1 ? (float)(wi - 1) / (float)(wo - 1) : 0.0f;
    hipLaunchKernelGGL(depth_resize_kernel, dim3((unsigned)((wo + 63) / 64), (unsigned)((ho + 3) / 4), (unsigned)batch), dim3(64, 4), 0,
                       (hipStream_t)stream, a);
    return ada_check_launch("ada_depth_resize_fwd");
}

extern "C" int ada_photo_prep_fwd(const uint8_t* src, int32_t hi, int32_t wi, int32_t channels, int64_t row_pitch_bytes, int32_t ho, int32_t wo,
                                  float* raw_out, float* near_out, void* stream) {
    ADA_REQUIRE(src && (raw_out || near_out), ADA_EINVAL, "ada_photo_prep_fwd: null pointer");
    ADA_REQUIRE(hi > 0 && wi > 0 && ho > 0 && wo > 0, ADA_EINVAL, "ada_photo_prep_fwd: bad shape %dx%d -> %dx%d", hi, wi, ho, wo);
    ADA_REQUIRE(channels == 3 || channels == 4, ADA_EINVAL, "ada_photo_prep_fwd: %d channels (3 = BGR, 4 = BGRA)", channels);
    ADA_REQUIRE(row_pitch_bytes >= (int64_t)wi * channels, ADA_EINVAL, "ada_photo_prep_fwd: row pitch %ld < %d pixels x %d bytes", (long)row_pitch_bytes, wi, channels);
    ADA_REQUIRE((ho + 3) / 4 <= 65535, ADA_EUNSUPPORTED, "ada_photo_prep_fwd: ho exceeds the grid limit");
    PhotoArgs a;
    a.src = src; a.pitch = row_pitch_bytes;
    a.hi = hi; a.wi = wi; a.cn = channels; a.ho = ho; a.wo = wo;
    a.sy = 1.0 / ((double)ho / hi);
    a.sx = 1.0 / ((double)wo / wi);
    a.ny = (float)hi / (float)ho;
    a.nx = (float)wi / (float)wo;
    a.area = (hi == 2 * ho && wi == 2 * wo) ? 1 : 0;
    a.raw = raw_out; a.near = near_out;
    hipLaunchKernelGGL(photo_prep_kernel, dim3((unsigned)((wo + 63) / 64), (unsigned)((ho + 3) / 4), 1), dim3(64, 4), 0, (hipStream_t)stream, a);
    return ada_check_launch("ada_photo_prep_fwd");
}

extern "C" int ada_mask_prep_fwd(const uint8_t* src, int32_t batch, int32_t hi, int32_t wi, int64_t row_pitch_bytes, int64_t image_stride_bytes,
                                 int32_t ho, int32_t wo, float* out01, float* out_pm1, void* stream) {
    ADA_REQUIRE(src && out01, ADA_EINVAL, "ada_mask_prep_fwd: null pointer");
    ADA_REQUIRE(batch > 0 && hi > 0 && wi > 0 && ho > 0 && wo > 0, ADA_EINVAL, "ada_mask_prep_fwd: bad shape batch=%d %dx%d -> %dx%d", batch, hi, wi, ho, wo);
    ADA_REQUIRE(row_pitch_bytes >= (int64_t)wi, ADA_EINVAL, "ada_mask_prep_fwd: row pitch %ld < %d pixels", (long)row_pitch_bytes, wi);
    ADA_REQUIRE(batch == 1 || image_stride_bytes >= (int64_t)(hi - 1) * row_pitch_bytes + (int64_t)wi, ADA_EINVAL,
                "ada_mask_prep_fwd: mask stride %ld overlaps the previous mask", (long)image_stride_bytes);
    ADA_REQUIRE((ho + 3) / 4 <= 65535 && batch <= 65535, ADA_EUNSUPPORTED, "ada_mask_prep_fwd: ho / batch exceed the grid limits");
    MaskArgs a;
    a.src = src; a.pitch = row_pitch_bytes; a.istride = batch == 1 ? 0 : image_stride_bytes;
    a.hi = hi; a.wi = wi; a.ho = ho; a.wo = wo;
    a.ny = (float)hi / (float)ho;
    a.nx = (float)wi / (float)wo;
    a.out01 = out01; a.out_pm1 = out_pm1;
    hipLaunchKernelGGL(mask_prep_kernel, dim3((unsigned)((wo + 63) / 64), (unsigned)((ho + 3) / 4), (unsigned)batch), dim3(64, 4), 0,
                       (hipStream_t)stream, a);
    return ada_check_launch("ada_mask_prep_fwd");
}

extern "C" int ada_nearest_resize_fwd(const float* in, int32_t batch, int32_t hi, int32_t wi, int32_t ho, int32_t wo, float* out, void* stream) {
    ADA_REQUIRE(in && out, ADA_EINVAL, "ada_nearest_resize_fwd: null pointer");
    ADA_REQUIRE(batch > 0 && hi > 0 && wi > 0 && ho > 0 && wo > 0, ADA_EINVAL, "ada_nearest_resize_fwd: bad shape batch=%d %dx%d -> %dx%d", batch, hi, wi, ho, wo);
    ADA_REQUIRE((ho + 3) / 4 <= 65535 && batch <= 65535, ADA_EUNSUPPORTED, "ada_nearest_resize_fwd: ho / batch exceed the grid limits");
    NearestArgs a;
    a.in = in; a.out = out; a.hi = hi; a.wi = wi; a.ho = ho; a.wo = wo;
    a.ify = 1.0 / ((double)ho / hi);
    a.ifx = 1.0 / ((double)wo / wi);
    hipLaunchKernelGGL(nearest_resize_kernel, dim3((unsigned)((wo + 63) / 64), (unsigned)((ho + 3) / 4), (unsigned)batch), dim3(64, 4), 0,
                       (hipStream_t)stream, a);
    return ada_check_launch("ada_nearest_resize_fwd");
}

extern "C" int ada_depth_render_fwd(const float* depth, int32_t batch, int32_t hi, int32_t wi, const float* minmax, float lo, float hi_value,
                                    const uint8_t* lut, const float* mask, int32_t thickness, uint32_t outline_rgb, double alpha,
                                    int32_t ho, int32_t wo, int32_t bgr, uint8_t* out, uint16_t* out_u16, void* stream) {
    ADA_REQUIRE(depth && lut, ADA_EINVAL, "ada_depth_render_fwd: null pointer");
    ADA_REQUIRE(out || out_u16, ADA_EINVAL, "ada_depth_render_fwd: null pointer (both outputs)");
    ADA_REQUIRE(batch > 0 && hi > 0 && wi > 0 && ho > 0 && wo > 0, ADA_EINVAL, "ada_depth_render_fwd: bad shape batch=%d %dx%d -> %dx%d", batch, hi, wi, ho, wo);
    ADA_REQUIRE(thickness >= 1 && thickness <= 4, ADA_EINVAL, "ada_depth_render_fwd: thickness %d (1..4)", thickness);
    ADA_REQUIRE(outline_rgb <= 0xffffffu, ADA_EINVAL, "ada_depth_render_fwd: outline colour 0x%x is not 0xRRGGBB", outline_rgb);
    ADA_REQUIRE(alpha >= 0.0 && alpha <= 1.0, ADA_EINVAL, "ada_depth_render_fwd: alpha %g outside [0, 1]", alpha);
    ADA_REQUIRE((ho + 3) / 4 <= 65535 && batch <= 65535, ADA_EUNSUPPORTED, "ada_depth_render_fwd: ho / batch exceed the grid limits");
    RenderArgs a;
    a.depth = depth; a.minmax = minmax; a.lut = lut; a.mask = mask; a.out = out; a.out_u16 = out_u16;
    a.hi = hi; a.wi = wi; a.ho = ho; a.wo = wo;
    a.ify = 1.0 / ((double)ho / hi);
    a.ifx = 1.0 / ((double)wo / wi);
    a.lo = lo;
    a.span = (float)((double)hi_value - (double)lo);
    a.keep = 1.0 - alpha;
    a.fg = alpha * 200.0;
    a.overlay = (mask && alpha != 0.0) ? 1 : 0;
    a.radius = thickness - 1;
    a.outline = ((outline_rgb >> 16) & 0xffu) | (outline_rgb & 0x00ff00u) | ((outline_rgb & 0xffu) << 16);
    a.bgr = bgr ? 1 : 0;
    const dim3 block(64, 4);
    if (wo % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)out_u16 % 8 == 0)
        hipLaunchKernelGGL(depth_render_kernel<4>, dim3((unsigned)((wo + 255) / 256), (unsigned)((ho + 3) / 4), (unsigned)batch), block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(depth_render_kernel<1>, dim3((unsigned)((wo + 63) / 64), (unsigned)((ho + 3) / 4), (unsigned)batch), block, 0, (hipStream_t)stream, a);
    return ada_check_launch("ada_depth_render_fwd");
}

// ---- the maps behind the quantiles (ada_quantile.hip): the normalizer's scale-and-shift and the reference's colorize() ----
namespace {

struct RangeMapArgs {
    const float* d;
    const float* range;      // [batch, 2]
    float* out;
    long n;
    float scale, shift, clip_lo, clip_hi;
    int clip;
};

// ScaleShiftDepthNormalizer.__call__ (src/util/depth_transform.py:87-94): four torch ops, each rounded to fp32, then torch.clip (NaN passes)
__global__ __launch_bounds__(256) void range_map_kernel(RangeMapArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const float lo = a.range[2 * b], span = a.range[2 * b + 1] - lo;
    const float* d = a.d + (long)b * a.n;
    float* o = a.out + (long)b * a.n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
        float t = (d[i] - lo) / span;
        t = t * a.scale;
        t = t + a.shift;
        if (a.clip) t = t < a.clip_lo ? a.clip_lo : (t > a.clip_hi ? a.clip_hi : t);
        o[i] = t;
    }
}

struct ColorizeArgs {
    const float* value;
    const double* range;     // [batch, 2] or NULL
    const uint8_t* lut;      // [256][4]
    const uint8_t* invalid;  // [batch, h * w] or NULL
    uint32_t* out;           // [batch, h * w] RGBA pixels
    long n;
    double vmin, vmax, invalid_val;
    uint32_t background;
};

// colorize() (src/scripts/colorize_depth.py:50-75) on the map promoted to double; the table sits in LDS as pixels
__global__ __launch_bounds__(256) void depth_colorize_kernel(ColorizeArgs a) {
#pragma clang fp contract(off)
    __shared__ uint32_t lut[256];
    lut[threadIdx.x] = reinterpret_cast<const uint32_t*>(a.lut)[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y;
    const double vmin = a.range ? a.range[2 * b] : a.vmin, vmax = a.range ? a.range[2 * b + 1] : a.vmax;
    const bool flat = !(vmin != vmax);       // `if vmin != vmax`: a NaN bound normalises (and every t is NaN)
    const double span = vmax - vmin;
    const long base = (long)b * a.n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
        const double v = (double)a.value[base + i];
        const bool bad = a.invalid ? a.invalid[base + i] != 0 : v == a.invalid_val;
        uint32_t px = a.background;
        if (!bad) {
            const double t = flat ? v * 0.0 : (v - vmin) / span;
            if (t != t) px = 0u;
            else if (t < 0.0) px = lut[0];
            else if (t >= 1.0) px = lut[255];
            else px = lut[(int)(t * 256.0)];     // t in [0, 1): the index is 0 .. 255
        }
        a.out[base + i] = px;
    }
}

}  // namespace

extern "C" int ada_range_map_fwd(const float* d, const float* range, int32_t batch, int64_t n_per_image, float scale, float shift, int32_t clip,
                                 float clip_lo, float clip_hi, float* out, void* stream) {
    ADA_REQUIRE(d && range && out, ADA_EINVAL, "ada_range_map_fwd: null pointer");
    ADA_REQUIRE(batch > 0 && n_per_image > 0, ADA_EINVAL, "ada_range_map_fwd: bad shape batch=%d n=%ld", batch, (long)n_per_image);
    ADA_REQUIRE(batch <= 65535, ADA_EUNSUPPORTED, "ada_range_map_fwd: batch exceeds the grid limit");
    RangeMapArgs a;
    a.d = d; a.range = range; a.out = out; a.n = (long)n_per_image;
    a.scale = scale; a.shift = shift; a.clip = clip ? 1 : 0; a.clip_lo = clip_lo; a.clip_hi = clip_hi;
    const int64_t blocks = (n_per_image + 255) / 256;
    hipLaunchKernelGGL(range_map_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    return ada_check_launch("ada_range_map_fwd");
}

extern "C" int ada_depth_colorize_fwd(const float* value, int32_t batch, int32_t h, int32_t w, const double* range, double vmin, double vmax,
                                      const uint8_t* lut, const uint8_t* invalid_mask, double invalid_val, uint32_t background_rgba, uint8_t* out,
                                      void* stream) {
    ADA_REQUIRE(value && lut && out, ADA_EINVAL, "ada_depth_colorize_fwd: null pointer");
    ADA_REQUIRE(batch > 0 && h > 0 && w > 0, ADA_EINVAL, "ada_depth_colorize_fwd: bad shape batch=%d %dx%d", batch, h, w);
    ADA_REQUIRE(batch <= 65535, ADA_EUNSUPPORTED, "ada_depth_colorize_fwd: batch exceeds the grid limit");
    ADA_REQUIRE((uintptr_t)lut % 4 == 0 && (uintptr_t)out % 4 == 0, ADA_EINVAL, "ada_depth_colorize_fwd: lut and out must be 4-byte aligned");
    ColorizeArgs a;
    a.value = value; a.range = range; a.lut = lut; a.invalid = invalid_mask; a.out = reinterpret_cast<uint32_t*>(out);
    a.n = (long)h * w; a.vmin = vmin; a.vmax = vmax; a.invalid_val = invalid_val; a.background = background_rgba;
    const long blocks = (a.n + 255) / 256;
    hipLaunchKernelGGL(depth_colorize_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    return ada_check_launch("ada_depth_colorize_fwd");
}
