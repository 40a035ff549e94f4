// Host-side image preparation and depth read-out of the raw model's infer_image, on the device (reference RAW/dpt.py:186-221,
// RAW/util/transform.py:5-158).  The reference prepares a decoded photo with OpenCV on the host: BGR -> RGB, / 255 (float64),
// cv2.resize INTER_CUBIC to the network size, ImageNet normalisation; after the forward it resizes the depth map back to the photo
// with F.interpolate(bilinear, align_corners=True).  Neither kernel is on the benchmark path: each is one memory-bound pass.
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
