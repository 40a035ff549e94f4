// The preparation and the read-out of the ADIW pseudo-label generator (reference src/scripts/sam_pl_gen_dav2.py) on the device.  The reference
// prepares every photo and mask with Pillow on the host -- Image.open(fp).convert('RGB').resize((518, 518)), line 28; the masks the same way, lines
// 93-98 -- which is Pillow's antialiased BICUBIC convolution on 8-bit pixels (libImaging/Resample.c, ImagingResample), two integer passes with a uint8
// intermediate.  The first half of this file is that resize and Pillow's NEAREST (libImaging/Geometry.c, ImagingScaleAffine), byte for byte; the
// coefficient tables are the caller's (computed in double on the host, hip_ext/labels.py).  The second half is lines 115-117 and 121: paste the fitted
// map inside the whole mask, * 65535, numpy's astype(np.uint16), the NEAREST resize to the label size.
// Pillow 10.0.1 (the reference's pin, environment.yaml:227) resizes modes with ';' -- "I;16" -- with NEAREST by default; Pillow 12 defaults to BICUBIC
// for them.  The label is what the pinned version wrote: NEAREST.
// Neither is on the benchmark path: single memory-bound passes, no scratch, no atomics.
#include "ada_common.h"

namespace {

#define PIL_PRECISION_BITS 22    /* Resample.c: 32 - 8 - 2 */

struct EmitArgs {
    uint8_t* u8;             // HWC [batch][ho][wo][cn] or NULL
    float* f32;              // planar [batch, cn, ho, wo] or NULL
    uint8_t* mask;           // [batch][ho][wo] or NULL (cn == 1)
    int ho, wo;
};

// the outputs of one pixel: Pillow's bytes, np.array(im) / 255 as float32 (v / 255.f is IEEE division: the correctly rounded quotient, which equals
// (float)((double)v / 255.0) for all 256 values), v > 0
template <int CN>
ADA_DEV void emit(const EmitArgs& e, int b, int y, int x, const int v[CN]) {
    const long pix = ((long)b * e.ho + y) * e.wo + x;
    if (e.u8) {
#pragma unroll
        for (int c = 0; c < CN; ++c) e.u8[pix * CN + c] = (uint8_t)v[c];
    }
    if (e.f32) {
        const long plane = (long)e.ho * e.wo;
        float* o = e.f32 + (long)b * CN * plane + (long)y * e.wo + x;
#pragma unroll
        for (int c = 0; c < CN; ++c) o[c * plane] = (float)v[c] / 255.f;
    }
    if (CN == 1 && e.mask) e.mask[pix] = v[0] > 0 ? 1 : 0;
}

struct PassArgs {
    const uint8_t* in;       // HWC, cn bytes per pixel
    long pitch, istride;     // bytes between rows / images of `in`
    int n_in;                // length of the resized axis of `in`
    const int32_t* bounds;   // [n_out][2] = (xmin, n)
    const int32_t* kk;       // [n_out][ksize]
    int ksize;
    EmitArgs e;              // e.ho x e.wo: the grid of this pass
};

// clip8(acc >> 22): the shift is arithmetic, a negative sum clamps to 0
ADA_DEV int clip8(int acc) {
    const int v = acc >> PIL_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One pass of ImagingResample (AXIS 1: ImagingResampleHorizontal_8bpc, AXIS 0: ...Vertical_8bpc): acc = 2^21 + sum k[x] * pixel[xmin + x] in int32
// (Pillow's int; |k| sums to < 1.3 * 2^22, times 255 < 2^31), out = clip8(acc >> 22).  Block (64, 4), one output pixel per thread, every channel; the
// tap count is a loop.  The vertical pass reads rows coalesced along x with wave-uniform coefficients; the horizontal pass gathers bytes through the
// caches (a source row is read about once).  The table entries are clamped to the axis: a bad table cannot read outside the image.
template <int CN, int AXIS>
__global__ __launch_bounds__(256) void pil_pass_kernel(PassArgs a) {
    const int dx = blockIdx.x * 64 + threadIdx.x;
    const int dy = blockIdx.y * 4 + threadIdx.y;
    const int b = blockIdx.z;
    if (dx >= a.e.wo || dy >= a.e.ho) return;
    const int d = AXIS ? dx : dy;
    int xmin = a.bounds[2 * d], n = a.bounds[2 * d + 1];
    xmin = xmin < 0 ? 0 : (xmin > a.n_in ? a.n_in : xmin);
    n = n < a.ksize ? n : a.ksize;
    n = n < a.n_in - xmin ? n : a.n_in - xmin;
    const int32_t* k = a.kk + (long)d * a.ksize;
    const uint8_t* p = a.in + (long)b * a.istride + (AXIS ? (long)dy * a.pitch + (long)xmin * CN : (long)xmin * a.pitch + (long)dx * CN);
    const long step = AXIS ? CN : a.pitch;
    int acc[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) acc[c] = 1 << (PIL_PRECISION_BITS - 1);
    for (int x = 0; x < n; ++x) {
        const int w = k[x];
#pragma unroll
        for (int c = 0; c < CN; ++c) acc[c] += (int)p[c] * w;
        p += step;
    }
    int v[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) v[c] = clip8(acc[c]);
    emit<CN>(a.e, b, dy, dx, v);
}

// Pillow's NEAREST source index (Geometry.c): min((int)floor((d + 0.5) * scale), n_in - 1), scale = (double)n_in / n_out, in double
ADA_DEV int pil_nearest_src(int d, double scale, int n_in) {
#pragma clang fp contract(off)
    const int s = (int)__builtin_floor(((double)d + 0.5) * scale);
    return s < n_in - 1 ? s : n_in - 1;
}

struct GatherArgs {
    const uint8_t* in;
    long pitch, istride;
    int hi, wi;
    double sy, sx;           // (double)hi / ho, (double)wi / wo
    EmitArgs e;
};

// Image.resize(size, NEAREST) -- and, at equal sizes, the copy of a BICUBIC resize that has no pass to run.  Block (64, 4), one output pixel per thread.
template <int CN>
__global__ __launch_bounds__(256) void pil_nearest_kernel(GatherArgs a) {
    const int dx = blockIdx.x * 64 + threadIdx.x;
    const int dy = blockIdx.y * 4 + threadIdx.y;
    const int b = blockIdx.z;
    if (dx >= a.e.wo || dy >= a.e.ho) return;
    const uint8_t* p = a.in + (long)b * a.istride + (long)pil_nearest_src(dy, a.sy, a.hi) * a.pitch + (long)pil_nearest_src(dx, a.sx, a.wi) * CN;
    int v[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) v[c] = p[c];
    emit<CN>(a.e, b, dy, dx, v);
}

struct CombineArgs {
    const float* whole;      // [P, h, w]
    const float* occ;        // [P, h, w]
    const uint8_t* mask;     // [P, h, w]
    const float* ss;         // [P, 2]
    uint16_t* out_u16;       // [P, ho, wo]
    float* out_f32;          // [P, h, w] or NULL
    int32_t* oor;            // [P, ho] or NULL
    int h, w, ho, wo, rows;  // rows = max(h, ho)
    double sy, sx;           // (double)h / ho, (double)w / wo
    int clip;
};

// line 116: combine = whole_mask ? depth * scale + shift : occ_depth, in fp32, the product rounded before the sum (torch's `depth * scale + shift`)
ADA_DEV float combine_value(const CombineArgs& a, long i, float scale, float shift) {
#pragma clang fp contract(off)
    const float prod = a.whole[i] * scale;
    return a.mask[i] ? prod + shift : a.occ[i];
}

// line 117: (combine * 65535.0).astype(np.uint16).  numpy's cast on x86-64 is cvttss2si to int32 with the low 16 bits kept ("wrap"): NaN and
// |t| >= 2^31 give the indefinite integer 0x80000000, whose low half is 0.  The hardware's float -> integer conversion saturates instead, so the
// rule is written out.  clip: truncation after clamping to [0, 65535], NaN gives 0.
ADA_DEV uint32_t quantise(float t, int clip) {
    if (clip) {
        if (!(t > 0.f)) return 0u;
        return t >= 65535.f ? 65535u : (uint32_t)(int)t;
    }
    if (!(__builtin_fabsf(t) < 2147483648.f)) return 0u;
    return (uint32_t)(int)t & 0xffffu;
}

// Block (64, 4), grid (ceil(rows / 4), P): a wave owns row r of image b -- the row of the combined map (r < h) and the row of the label (r < ho) --
// and walks it 64 pixels at a time, so the row's out-of-range count is one wave's ballots added in order: no atomics, nothing to zero.  The label pixel
// (dy, dx) shows source pixel (sy, sx) by Pillow's NEAREST rule; nearest is a pure gather, so quantising what was gathered is the reference's
// quantise-then-resize.
__global__ __launch_bounds__(256) void label_combine_kernel(CombineArgs a) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 4 + threadIdx.y;
    const int b = blockIdx.y;
    if (r >= a.rows) return;     // wave-uniform
    const float scale = a.ss[2 * b], shift = a.ss[2 * b + 1];
    const long img = (long)b * a.h * a.w;
    if (a.out_f32 && r < a.h) {
        for (int x = threadIdx.x; x < a.w; x += 64) {
            const long i = img + (long)r * a.w + x;
            a.out_f32[i] = combine_value(a, i, scale, shift);
        }
    }
    if (r < a.ho) {
        const long srow = img + (long)pil_nearest_src(r, a.sy, a.h) * a.w;
        uint16_t* orow = a.out_u16 + ((long)b * a.ho + r) * a.wo;
        int count = 0;
        for (int x0 = 0; x0 < a.wo; x0 += 64) {
            const int dx = x0 + (int)threadIdx.x;
            bool bad = false;
            if (dx < a.wo) {
                const float t = combine_value(a, srow + pil_nearest_src(dx, a.sx, a.w), scale, shift) * 65535.f;
                orow[dx] = (uint16_t)quantise(t, a.clip);
                bad = !(t >= 0.f && t < 65536.f);
            }
            count += __popcll(__ballot(bad));
        }
        if (a.oor && threadIdx.x == 0) a.oor[(long)b * a.ho + r] = count;
    }
}

template <int CN, int AXIS>
void launch_pass(const PassArgs& a, int batch, hipStream_t s) {
    hipLaunchKernelGGL((pil_pass_kernel<CN, AXIS>), dim3((unsigned)((a.e.wo + 63) / 64), (unsigned)((a.e.ho + 3) / 4), (unsigned)batch), dim3(64, 4), 0, s, a);
}

}  // namespace

extern "C" int ada_pil_resize_u8_fwd(const uint8_t* src, int32_t batch, int32_t hi, int32_t wi, int32_t channels, int64_t row_pitch_bytes,
                                     int64_t image_stride_bytes, int32_t ho, int32_t wo, int32_t filter, const int32_t* bounds_x, const int32_t* kk_x,
                                     int32_t ksize_x, const int32_t* bounds_y, const int32_t* kk_y, int32_t ksize_y, uint8_t* tmp, int64_t tmp_bytes,
                                     uint8_t* out_u8, float* out_f32, uint8_t* out_mask, void* stream) {
    ADA_REQUIRE(src, ADA_EINVAL, "ada_pil_resize_u8_fwd: null pointer");
    ADA_REQUIRE(out_u8 || out_f32 || out_mask, ADA_EINVAL, "ada_pil_resize_u8_fwd: null pointer (every output)");
    ADA_REQUIRE(batch > 0 && hi > 0 && wi > 0 && ho > 0 && wo > 0, ADA_EINVAL, "ada_pil_resize_u8_fwd: bad shape batch=%d %dx%d -> %dx%d", batch, hi, wi, ho, wo);
    ADA_REQUIRE(channels == 1 || channels == 3, ADA_EINVAL, "ada_pil_resize_u8_fwd: %d channels (1 = L, 3 = RGB)", channels);
    ADA_REQUIRE(!out_mask || channels == 1, ADA_EINVAL, "ada_pil_resize_u8_fwd: out_mask needs channels == 1, got %d", channels);
    ADA_REQUIRE(filter == ADA_PIL_NEAREST || filter == ADA_PIL_BICUBIC, ADA_EINVAL, "ada_pil_resize_u8_fwd: filter %d (ADA_PIL_NEAREST, ADA_PIL_BICUBIC)", filter);
    ADA_REQUIRE(row_pitch_bytes >= (int64_t)wi * channels, ADA_EINVAL, "ada_pil_resize_u8_fwd: row pitch %ld < %d pixels x %d bytes", (long)row_pitch_bytes, wi, channels);
    ADA_REQUIRE(batch == 1 || image_stride_bytes >= (int64_t)(hi - 1) * row_pitch_bytes + (int64_t)wi * channels, ADA_EINVAL,
                "ada_pil_resize_u8_fwd: image stride %ld overlaps the previous image", (long)image_stride_bytes);
    ADA_REQUIRE((ho + 3) / 4 <= 65535 && (hi + 3) / 4 <= 65535 && batch <= 65535, ADA_EUNSUPPORTED, "ada_pil_resize_u8_fwd: hi / ho / batch exceed the grid limits");
    const bool horiz = filter == ADA_PIL_BICUBIC && wi != wo, vert = filter == ADA_PIL_BICUBIC && hi != ho;
    ADA_REQUIRE(!horiz || (bounds_x && kk_x && ksize_x > 0), ADA_EINVAL, "ada_pil_resize_u8_fwd: width %d -> %d needs the horizontal tables", wi, wo);
    ADA_REQUIRE(!vert || (bounds_y && kk_y && ksize_y > 0), ADA_EINVAL, "ada_pil_resize_u8_fwd: height %d -> %d needs the vertical tables", hi, ho);
    const int64_t tmp_need = (int64_t)batch * hi * wo * channels;
    ADA_REQUIRE(!(horiz && vert) || (tmp && tmp_bytes >= tmp_need), ADA_EINVAL, "ada_pil_resize_u8_fwd: two passes need %ld bytes of tmp, got %ld",
                (long)tmp_need, (long)(tmp ? tmp_bytes : 0));
    const hipStream_t s = (hipStream_t)stream;
    const long istride = batch == 1 ? 0 : (long)image_stride_bytes;
    EmitArgs fin;
    fin.u8 = out_u8; fin.f32 = out_f32; fin.mask = out_mask; fin.ho = ho; fin.wo = wo;
    if (!horiz && !vert) {
        GatherArgs g;
        g.in = src; g.pitch = row_pitch_bytes; g.istride = istride; g.hi = hi; g.wi = wi;
        g.sy = (double)hi / ho; g.sx = (double)wi / wo;
        g.e = fin;
        const dim3 grid((unsigned)((wo + 63) / 64), (unsigned)((ho + 3) / 4), (unsigned)batch);
        if (channels == 3) hipLaunchKernelGGL(pil_nearest_kernel<3>, grid, dim3(64, 4), 0, s, g);
        else hipLaunchKernelGGL(pil_nearest_kernel<1>, grid, dim3(64, 4), 0, s, g);
        return ada_check_launch("ada_pil_resize_u8_fwd");
    }
    PassArgs v;     // the vertical pass reads the source itself when the width is kept
    v.in = src; v.pitch = row_pitch_bytes; v.istride = istride;
    if (horiz) {
        PassArgs h;
        h.in = src; h.pitch = row_pitch_bytes; h.istride = istride; h.n_in = wi;
        h.bounds = bounds_x; h.kk = kk_x; h.ksize = ksize_x;
        if (vert) {
            h.e.u8 = tmp; h.e.f32 = nullptr; h.e.mask = nullptr; h.e.ho = hi; h.e.wo = wo;
            v.in = tmp; v.pitch = (long)wo * channels; v.istride = (long)hi * wo * channels;
        } else {
            h.e = fin;
        }
        if (channels == 3) launch_pass<3, 1>(h, batch, s);
        else launch_pass<1, 1>(h, batch, s);
    }
    if (vert) {
        v.n_in = hi; v.bounds = bounds_y; v.kk = kk_y; v.ksize = ksize_y; v.e = fin;
        if (channels == 3) launch_pass<3, 0>(v, batch, s);
        else launch_pass<1, 0>(v, batch, s);
    }
    return ada_check_launch("ada_pil_resize_u8_fwd");
}

extern "C" int ada_label_combine_fwd(const float* whole, const float* occ, const uint8_t* whole_mask, const float* scale_shift, int32_t batch, int32_t h,
                                     int32_t w, int32_t ho, int32_t wo, int32_t overflow, uint16_t* out_u16, float* out_f32, int32_t* out_of_range,
                                     void* stream) {
    ADA_REQUIRE(whole && occ && whole_mask && scale_shift && out_u16, ADA_EINVAL, "ada_label_combine_fwd: null pointer");
    ADA_REQUIRE(batch > 0 && h > 0 && w > 0 && ho > 0 && wo > 0, ADA_EINVAL, "ada_label_combine_fwd: bad shape batch=%d %dx%d -> %dx%d", batch, h, w, ho, wo);
    ADA_REQUIRE(overflow == ADA_LABEL_WRAP || overflow == ADA_LABEL_CLIP, ADA_EINVAL, "ada_label_combine_fwd: overflow %d (ADA_LABEL_WRAP, ADA_LABEL_CLIP)", overflow);
    const int rows = h > ho ? h : ho;
    ADA_REQUIRE(batch <= 65535, ADA_EUNSUPPORTED, "ada_label_combine_fwd: batch exceeds the grid limit");
    CombineArgs a;
    a.whole = whole; a.occ = occ; a.mask = whole_mask; a.ss = scale_shift;
    a.out_u16 = out_u16; a.out_f32 = out_f32; a.oor = out_of_range;
    a.h = h; a.w = w; a.ho = ho; a.wo = wo; a.rows = rows;
    a.sy = (double)h / ho; a.sx = (double)w / wo;
    a.clip = overflow == ADA_LABEL_CLIP ? 1 : 0;
    hipLaunchKernelGGL(label_combine_kernel, dim3((unsigned)((rows + 3) / 4), (unsigned)batch), dim3(64, 4), 0, (hipStream_t)stream, a);
    return ada_check_launch("ada_label_combine_fwd");
}
