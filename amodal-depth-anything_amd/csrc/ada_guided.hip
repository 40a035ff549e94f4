// Guided filter and guided joint up-sampling (He, Sun, Tang) -- the contract is include/ada_hip.h's "Guided filter" section, restated in numpy by
// tests/_guided_ref.py.  Everything is fp64: the window sums, the moments, the solve, the bilinear weights and a I + b; one rounding to fp32 at the end.
// Built without floating-point contraction (csrc/build.py): the apply pass's coordinate, weights and final sum are the restatement's bit for bit.
//
// Coefficient pass, at the map's size, four launches over a caller's workspace:
//   1. gf_moment_col_kernel   per pixel the sums over the window's ROWS of the M = 5 (C = 1) / 14 (C = 3) planes  1, I, I I^T, p, I p  of the voting samples
//   2. gf_fit_row_kernel      sums those over the window's COLUMNS (a row's planes staged through LDS), then per pixel the moments and the LDL^T solve:
//                             planes (a, b, has) of the window fit
//   3. gf_plane_col_kernel    column sums of those C + 2 planes
//   4. gf_mean_row_kernel     row sums, the division by the number of windows that had a fit: coefficients and ``covered``
// A thread owns one pixel; its accumulators are arrays indexed by unrolled constants.  A window clipped by the image is a shorter loop (columns) or
// zeros staged into LDS (rows); trip counts depend on the shapes and the radius alone.
// Apply pass, at the guide's size: a thread owns four pixels of a row -- one 4 C-byte (uint8) or C 16-byte (fp32) load of the guide and one 16-byte
// store when the row length is a multiple of four, element by element otherwise -- and gathers the four bilinear taps of each from the coefficient table.
#include "ada_common.h"

namespace {

constexpr int GF_THREADS = 256;
constexpr int GF_TILE_W = ADA_GUIDED_TILE_W;                       // outputs of a row per workgroup of the row passes
constexpr int GF_TILE_LD = GF_TILE_W + 2 * ADA_GUIDED_MAX_RADIUS;   // with the halo of the widest window
constexpr int GF_APPLY_PX = ADA_GUIDED_APPLY_PX;
static_assert(GF_TILE_W == GF_THREADS, "a thread of the row passes owns one output");

constexpr int gf_moments(int C) { return C == 1 ? 5 : 14; }

// (2 i + 1) n / (2 m): the guide sample of map index i.  i, m, n <= 32767, so the product stays below 2^31
ADA_DEV uint32_t gf_sample_index(int i, int m, int n) { return ((2u * (uint32_t)i + 1u) * (uint32_t)n) / (2u * (uint32_t)m); }

template <int C, typename G>
__global__ __launch_bounds__(GF_THREADS) void gf_moment_col_kernel(const float* p, const uint8_t* valid, const G* guide, int h, int w, int gh, int gw, int r,
                                                                   double* col) {
    constexpr int M = gf_moments(C);
    const int x = blockIdx.x * GF_THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const long b = blockIdx.z;
    const float* pb = p + b * h * w;
    const uint8_t* vb = valid ? valid + b * h * w : nullptr;
    const G* gb = guide + b * gh * gw * C;
    const long gx = gf_sample_index(x, w, gw);
    double s[M];
#pragma unroll
    for (int m = 0; m < M; ++m) s[m] = 0.0;
    const int ya = y - r > 0 ? y - r : 0, yb = y + r < h - 1 ? y + r : h - 1;
    for (int yy = ya; yy <= yb; ++yy) {
        const long i = (long)yy * w + x;
        const float pv = pb[i];
        const bool vote = (!vb || vb[i]) && pv == pv;
        const G* gp = gb + ((long)gf_sample_index(yy, h, gh) * gw + gx) * C;
        double g[C];
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = vote ? (double)gp[c] : 0.0;      // by a select: what lies under a sample that does not vote never reaches a sum
        const double pd = vote ? (double)pv : 0.0;
        // planes: 1 | I_c | I_c I_d (c <= d, row-major) | p | I_c p.  Every product is exact in fp64 (8 or 24 bits times 24 bits)
        int m = 0;
        s[m++] += vote ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) s[m++] += g[c];
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int d = c; d < C; ++d) s[m++] += g[c] * g[d];
        s[m++] += pd;
#pragma unroll
        for (int c = 0; c < C; ++c) s[m++] += g[c] * pd;
    }
    double* o = col + ((b * h + y) * M) * w + x;
#pragma unroll
    for (int m = 0; m < M; ++m) o[(long)m * w] = s[m];
}

// column sums of P planes [batch][h][P][w] -> the same layout
template <int P>
__global__ __launch_bounds__(GF_THREADS) void gf_plane_col_kernel(const double* in, int h, int w, int r, double* col) {
    const int x = blockIdx.x * GF_THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const long b = blockIdx.z;
    double s[P];
#pragma unroll
    for (int m = 0; m < P; ++m) s[m] = 0.0;
    const int ya = y - r > 0 ? y - r : 0, yb = y + r < h - 1 ? y + r : h - 1;
    for (int yy = ya; yy <= yb; ++yy) {
        const double* q = in + ((b * h + yy) * P) * w + x;
#pragma unroll
        for (int m = 0; m < P; ++m) s[m] += q[(long)m * w];
    }
    double* o = col + ((b * h + y) * P) * w + x;
#pragma unroll
    for (int m = 0; m < P; ++m) o[(long)m * w] = s[m];
}

// acc[m] = the sum over the window's columns of plane m of the row ``rowp`` ([NP][w]) for this thread's output column; columns outside the image are
// staged as zeros.  Every thread of the workgroup calls it (one barrier)
template <int NP>
ADA_DEV void gf_row_sums(const double* rowp, int w, int r, double (&acc)[NP], double (*tile)[GF_TILE_LD]) {
    const int x0 = blockIdx.x * GF_TILE_W - r, n = GF_TILE_W + 2 * r;
#pragma unroll
    for (int m = 0; m < NP; ++m)
        for (int j = threadIdx.x; j < n; j += GF_THREADS) {
            const int x = x0 + j;
            tile[m][j] = x >= 0 && x < w ? rowp[(long)m * w + x] : 0.0;
        }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NP; ++m) acc[m] = 0.0;
    for (int j = 0; j <= 2 * r; ++j)
#pragma unroll
        for (int m = 0; m < NP; ++m) acc[m] += tile[m][threadIdx.x + j];
}

// the window fit of one pixel from its M sums: planes (a_c, b, has) of [batch][h][C + 2][w]
template <int C>
__global__ __launch_bounds__(GF_THREADS) void gf_fit_row_kernel(const double* col, int h, int w, int r, double eps, double* ab) {
    constexpr int M = gf_moments(C), P = C + 2;
    __shared__ double tile[M][GF_TILE_LD];
    const int x = blockIdx.x * GF_TILE_W + threadIdx.x, y = blockIdx.y;
    const long b = blockIdx.z;
    double s[M];
    gf_row_sums<M>(col + ((b * h + y) * M) * w, w, r, s, tile);
    if (x >= w) return;
    double out[P];
#pragma unroll
    for (int m = 0; m < P; ++m) out[m] = 0.0;
    const double n = s[0];
    if (n > 0.0) {
        double mi[C], cp[C];
        const double mp = s[M - C - 1] / n;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            mi[c] = s[1 + c] / n;
            cp[c] = s[M - C + c] / n - mi[c] * mp;
        }
        if constexpr (C == 1) {
            out[0] = cp[0] / ((s[2] / n - mi[0] * mi[0]) + eps);
            out[1] = mp - out[0] * mi[0];
        } else {
            // A = Cov(I, I) + eps U = L D L^T, by the rows of L; then L z = Cov(I, p), D y = z, L^T a = y
            const double a00 = (s[4] / n - mi[0] * mi[0]) + eps, a01 = s[5] / n - mi[0] * mi[1], a02 = s[6] / n - mi[0] * mi[2];
            const double a11 = (s[7] / n - mi[1] * mi[1]) + eps, a12 = s[8] / n - mi[1] * mi[2], a22 = (s[9] / n - mi[2] * mi[2]) + eps;
            const double l10 = a01 / a00, l20 = a02 / a00;
            const double d1 = a11 - l10 * a01;
            const double t21 = a12 - l20 * a01;
            const double l21 = t21 / d1;
            const double d2 = (a22 - l20 * a02) - l21 * t21;
            const double z1 = cp[1] - l10 * cp[0];
            const double z2 = (cp[2] - l20 * cp[0]) - l21 * z1;
            const double a2 = z2 / d2;
            const double a1 = z1 / d1 - l21 * a2;
            const double a0 = (cp[0] / a00 - l10 * a1) - l20 * a2;
            out[0] = a0; out[1] = a1; out[2] = a2;
            out[3] = mp - ((a0 * mi[0] + a1 * mi[1]) + a2 * mi[2]);
        }
        out[P - 1] = 1.0;
    }
    double* o = ab + ((b * h + y) * P) * w + x;
#pragma unroll
    for (int m = 0; m < P; ++m) o[(long)m * w] = out[m];
}

// the mean of the fits over the window's pixels that have one: coeff [batch][h][w][C + 1], covered [batch][h][w]
template <int C>
__global__ __launch_bounds__(GF_THREADS) void gf_mean_row_kernel(const double* col, int h, int w, int r, double* coeff, uint8_t* covered) {
    constexpr int P = C + 2;
    __shared__ double tile[P][GF_TILE_LD];
    const int x = blockIdx.x * GF_TILE_W + threadIdx.x, y = blockIdx.y;
    const long b = blockIdx.z;
    double s[P];
    gf_row_sums<P>(col + ((b * h + y) * P) * w, w, r, s, tile);
    if (x >= w) return;
    const long i = (b * h + y) * w + x;
    const double n = s[P - 1];
#pragma unroll
    for (int m = 0; m <= C; ++m) coeff[i * (C + 1) + m] = n > 0.0 ? s[m] / n : 0.0;
    covered[i] = n > 0.0 ? 1 : 0;
}

// GF_APPLY_PX guide pixels starting at ``s`` as doubles: g[px * C + c].  VEC: one aligned word (uint8) or 16 bytes (fp32) per channel count
template <int C, bool VEC>
ADA_DEV void gf_load_guide(const uint8_t* s, int n, double (&g)[GF_APPLY_PX * C]) {
    if constexpr (VEC) {
        uint32_t wd[C];
#pragma unroll
        for (int i = 0; i < C; ++i) wd[i] = ((const uint32_t*)s)[i];
#pragma unroll
        for (int i = 0; i < GF_APPLY_PX * C; ++i) g[i] = (double)((wd[i >> 2] >> (8 * (i & 3))) & 255u);
    } else {
#pragma unroll
        for (int i = 0; i < GF_APPLY_PX * C; ++i) g[i] = i < n * C ? (double)s[i] : 0.0;
    }
}
template <int C, bool VEC>
ADA_DEV void gf_load_guide(const float* s, int n, double (&g)[GF_APPLY_PX * C]) {
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const float4 v = ((const float4*)s)[i];
            g[4 * i] = (double)v.x; g[4 * i + 1] = (double)v.y; g[4 * i + 2] = (double)v.z; g[4 * i + 3] = (double)v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < GF_APPLY_PX * C; ++i) g[i] = i < n * C ? (double)s[i] : 0.0;
    }
}

// source coordinate of output index X on an axis of n_in samples stretched to n_out: ((X + 0.5) n_in) / n_out - 0.5 clamped to [0, n_in - 1], in this order
ADA_DEV double gf_source(int X, int n_in, int n_out) {
    double s = (((double)X + 0.5) * (double)n_in) / (double)n_out - 0.5;
    s = s < 0.0 ? 0.0 : s;
    const double top = (double)(n_in - 1);
    return s > top ? top : s;
}

template <int C, typename G, bool VEC>
__global__ __launch_bounds__(GF_THREADS) void gf_apply_kernel(const double* coeff, const uint8_t* covered, const G* guide, int h, int w, int H, int W,
                                                              float fill, float* out) {
    const int X0 = (blockIdx.x * GF_THREADS + threadIdx.x) * GF_APPLY_PX, Y = blockIdx.y;
    if (X0 >= W) return;
    const long b = blockIdx.z;
    const int n = W - X0 < GF_APPLY_PX ? W - X0 : GF_APPLY_PX;
    const double* cb = coeff + b * h * w * (C + 1);
    const uint8_t* vb = covered + b * h * w;
    const long row = (b * H + Y) * W + X0;
    double g[GF_APPLY_PX * C];
    gf_load_guide<C, VEC>(guide + row * C, n, g);
    const double sy = gf_source(Y, h, H);
    const int y0 = (int)sy, y1 = y0 + 1 < h ? y0 + 1 : h - 1;
    const double fy = sy - (double)y0;
    float q[GF_APPLY_PX];
#pragma unroll
    for (int k = 0; k < GF_APPLY_PX; ++k) {
        const int X = X0 + k < W ? X0 + k : W - 1;
        const double sx = gf_source(X, w, W);
        const int x0 = (int)sx, x1 = x0 + 1 < w ? x0 + 1 : w - 1;
        const double fx = sx - (double)x0;
        const double wt[4] = {(1.0 - fy) * (1.0 - fx), (1.0 - fy) * fx, fy * (1.0 - fx), fy * fx};
        const long at[4] = {(long)y0 * w + x0, (long)y0 * w + x1, (long)y1 * w + x0, (long)y1 * w + x1};
        double acc[C + 1], wsum = 0.0;
#pragma unroll
        for (int j = 0; j <= C; ++j) acc[j] = 0.0;
        bool dropped = false;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (wt[t] > 0.0) {      // a tap of weight zero is not read: a same-size call is the single tap
                if (vb[at[t]]) {
                    wsum += wt[t];
#pragma unroll
                    for (int j = 0; j <= C; ++j) acc[j] += wt[t] * cb[at[t] * (C + 1) + j];
                } else {
                    dropped = true;
                }
            }
        }
        if (dropped && wsum > 0.0) {
#pragma unroll
            for (int j = 0; j <= C; ++j) acc[j] = acc[j] / wsum;
        }
        double v = acc[0] * g[k * C];
#pragma unroll
        for (int c = 1; c < C; ++c) v = v + acc[c] * g[k * C + c];
        v = v + acc[C];
        q[k] = wsum > 0.0 ? (float)v : fill;
    }
    if constexpr (VEC) {
        *(float4*)(out + row) = make_float4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
        for (int k = 0; k < GF_APPLY_PX; ++k)
            if (k < n) out[row + k] = q[k];
    }
}

unsigned gf_blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }

int gf_check(const char* who, int32_t guide_dtype, int32_t batch, int32_t h, int32_t w, int32_t gh, int32_t gw, int32_t channels) {
    ADA_REQUIRE(batch > 0 && h > 0 && w > 0 && gh > 0 && gw > 0, ADA_EINVAL, "%s: bad shape batch=%d map %dx%d guide %dx%d", who, batch, h, w, gh, gw);
    ADA_REQUIRE(channels == 1 || channels == 3, ADA_EINVAL, "%s: the guide has 1 or 3 channels, got %d", who, channels);
    ADA_REQUIRE(guide_dtype == ADA_DT_U8 || guide_dtype == ADA_DT_F32, ADA_EINVAL, "%s: the guide is uint8 or fp32, got dtype %d", who, guide_dtype);
    ADA_REQUIRE(gh >= h && gw >= w, ADA_EINVAL, "%s: the guide (%dx%d) must not be smaller than the map (%dx%d)", who, gh, gw, h, w);
    ADA_REQUIRE(gh <= 32767 && gw <= 32767, ADA_EUNSUPPORTED, "%s: sides must stay within 32767, got %dx%d", who, gh, gw);
    ADA_REQUIRE(batch <= 65535, ADA_EUNSUPPORTED, "%s: batch must stay within 65535, got %d", who, batch);
    return ADA_OK;
}

int64_t gf_workspace(int32_t batch, int32_t h, int32_t w, int32_t channels) {
    return (int64_t)8 * batch * h * w * (gf_moments(channels) + channels + 2);
}

template <int C, typename G>
void gf_coeff_launch(const float* p, const uint8_t* valid, const G* guide, int batch, int h, int w, int gh, int gw, int r, double eps, double* coeff,
                     uint8_t* covered, double* col, hipStream_t s) {
    double* ab = col + (int64_t)batch * h * w * gf_moments(C);
    const dim3 grid(gf_blocks(w, GF_THREADS), (unsigned)h, (unsigned)batch), block(GF_THREADS);
    hipLaunchKernelGGL((gf_moment_col_kernel<C, G>), grid, block, 0, s, p, valid, guide, h, w, gh, gw, r, col);
    hipLaunchKernelGGL((gf_fit_row_kernel<C>), grid, block, 0, s, (const double*)col, h, w, r, eps, ab);
    hipLaunchKernelGGL((gf_plane_col_kernel<C + 2>), grid, block, 0, s, (const double*)ab, h, w, r, col);
    hipLaunchKernelGGL((gf_mean_row_kernel<C>), grid, block, 0, s, (const double*)col, h, w, r, coeff, covered);
}

template <int C, typename G>
void gf_apply_launch(const double* coeff, const uint8_t* covered, const G* guide, int batch, int h, int w, int H, int W, float fill, float* out, hipStream_t s) {
    const dim3 grid(gf_blocks(W, GF_THREADS * GF_APPLY_PX), (unsigned)H, (unsigned)batch), block(GF_THREADS);
    // rows of a multiple of four pixels keep every group of four aligned: 4 C bytes of a uint8 guide on 4, fp32 and the output on 16
    const bool vec = W % GF_APPLY_PX == 0 && ((uintptr_t)guide | (uintptr_t)out) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL((gf_apply_kernel<C, G, true>), grid, block, 0, s, coeff, covered, guide, h, w, H, W, fill, out);
    else
        hipLaunchKernelGGL((gf_apply_kernel<C, G, false>), grid, block, 0, s, coeff, covered, guide, h, w, H, W, fill, out);
}

}  // namespace

extern "C" int ada_guided_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t channels, int64_t* bytes) {
    ADA_REQUIRE(bytes, ADA_EINVAL, "ada_guided_workspace_bytes: null pointer");
    if (int rc = gf_check("ada_guided_workspace_bytes", ADA_DT_U8, batch, h, w, h, w, channels)) return rc;
    *bytes = gf_workspace(batch, h, w, channels);
    return ADA_OK;
}

extern "C" int ada_guided_coeff_fwd(const float* p, const uint8_t* valid, const void* guide, int32_t guide_dtype, int32_t batch, int32_t h, int32_t w,
                                    int32_t gh, int32_t gw, int32_t channels, int32_t radius, double eps, double* coeff, uint8_t* covered,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(p && guide && coeff && covered, ADA_EINVAL, "ada_guided_coeff_fwd: null pointer");
    if (int rc = gf_check("ada_guided_coeff_fwd", guide_dtype, batch, h, w, gh, gw, channels)) return rc;
    ADA_REQUIRE(radius >= 0 && radius <= ADA_GUIDED_MAX_RADIUS, ADA_EINVAL, "ada_guided_coeff_fwd: the radius must lie in 0 .. %d, got %d",
                ADA_GUIDED_MAX_RADIUS, radius);
    ADA_REQUIRE(eps > 0.0 && eps <= 1.79769313486231570e308, ADA_EINVAL, "ada_guided_coeff_fwd: eps must be finite and positive, got %g", eps);
    const int64_t need = gf_workspace(batch, h, w, channels);
    ADA_REQUIRE(workspace && workspace_bytes >= need && (uintptr_t)workspace % 8 == 0, ADA_EINVAL,
                "ada_guided_coeff_fwd: the workspace needs %ld bytes on an 8-byte boundary, got %ld", (long)need, (long)(workspace ? workspace_bytes : 0));
    const hipStream_t s = (hipStream_t)stream;
    double* col = (double*)workspace;
    if (guide_dtype == ADA_DT_U8) {
        if (channels == 1) gf_coeff_launch<1>(p, valid, (const uint8_t*)guide, batch, h, w, gh, gw, radius, eps, coeff, covered, col, s);
        else gf_coeff_launch<3>(p, valid, (const uint8_t*)guide, batch, h, w, gh, gw, radius, eps, coeff, covered, col, s);
    } else {
        if (channels == 1) gf_coeff_launch<1>(p, valid, (const float*)guide, batch, h, w, gh, gw, radius, eps, coeff, covered, col, s);
        else gf_coeff_launch<3>(p, valid, (const float*)guide, batch, h, w, gh, gw, radius, eps, coeff, covered, col, s);
    }
    return ada_check_launch("ada_guided_coeff_fwd");
}

extern "C" int ada_guided_apply_fwd(const double* coeff, const uint8_t* covered, const void* guide, int32_t guide_dtype, int32_t batch, int32_t h,
                                    int32_t w, int32_t gh, int32_t gw, int32_t channels, float fill, float* out, void* stream) {
    ADA_REQUIRE(coeff && covered && guide && out, ADA_EINVAL, "ada_guided_apply_fwd: null pointer");
    if (int rc = gf_check("ada_guided_apply_fwd", guide_dtype, batch, h, w, gh, gw, channels)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (guide_dtype == ADA_DT_U8) {
        if (channels == 1) gf_apply_launch<1>(coeff, covered, (const uint8_t*)guide, batch, h, w, gh, gw, fill, out, s);
        else gf_apply_launch<3>(coeff, covered, (const uint8_t*)guide, batch, h, w, gh, gw, fill, out, s);
    } else {
        if (channels == 1) gf_apply_launch<1>(coeff, covered, (const float*)guide, batch, h, w, gh, gw, fill, out, s);
        else gf_apply_launch<3>(coeff, covered, (const float*)guide, batch, h, w, gh, gw, fill, out, s);
    }
    return ada_check_launch("ada_guided_apply_fwd");
}
