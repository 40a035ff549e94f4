// Hole filling on the device: a pixel without a sample gets a value from the pixels that have one.  Two forms (include/ada_hip.h, "Hole filling"):
//   * the exact Euclidean feature transform -- for every pixel the flat position of the nearest valid pixel of its image, ties to the smallest flat
//     position -- and the gather that copies the value found there;
//   * the push-pull fill: a pyramid of masked 2 x 2 means (pull), then bilinear interpolation of the coarser level into the pixels that are still
//     empty (push), top down.
//
// ARITHMETIC CONTRACT ("Hole filling").  The feature transform is integer arithmetic only: squared distances are exact in 32 bits for
// h, w <= 32767.  The push-pull fill is fp32 throughout and is compared bit for bit with tests/_inpaint_ref.py: this file is built with
// -ffp-contract=off (csrc/build.py), every product and every sum written here is rounded on its own, no FMA may appear, and the division is the
// correctly rounded one (no fast-math flag anywhere in the build).  The value of an invalid pixel is never loaded into an arithmetic operation: it is
// replaced by a select, so NaN and inf under a hole change nothing.
//
// No atomics, no host read, nothing allocated: the launch sequence of every entry point depends on the shapes alone.  Every cell of the workspace
// that is read was written earlier in the same call.  No scratch (NO_SCRATCH).
#include "ada_common.h"

namespace {

constexpr int FT_NONE = 0x7fffffff;            // no valid pixel in this column / image
constexpr int FT_CHUNK = ADA_INPAINT_CHUNK;    // columns of one row staged per step of the row pass

unsigned ip_blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }

// ---- feature transform -----------------------------------------------------------------------------------------------------------------------
// one thread per column: for every pixel the row of the nearest valid pixel of its column (-1: the column has none), the upper one at equal |dy|.
// Two scans: the first leaves the nearest valid row at or above, the second meets it with the nearest at or below.
__global__ __launch_bounds__(256) void ft_col_kernel(const uint8_t* valid, int* near_row, int h, int w) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    const long base = (long)blockIdx.y * h * w + x;
    int up = -1;
    for (int y = 0; y < h; ++y) {
        const long o = base + (long)y * w;
        up = valid[o] ? y : up;
        near_row[o] = up;
    }
    int dn = -1;
    for (int y = h - 1; y >= 0; --y) {
        const long o = base + (long)y * w;
        const int u = near_row[o];
        dn = u == y ? y : dn;      // u == y: the pixel itself is valid
        int r;
        if (u < 0) r = dn;
        else if (dn < 0) r = u;
        else r = (y - u <= dn - y) ? u : dn;
        near_row[o] = r;
    }
}

// grid (ceil(w / 256), h, batch): min over x' of ((x - x')^2 + g(x')^2, r(x') w + x') in lexicographic order, the row's (g^2, flat position) pairs
// staged through LDS in chunks.  A column's nearest rows are the only candidates of that column (any other valid pixel of it is strictly farther), and
// of two at the same |dy| the upper has the smaller flat position, so the lexicographic minimum is the contract's nearest pixel.
__global__ __launch_bounds__(256) void ft_row_kernel(const int* near_row, int* index, int* dist2, int h, int w) {
    __shared__ int sg[FT_CHUNK];
    __shared__ int sf[FT_CHUNK];
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    const long row = ((long)blockIdx.z * h + y) * w;
    unsigned best_d = 0xffffffffu;
    int best_f = -1;
    for (int c0 = 0; c0 < w; c0 += FT_CHUNK) {
        const int n = w - c0 < FT_CHUNK ? w - c0 : FT_CHUNK;
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += 256) {
            const int r = near_row[row + c0 + j];
            const int g = y - r;
            sg[j] = r < 0 ? FT_NONE : g * g;
            sf[j] = r < 0 ? -1 : r * w + c0 + j;
        }
        __syncthreads();
        if (x < w) {
            const int nd = x < c0 ? c0 - x : (x >= c0 + n ? x - (c0 + n - 1) : 0);     // the chunk's nearest column
            if ((unsigned)(nd * nd) <= best_d) {      // <=: a chunk at the best distance may still hold a smaller flat position
                for (int j = 0; j < n; ++j) {
                    const int dx = x - (c0 + j);
                    const unsigned d = (unsigned)(dx * dx) + (unsigned)sg[j];      // FT_NONE + dx^2 stays below 2^32 and above every real distance
                    const int f = sf[j];
                    const bool better = d < best_d || (d == best_d && f < best_f);
                    best_d = better ? d : best_d;
                    best_f = better ? f : best_f;
                }
            }
        }
    }
    if (x < w) {
        const bool none = best_d >= (unsigned)FT_NONE;
        index[row + x] = none ? -1 : best_f;
        if (dist2) dist2[row + x] = none ? FT_NONE : (int)best_d;
    }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(h w / 256), batch): values move as 32-bit words, so a valid pixel and a copied one keep every bit (-0.0, NaN payloads).  An index outside
// the image is treated as "none": nothing is read out of bounds whatever the caller hands in.
__global__ __launch_bounds__(256) void fill_gather_kernel(const uint32_t* x, const uint8_t* valid, const int* index, int channels, long hw, uint32_t empty,
                                                          uint32_t* out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const long b = blockIdx.y;
    const bool v = valid[b * hw + p] != 0;
    const int idx = index[b * hw + p];
    const bool found = idx >= 0 && (long)idx < hw;
    const long src = v ? p : (found ? (long)idx : 0);
    for (int c = 0; c < channels; ++c) {
        const long plane = (b * channels + c) * hw;
        out[plane + p] = (v || found) ? x[plane + src] : empty;
    }
}

// ---- push-pull -------------------------------------------------------------------------------------------------------------------------------
// Pull, level l -> l + 1: grid (ceil(ho wo / 256), batch), one thread per coarse pixel and all channels.  Level 0 reads x and valid themselves (lo_v = x,
// lo_m = valid); the select keeps an invalid pixel's value out of the sum.  ``top``: the coarse level is the 1 x 1 top, whose empty pixel takes ``empty``.
__global__ __launch_bounds__(256) void pp_pull_kernel(const float* lo_v, const uint8_t* lo_m, int channels, int hi, int wi, int ho, int wo, float* up_v,
                                                      uint8_t* up_m, int top, float empty) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long no = (long)ho * wo, ni = (long)hi * wi;
    if (i >= no) return;
    const long b = blockIdx.y;
    const int I = (int)(i / wo), J = (int)(i - (long)I * wo);
    const int y0 = 2 * I, x0 = 2 * J;
    const bool in_y = y0 + 1 < hi, in_x = x0 + 1 < wi;
    const long o00 = (long)y0 * wi + x0;
    const uint8_t* m = lo_m + b * ni;
    const bool m00 = m[o00] != 0;
    const bool m01 = in_x && m[o00 + 1] != 0;
    const bool m10 = in_y && m[o00 + wi] != 0;
    const bool m11 = in_y && in_x && m[o00 + wi + 1] != 0;
    const int n = (int)m00 + (int)m01 + (int)m10 + (int)m11;
    up_m[b * no + i] = n > 0 ? 1 : 0;
    const float fn = (float)n;
    for (int c = 0; c < channels; ++c) {
        const float* v = lo_v + (b * channels + c) * ni;
        const float s00 = m00 ? v[o00] : 0.f;
        const float s01 = m01 ? v[o00 + 1] : 0.f;
        const float s10 = m10 ? v[o00 + wi] : 0.f;
        const float s11 = m11 ? v[o00 + wi + 1] : 0.f;
        const float sum = ((s00 + s01) + s10) + s11;
        up_v[(b * channels + c) * no + i] = n > 0 ? sum / fn : (top ? empty : 0.f);
    }
}

ADA_DEV int pp_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Push, level l + 1 -> l: grid (ceil(h w / 256), batch).  A pixel with a sample keeps it (src, bit for bit); an empty one takes the bilinear value of the
// level above (half-pixel centres, clamped borders), which is completely filled by then.  Level 0 reads src = x, m = valid and writes dst = out;
// the levels between are rewritten in place (src == dst: a thread reads and writes its own pixel only).  ``up_v == nullptr``: the level is the
// top itself (a 1 x 1 image) and an empty pixel takes ``empty``.
__global__ __launch_bounds__(256) void pp_push_kernel(const float* src, const uint8_t* m, const float* up_v, int channels, int h, int w, int hu, int wu, float* dst,
                                                      float empty) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)h * w, nu = (long)hu * wu;
    if (p >= n) return;
    const long b = blockIdx.y;
    const bool keep = m[b * n + p] != 0;
    const int i = (int)(p / w), j = (int)(p - (long)i * w);
    const int I = i >> 1, J = j >> 1;
    const int I2 = pp_clamp(I + ((i & 1) ? 1 : -1), hu - 1), J2 = pp_clamp(J + ((j & 1) ? 1 : -1), wu - 1);
    for (int c = 0; c < channels; ++c) {
        const long plane = (b * channels + c) * n;
        if (keep) {
            if (dst != src) ((uint32_t*)dst)[plane + p] = ((const uint32_t*)src)[plane + p];
            continue;
        }
        float r = empty;
        if (up_v) {
            const float* u = up_v + (b * channels + c) * nu;
            const float va = u[(long)I * wu + J], vb = u[(long)I * wu + J2], vc = u[(long)I2 * wu + J], vd = u[(long)I2 * wu + J2];
            r = (((9.f * va + 3.f * vb) + 3.f * vc) + vd) * 0.0625f;
        }
        dst[plane + p] = r;
    }
}

int check_shape(const char* who, int32_t batch, int32_t channels, int32_t h, int32_t w) {
    ADA_REQUIRE(batch > 0 && channels > 0 && h > 0 && w > 0, ADA_EINVAL, "%s: bad shape batch=%d channels=%d %dx%d", who, batch, channels, h, w);
    ADA_REQUIRE(h <= 32767 && w <= 32767, ADA_EUNSUPPORTED, "%s: h and w must stay within 32767 (squared distances are exact in 32 bits), got %dx%d", who, h, w);
    ADA_REQUIRE(batch <= 65535, ADA_EUNSUPPORTED, "%s: batch must stay within 65535, got %d", who, batch);
    return ADA_OK;
}

// the pyramid above level 0: per level fp32 [batch][channels][h_l][w_l], all levels' values first, then per level uint8 [batch][h_l][w_l]
int64_t pp_level_pixels(int32_t h, int32_t w) {
    int64_t px = 0;
    while (h > 1 || w > 1) {
        h = (h + 1) / 2;
        w = (w + 1) / 2;
        px += (int64_t)h * w;
    }
    return px;
}

}  // namespace

extern "C" int ada_nearest_valid_workspace_bytes(int32_t batch, int32_t h, int32_t w, int64_t* bytes) {
    ADA_REQUIRE(bytes, ADA_EINVAL, "ada_nearest_valid_workspace_bytes: null pointer");
    if (int rc = check_shape("ada_nearest_valid_workspace_bytes", batch, 1, h, w)) return rc;
    *bytes = (int64_t)4 * batch * h * w;
    return ADA_OK;
}

extern "C" int ada_nearest_valid_fwd(const uint8_t* valid, int32_t batch, int32_t h, int32_t w, int32_t* index, int32_t* dist2, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(valid && index, ADA_EINVAL, "ada_nearest_valid_fwd: null pointer");
    if (int rc = check_shape("ada_nearest_valid_fwd", batch, 1, h, w)) return rc;
    const int64_t need = (int64_t)4 * batch * h * w;
    ADA_REQUIRE(workspace && workspace_bytes >= need, ADA_EINVAL, "ada_nearest_valid_fwd: the workspace needs %ld bytes, got %ld", (long)need,
                (long)(workspace ? workspace_bytes : 0));
    const hipStream_t s = (hipStream_t)stream;
    int* near_row = (int*)workspace;
    hipLaunchKernelGGL(ft_col_kernel, dim3(ip_blocks(w, 256), (unsigned)batch), dim3(256), 0, s, valid, near_row, h, w);
    hipLaunchKernelGGL(ft_row_kernel, dim3(ip_blocks(w, 256), (unsigned)h, (unsigned)batch), dim3(256), 0, s, (const int*)near_row, index, dist2, h, w);
    return ada_check_launch("ada_nearest_valid_fwd");
}

extern "C" int ada_fill_gather_fwd(const float* x, const uint8_t* valid, const int32_t* index, int32_t batch, int32_t channels, int32_t h, int32_t w,
                                   float empty, float* out, void* stream) {
    ADA_REQUIRE(x && valid && index && out, ADA_EINVAL, "ada_fill_gather_fwd: null pointer");
    if (int rc = check_shape("ada_fill_gather_fwd", batch, channels, h, w)) return rc;
    const long hw = (long)h * w;
    hipLaunchKernelGGL(fill_gather_kernel, dim3(ip_blocks(hw, 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)x, valid, index,
                       channels, hw, __builtin_bit_cast(uint32_t, empty), (uint32_t*)out);
    return ada_check_launch("ada_fill_gather_fwd");
}

extern "C" int ada_push_pull_workspace_bytes(int32_t batch, int32_t channels, int32_t h, int32_t w, int64_t* bytes) {
    ADA_REQUIRE(bytes, ADA_EINVAL, "ada_push_pull_workspace_bytes: null pointer");
    if (int rc = check_shape("ada_push_pull_workspace_bytes", batch, channels, h, w)) return rc;
    *bytes = (int64_t)batch * pp_level_pixels(h, w) * (4 * (int64_t)channels + 1);
    return ADA_OK;
}

extern "C" int ada_push_pull_fwd(const float* x, const uint8_t* valid, int32_t batch, int32_t channels, int32_t h, int32_t w, float empty, float* out,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(x && valid && out, ADA_EINVAL, "ada_push_pull_fwd: null pointer");
    if (int rc = check_shape("ada_push_pull_fwd", batch, channels, h, w)) return rc;
    const int64_t px = pp_level_pixels(h, w);
    const int64_t need = (int64_t)batch * px * (4 * (int64_t)channels + 1);
    ADA_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), ADA_EINVAL, "ada_push_pull_fwd: the workspace needs %ld bytes, got %ld", (long)need,
                (long)(workspace ? workspace_bytes : 0));
    const hipStream_t s = (hipStream_t)stream;
    constexpr int MAX_LEVELS = 16;      // 32767 -> 1 in 15 halvings
    int hs[MAX_LEVELS], wsz[MAX_LEVELS];
    float* lv[MAX_LEVELS];
    uint8_t* lm[MAX_LEVELS];
    float* vals = (float*)workspace;
    uint8_t* masks = (uint8_t*)workspace + (int64_t)4 * batch * channels * px;
    int L = 0;
    hs[0] = h; wsz[0] = w; lv[0] = nullptr; lm[0] = nullptr;
    while (hs[L] > 1 || wsz[L] > 1) {
        hs[L + 1] = (hs[L] + 1) / 2;
        wsz[L + 1] = (wsz[L] + 1) / 2;
        lv[L + 1] = vals;
        lm[L + 1] = masks;
        const int64_t n = (int64_t)hs[L + 1] * wsz[L + 1];
        vals += (int64_t)batch * channels * n;
        masks += (int64_t)batch * n;
        ++L;
    }
    for (int l = 0; l < L; ++l) {
        const long no = (long)hs[l + 1] * wsz[l + 1];
        hipLaunchKernelGGL(pp_pull_kernel, dim3(ip_blocks(no, 256), (unsigned)batch), dim3(256), 0, s, l ? (const float*)lv[l] : x,
                           l ? (const uint8_t*)lm[l] : valid, channels, hs[l], wsz[l], hs[l + 1], wsz[l + 1], lv[l + 1], lm[l + 1], l + 1 == L ? 1 : 0, empty);
    }
    for (int l = L - 1; l >= 1; --l) {
        hipLaunchKernelGGL(pp_push_kernel, dim3(ip_blocks((long)hs[l] * wsz[l], 256), (unsigned)batch), dim3(256), 0, s, (const float*)lv[l],
                           (const uint8_t*)lm[l], (const float*)lv[l + 1], channels, hs[l], wsz[l], hs[l + 1], wsz[l + 1], lv[l], empty);
    }
    hipLaunchKernelGGL(pp_push_kernel, dim3(ip_blocks((long)h * w, 256), (unsigned)batch), dim3(256), 0, s, x, valid, L ? (const float*)lv[1] : (const float*)nullptr,
                       channels, h, w, L ? hs[1] : 1, L ? wsz[1] : 1, out, empty);
    return ada_check_launch("ada_push_pull_fwd");
}
