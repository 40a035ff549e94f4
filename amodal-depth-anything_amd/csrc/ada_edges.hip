// The edge metrics of the reference's evaluation (src/util/metric.py:181-328) on the device: skimage's Canny detector as the reference calls it
// (canny(float32 image, sigma), mode 'constant', no mask), scipy's exact Euclidean distance transform, and the sums behind EdgeAcc / EdgeComp /
// soft_edge_error.  The reference copies two full-size maps per sample to the host and runs all of it there, twice.
//
// ARITHMETIC CONTRACT ("Edge metrics").  skimage keeps every stage of the detector in the image's dtype (float32 here) and scipy's 1-D
// correlations accumulate in double and round when they store.  Every stage below does the same: fp64 accumulation in scipy's order, one rounding to
// fp32 per stored stage, fp32 magnitude in three separately rounded operations, the suppression's weight and interpolation in fp64.  This file is
// built with -ffp-contract=off (csrc/build.py): every product and every sum written here is rounded on its own, as the host's are; no FMA may
// appear.  Divisions and square roots are the correctly rounded ones (no fast-math flag anywhere in the build).
//
// No atomics of this file's own (the hysteresis calls ada_mask_label_fwd, whose integer atomic-min union-find is exact and reproducible), no host
// read, nothing allocated: the launch sequence of every entry point depends on the shapes alone.  No scratch (NO_SCRATCH).
#include "ada_common.h"

#include <math.h>

namespace {

constexpr int ED_T = 32;                        // output tile edge of the detector
constexpr int ED_RMAX = ADA_CANNY_MAX_RADIUS;   // Gaussian radius cap
constexpr int ED_SMAX = ED_T + 2 * (ED_RMAX + 2);   // input tile edge at the cap: smoothing + 1 (Sobel) + 1 (suppression) on each side
constexpr int ED_M = ED_T + 4;                  // smoothed region: the tile and two rings
constexpr int ED_G = ED_T + 2;                  // gradient / magnitude region: the tile and one ring
constexpr float ED_EPS32 = 1.1920928955078125e-07f;

struct CannyArgs {
    const float* img;
    const double* weights;     // device, 2 r + 1
    int h, w, r, pre, tiles_x;
    float low, log15;
    float* low_masked;
    float* pre_out;
    float* smoothed;
    float* isobel;
    float* jsobel;
    float* magnitude;
};

// the reference's maps before the detector: to_log (metric.py:169-173) and extract_edges' default branch (metric.py:206-210); the logarithm is
// evaluated in fp64 from the fp32 value and rounded once
ADA_DEV float ed_pre(float d, int mode, float log15) {
    if (mode == 0) return d;
    const float c = d < ED_EPS32 ? ED_EPS32 : d;      // clamp(min=eps): a NaN passes
    const float pos = d > 0.f ? 1.f : 0.f;
    if (mode == 1) return pos * (float)log((double)c);
    return (float)log((double)(pos * c)) / log15;
}

ADA_DEV int ed_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One workgroup per 32 x 32 output tile; the image is read from HBM once, every stage runs out of LDS.  Local coordinate systems:
//   sA  rows / columns  ty0 - R ..  (R = r + 2)      the pre-transformed image, zero outside the image (mode 'constant')
//   sB  rows ty0 - 2 .., columns tx0 - R ..          after the Gaussian along axis 0
//   sC  rows ty0 - 2 .., columns tx0 - 2 ..          smoothed and normalised; later stages read it at indices CLAMPED INSIDE THE IMAGE, which is
//                                                    scipy's 'reflect' for an offset of one, so positions outside the image are never read
//   sD0 / sD1 (in sA's storage)  as sC               the [-1, 0, 1] correlations along axis 0 / 1
//   sI / sJ / sMag  rows ty0 - 1 .., columns tx0 - 1 ..
__global__ __launch_bounds__(256) void canny_kernel(CannyArgs a) {
    __shared__ float sA[ED_SMAX * ED_SMAX];
    __shared__ float sB[ED_M * ED_SMAX];
    __shared__ float sC[ED_M * ED_M];
    __shared__ float sI[ED_G * ED_G];
    __shared__ float sJ[ED_G * ED_G];
    __shared__ float sMag[ED_G * ED_G];
    __shared__ float sN0[ED_M];
    __shared__ double sW[2 * ED_RMAX + 1];
    const int tid = threadIdx.x;
    const int r = a.r, R = r + 2, S = ED_T + 2 * R;
    const int h = a.h, w = a.w;
    const int ty0 = ((int)blockIdx.x / a.tiles_x) * ED_T, tx0 = ((int)blockIdx.x % a.tiles_x) * ED_T;
    const long base = (long)blockIdx.y * h * w;
    const float* img = a.img + base;

    if (tid < 2 * r + 1) sW[tid] = a.weights[tid];
    for (int i = tid; i < S * S; i += 256) {
        const int ly = i / S, lx = i - ly * S;
        const int gy = ty0 - R + ly, gx = tx0 - R + lx;
        float v = 0.f;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            v = ed_pre(img[(long)gy * w + gx], a.pre, a.log15);
            if (a.pre_out && ly >= R && ly < R + ED_T && lx >= R && lx < R + ED_T) a.pre_out[base + (long)gy * w + gx] = v;
        }
        sA[i] = v;
    }
    __syncthreads();

    // Gaussian along axis 0, scipy's symmetric correlation: centre tap, then the pairs from the outermost inwards, fp64, stored fp32
    for (int i = tid; i < ED_M * S; i += 256) {
        const int my = i / S, lx = i - my * S;
        const float* c = sA + (my + r) * S + lx;
        double t = (double)c[0] * sW[r];
        for (int k = r; k >= 1; --k) t = t + ((double)c[-k * S] + (double)c[k * S]) * sW[r - k];
        sB[i] = (float)t;
    }
    // the same pass over a map of ones: a function of the row alone
    if (tid < ED_M) {
        const int gy = ty0 - 2 + tid;
        double t = sW[r];
        for (int k = r; k >= 1; --k) t = t + ((gy - k >= 0 && gy - k < h ? 1.0 : 0.0) + (gy + k >= 0 && gy + k < h ? 1.0 : 0.0)) * sW[r - k];
        sN0[tid] = (float)t;
    }
    __syncthreads();

    // Gaussian along axis 1, the bleed-over normaliser from the coordinates, and the fp32 division
    for (int i = tid; i < ED_M * ED_M; i += 256) {
        const int my = i / ED_M, mx = i - my * ED_M;
        const int gy = ty0 - 2 + my, gx = tx0 - 2 + mx;
        float s = 0.f;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const float* c = sB + my * S + mx + r;
            const double n0 = (double)sN0[my];
            double t = (double)c[0] * sW[r];
            double n = n0 * sW[r];
            for (int k = r; k >= 1; --k) {
                t = t + ((double)c[-k] + (double)c[k]) * sW[r - k];
                n = n + ((gx - k >= 0 ? n0 : 0.0) + (gx + k < w ? n0 : 0.0)) * sW[r - k];
            }
            const float den = (float)n + ED_EPS32;
            s = (float)t / den;
            if (a.smoothed && my >= 2 && my < 2 + ED_T && mx >= 2 && mx < 2 + ED_T) a.smoothed[base + (long)gy * w + gx] = s;
        }
        sC[i] = s;
    }
    __syncthreads();

    // ndi.sobel's first pass along either axis: weights [-1, 0, 1], scipy's antisymmetric form  in[0] * 0 + (in[-1] - in[+1]) * -1
    float* sD0 = sA;
    float* sD1 = sA + ED_M * ED_M;
    for (int i = tid; i < ED_M * ED_M; i += 256) {
        const int my = i / ED_M, mx = i - my * ED_M;
        const int gy = ty0 - 2 + my, gx = tx0 - 2 + mx;
        float d0 = 0.f, d1 = 0.f;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const int yu = ed_clamp(ed_clamp(gy - 1, 0, h - 1) - (ty0 - 2), 0, ED_M - 1), yd = ed_clamp(ed_clamp(gy + 1, 0, h - 1) - (ty0 - 2), 0, ED_M - 1);
            const int xl = ed_clamp(ed_clamp(gx - 1, 0, w - 1) - (tx0 - 2), 0, ED_M - 1), xr = ed_clamp(ed_clamp(gx + 1, 0, w - 1) - (tx0 - 2), 0, ED_M - 1);
            const double c = (double)sC[i] * 0.0;
            d0 = (float)(c + ((double)sC[yu * ED_M + mx] - (double)sC[yd * ED_M + mx]) * -1.0);
            d1 = (float)(c + ((double)sC[my * ED_M + xl] - (double)sC[my * ED_M + xr]) * -1.0);
        }
        sD0[i] = d0;
        sD1[i] = d1;
    }
    __syncthreads();

    // second pass, weights [1, 2, 1] along the other axis, and the magnitude in three fp32 operations
    for (int i = tid; i < ED_G * ED_G; i += 256) {
        const int py = i / ED_G, px = i - py * ED_G;
        const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
        float gi = 0.f, gj = 0.f, m = 0.f;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            const int my = py + 1, mx = px + 1;
            const int yu = ed_clamp(gy - 1, 0, h - 1) - (ty0 - 2), yd = ed_clamp(gy + 1, 0, h - 1) - (ty0 - 2);      // within my - 1 .. my + 1
            const int xl = ed_clamp(gx - 1, 0, w - 1) - (tx0 - 2), xr = ed_clamp(gx + 1, 0, w - 1) - (tx0 - 2);
            gi = (float)((double)sD0[my * ED_M + mx] * 2.0 + ((double)sD0[my * ED_M + xl] + (double)sD0[my * ED_M + xr]) * 1.0);
            gj = (float)((double)sD1[my * ED_M + mx] * 2.0 + ((double)sD1[yu * ED_M + mx] + (double)sD1[yd * ED_M + mx]) * 1.0);
            m = gi * gi;
            m = m + gj * gj;
            m = sqrtf(m);
            if (py >= 1 && py <= ED_T && px >= 1 && px <= ED_T) {
                const long o = base + (long)gy * w + gx;
                if (a.isobel) a.isobel[o] = gi;
                if (a.jsobel) a.jsobel[o] = gj;
                if (a.magnitude) a.magnitude[o] = m;
            }
        }
        sI[i] = gi;
        sJ[i] = gj;
        sMag[i] = m;
    }
    __syncthreads();

    // skimage's bilinear non-maximum suppression: off the border ring, magnitude >= low, the sector from the signs and |isobel| vs |jsobel|, the weight
    // and both interpolations in fp64, kept when both are <= the pixel's magnitude.  Both derivatives zero: w = 0 / 0 = NaN, nothing is <= : dropped.
    for (int i = tid; i < ED_T * ED_T; i += 256) {
        const int ly = i / ED_T, lx = i - ly * ED_T;
        const int gy = ty0 + ly, gx = tx0 + lx;
        if (gy >= h || gx >= w) continue;
        float out = 0.f;
        const int p = (ly + 1) * ED_G + lx + 1;
        const float m = sMag[p];
        if (gy >= 1 && gy < h - 1 && gx >= 1 && gx < w - 1 && m >= a.low) {
            const float gi = sI[p], gj = sJ[p];
            const bool down = gi <= 0.f, up = gi >= 0.f, left = gj <= 0.f, right = gj >= 0.f;
            const bool cond1 = (up && right) || (down && left), cond2 = (down && right) || (up && left);
            if (cond1 || cond2) {
                const double ai = (double)__builtin_fabsf(gi), aj = (double)__builtin_fabsf(gj);
                // offsets (rows, columns) of the first neighbour pair; the second pair is its mirror image
                int y1, x1, y2, x2;
                double wgt;
                if (cond1) {
                    if (ai > aj) { wgt = aj / ai; y1 = 1; x1 = 0; y2 = 1; x2 = 1; }
                    else         { wgt = ai / aj; y1 = 0; x1 = 1; y2 = 1; x2 = 1; }
                } else {
                    if (ai < aj) { wgt = ai / aj; y1 = 0; x1 = 1; y2 = -1; x2 = 1; }
                    else         { wgt = aj / ai; y1 = -1; x1 = 0; y2 = -1; x2 = 1; }
                }
                const double n11 = (double)sMag[p + y1 * ED_G + x1], n12 = (double)sMag[p + y2 * ED_G + x2];
                const double n21 = (double)sMag[p - y1 * ED_G - x1], n22 = (double)sMag[p - y2 * ED_G - x2];
                const double one_w = 1.0 - wgt;
                const bool c_plus = n12 * wgt + n11 * one_w <= (double)m;
                const bool c_minus = n22 * wgt + n21 * one_w <= (double)m;
                if (c_plus && c_minus) out = m;
            }
        }
        a.low_masked[base + (long)gy * w + gx] = out;
    }
}

// ---- hysteresis ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hyst_mask_kernel(const float* low_masked, uint8_t* mask, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) mask[i] = low_masked[i] > 0.f ? 1 : 0;
}

__global__ __launch_bounds__(256) void hyst_zero_kernel(uint8_t* flags, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = 0;
}

// every writer of a flag stores the same byte: plain stores, no atomic
__global__ __launch_bounds__(256) void hyst_flag_kernel(const float* low_masked, const int* labels, float high, uint8_t* flags, long hw, long nflags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const long o = (long)blockIdx.y * hw + i;
    const int l = labels[o];
    if (l > 0 && l < nflags && low_masked[o] >= high) flags[(long)blockIdx.y * nflags + l] = 1;
}

__global__ __launch_bounds__(256) void hyst_gather_kernel(const int* labels, const uint8_t* flags, uint8_t* out, long hw, long nflags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const long o = (long)blockIdx.y * hw + i;
    const int l = labels[o];
    out[o] = (l > 0 && l < nflags) ? flags[(long)blockIdx.y * nflags + l] : 0;
}

// ---- exact Euclidean distance transform ------------------------------------------------------------------------------------------------------
constexpr int EDT_NONE = 0x7fffffff;      // no edge pixel in this column
constexpr int EDT_CHUNK = 1024;           // squared column distances of one row staged per step

// one thread per column: squared distance to the nearest edge pixel of the column, two scans
__global__ __launch_bounds__(256) void edt_col_kernel(const uint8_t* edges, int* g2, int h, int w) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    const long base = (long)blockIdx.y * h * w + x;
    int d = EDT_NONE;
    for (int y = 0; y < h; ++y) {
        const long o = base + (long)y * w;
        d = edges[o] ? 0 : (d == EDT_NONE ? EDT_NONE : d + 1);
        g2[o] = d;
    }
    d = EDT_NONE;
    for (int y = h - 1; y >= 0; --y) {
        const long o = base + (long)y * w;
        const int dn = g2[o];
        d = dn == 0 ? 0 : (d == EDT_NONE ? EDT_NONE : d + 1);
        const int m = d < dn ? d : dn;
        g2[o] = m == EDT_NONE ? EDT_NONE : m * m;
    }
}

// grid (ceil(w / 256), h, batch): min over x' of (x - x')^2 + g2[x'], exact in 32 bits (h, w <= 32767), then one fp64 square root
__global__ __launch_bounds__(256) void edt_row_kernel(const int* g2, double* out, int h, int w) {
    __shared__ int s[EDT_CHUNK];
    const int x = blockIdx.x * 256 + threadIdx.x;
    const long row = ((long)blockIdx.z * h + blockIdx.y) * w;
    unsigned best = 0xffffffffu;
    for (int c0 = 0; c0 < w; c0 += EDT_CHUNK) {
        const int n = w - c0 < EDT_CHUNK ? w - c0 : EDT_CHUNK;
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += 256) s[j] = g2[row + c0 + j];
        __syncthreads();
        if (x < w) {
            const int nd = x < c0 ? c0 - x : (x >= c0 + n ? x - (c0 + n - 1) : 0);     // the chunk's nearest column
            if ((unsigned)(nd * nd) < best) {
                for (int j = 0; j < n; ++j) {
                    const int dx = x - (c0 + j);
                    const unsigned d = (unsigned)(dx * dx) + (unsigned)s[j];      // EDT_NONE + dx^2 stays below 2^32 and above every real distance
                    best = d < best ? d : best;
                }
            }
        }
    }
    if (x < w) out[row + x] = best >= (unsigned)EDT_NONE ? (double)INFINITY : sqrt((double)best);
}

// ---- sums ------------------------------------------------------------------------------------------------------------------------------------
constexpr int SUM_BLOCKS = ADA_EDGE_SUM_BLOCKS;     // partial rows per image

// Fixed-order reduction of K per-thread doubles over a workgroup of 256: shuffle tree inside each wave, then the four waves in order.
template <int K>
ADA_DEV void block_partials(double (&s)[K], double* dst) {
    __shared__ double part[4][K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s[i] += __shfl_xor(s[i], o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < K; ++i) part[threadIdx.x >> 6][i] = s[i];
    }
    __syncthreads();
    if (threadIdx.x < K) dst[threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void edge_sum_kernel(const uint8_t* pred_e, const uint8_t* gt_e, const uint8_t* valid, const double* d_target,
                                                       const double* d_pred, double th, long n, double* partial) {
    const long base = (long)blockIdx.y * n;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long o = base + i;
        if (valid && !valid[o]) continue;
        if (pred_e[o]) {
            const double dt = d_target[o];
            if (dt < th) { s[0] += 1.0; s[1] += dt; }
        }
        if (gt_e[o]) { s[2] += 1.0; s[3] += d_pred[o]; }
    }
    block_partials<4>(s, partial + ((long)blockIdx.y * SUM_BLOCKS + blockIdx.x) * 4);
}

// min over the (2 r + 1)^2 shifts of |shift(gt) - pred|, the shifted map 0 where it came from outside (shift_2d_replace, constant = 0); fp32
// difference and absolute value as numpy's on float32 arrays, np.minimum's NaN propagation
__global__ __launch_bounds__(256) void soft_edge_kernel(const float* pred, const float* gt, const uint8_t* valid, int h, int w, int radius, double* partial) {
    const long n = (long)h * w;
    const long base = (long)blockIdx.y * n;
    double s[2] = {0.0, 0.0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        if (valid && !valid[base + i]) continue;
        const int y = (int)(i / w), x = (int)(i - (long)y * w);
        const float p = pred[base + i];
        float m = INFINITY;
        for (int dy = -radius; dy <= radius; ++dy) {
            const int yy = y + dy;
            const bool row_in = yy >= 0 && yy < h;
            for (int dx = -radius; dx <= radius; ++dx) {
                const int xx = x + dx;
                const float g = (row_in && xx >= 0 && xx < w) ? gt[base + (long)yy * w + xx] : 0.f;
                const float e = __builtin_fabsf(g - p);
                m = (e < m || e != e) ? e : m;
            }
        }
        s[0] += 1.0;
        s[1] += (double)m;
    }
    block_partials<2>(s, partial + ((long)blockIdx.y * SUM_BLOCKS + blockIdx.x) * 2);
}

// one workgroup per image: partial row t to thread t, a fixed tree over LDS
template <int K>
__global__ __launch_bounds__(256) void final_sum_kernel(const double* partial, int rows, double* out) {
    __shared__ double t[SUM_BLOCKS][K];
    static_assert(SUM_BLOCKS == 256, "one partial row per thread");
    const double* p = partial + (long)blockIdx.x * SUM_BLOCKS * K;
#pragma unroll
    for (int i = 0; i < K; ++i) t[threadIdx.x][i] = (int)threadIdx.x < rows ? p[threadIdx.x * K + i] : 0.0;
    __syncthreads();
    for (int o = SUM_BLOCKS / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int i = 0; i < K; ++i) t[threadIdx.x][i] += t[threadIdx.x + o][i];
        }
        __syncthreads();
    }
    if (threadIdx.x < K) out[(long)blockIdx.x * K + threadIdx.x] = t[0][threadIdx.x];
}

unsigned ed_blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }

int sum_rows(long n) {
    long b = (n + 256 * 8 - 1) / (256 * 8);      // ~8 pixels per thread
    return (int)(b > SUM_BLOCKS ? SUM_BLOCKS : (b < 1 ? 1 : b));
}

int check_maps(const char* who, int32_t batch, int32_t h, int32_t w) {
    ADA_REQUIRE(batch > 0 && h > 0 && w > 0, ADA_EINVAL, "%s: bad shape batch=%d %dx%d", who, batch, h, w);
    ADA_REQUIRE((int64_t)h * w < ((int64_t)1 << 31) && batch <= 65535, ADA_EUNSUPPORTED, "%s: h * w must stay below 2^31 and batch within 65535", who);
    return ADA_OK;
}

// label map, component counts, the flags of labels 0 .. ceil(h w / 2) (+ slack, padded to 4 bytes), the 0 / 1 mask and the labeller's own workspace
int64_t hyst_flags_per_image(int64_t hw) { return ((hw / 2 + 2) + 3) / 4 * 4; }
int64_t label_ws_bytes(int64_t batch, int64_t hw) { return 4 * batch * (2 * hw + (hw + 1023) / 1024); }
int64_t hyst_ws_bytes(int64_t batch, int64_t hw) {
    return 4 * batch * hw + 4 * batch + label_ws_bytes(batch, hw) + batch * hyst_flags_per_image(hw) + (batch * hw + 3) / 4 * 4;
}

}  // namespace

extern "C" int ada_canny_fwd(const float* image, int32_t batch, int32_t h, int32_t w, int32_t pre, const double* weights, int32_t radius,
                             float low_threshold, float* low_masked, float* pre_out, float* smoothed, float* isobel, float* jsobel,
                             float* magnitude, void* stream) {
    ADA_REQUIRE(image && weights && low_masked, ADA_EINVAL, "ada_canny_fwd: null pointer");
    if (int rc = check_maps("ada_canny_fwd", batch, h, w)) return rc;
    ADA_REQUIRE(pre >= 0 && pre <= 2, ADA_EINVAL, "ada_canny_fwd: pre-transform %d (0 identity, 1 log, 2 log base 1.5)", pre);
    ADA_REQUIRE(radius >= 0 && radius <= ED_RMAX, ADA_EUNSUPPORTED, "ada_canny_fwd: Gaussian radius %d outside 0 .. %d", radius, ED_RMAX);
    CannyArgs a;
    a.img = image; a.weights = weights; a.h = h; a.w = w; a.r = radius; a.pre = pre; a.tiles_x = (w + ED_T - 1) / ED_T;
    a.low = low_threshold; a.log15 = (float)log(1.5);
    a.low_masked = low_masked; a.pre_out = pre_out; a.smoothed = smoothed; a.isobel = isobel; a.jsobel = jsobel; a.magnitude = magnitude;
    const long tiles = (long)a.tiles_x * ((h + ED_T - 1) / ED_T);
    hipLaunchKernelGGL(canny_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    return ada_check_launch("ada_canny_fwd");
}

extern "C" int ada_canny_hysteresis_fwd(const float* low_masked, int32_t batch, int32_t h, int32_t w, float high_threshold, uint8_t* edges,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(low_masked && edges, ADA_EINVAL, "ada_canny_hysteresis_fwd: null pointer");
    if (int rc = check_maps("ada_canny_hysteresis_fwd", batch, h, w)) return rc;
    const int64_t hw = (int64_t)h * w;
    const int64_t need = hyst_ws_bytes(batch, hw);
    ADA_REQUIRE(workspace && workspace_bytes >= need, ADA_EINVAL, "ada_canny_hysteresis_fwd: the workspace needs %ld bytes, got %ld", (long)need,
                (long)(workspace ? workspace_bytes : 0));
    const hipStream_t s = (hipStream_t)stream;
    const int64_t nflags = hyst_flags_per_image(hw);
    int* labels = (int*)workspace;
    int* n_labels = labels + batch * hw;
    char* label_ws = (char*)(n_labels + batch);
    uint8_t* flags = (uint8_t*)(label_ws + label_ws_bytes(batch, hw));
    uint8_t* mask = flags + batch * nflags;
    hipLaunchKernelGGL(hyst_mask_kernel, dim3(ed_blocks(batch * hw, 256)), dim3(256), 0, s, low_masked, mask, (long)(batch * hw));
    // skimage: ndi.label(low_mask, np.ones((3, 3))) -- the 8-connected labeller of the mask front-end
    if (int rc = ada_mask_label_fwd(mask, batch, h, w, w, hw, 8, labels, n_labels, label_ws, label_ws_bytes(batch, hw), stream)) return rc;
    hipLaunchKernelGGL(hyst_zero_kernel, dim3(ed_blocks(batch * nflags, 256)), dim3(256), 0, s, flags, (long)(batch * nflags));
    hipLaunchKernelGGL(hyst_flag_kernel, dim3(ed_blocks(hw, 256), (unsigned)batch), dim3(256), 0, s, low_masked, (const int*)labels, high_threshold, flags,
                       (long)hw, (long)nflags);
    hipLaunchKernelGGL(hyst_gather_kernel, dim3(ed_blocks(hw, 256), (unsigned)batch), dim3(256), 0, s, (const int*)labels, (const uint8_t*)flags, edges,
                       (long)hw, (long)nflags);
    return ada_check_launch("ada_canny_hysteresis_fwd");
}

extern "C" int ada_edt_fwd(const uint8_t* edges, int32_t batch, int32_t h, int32_t w, double* out, void* workspace, int64_t workspace_bytes,
                           void* stream) {
    ADA_REQUIRE(edges && out, ADA_EINVAL, "ada_edt_fwd: null pointer");
    if (int rc = check_maps("ada_edt_fwd", batch, h, w)) return rc;
    ADA_REQUIRE(h <= 32767 && w <= 32767, ADA_EUNSUPPORTED, "ada_edt_fwd: h and w must stay within 32767 (squared distances are exact in 32 bits), got %dx%d", h, w);
    const int64_t need = (int64_t)4 * batch * h * w;
    ADA_REQUIRE(workspace && workspace_bytes >= need, ADA_EINVAL, "ada_edt_fwd: the workspace needs %ld bytes, got %ld", (long)need,
                (long)(workspace ? workspace_bytes : 0));
    const hipStream_t s = (hipStream_t)stream;
    int* g2 = (int*)workspace;
    hipLaunchKernelGGL(edt_col_kernel, dim3(ed_blocks(w, 256), (unsigned)batch), dim3(256), 0, s, edges, g2, h, w);
    hipLaunchKernelGGL(edt_row_kernel, dim3(ed_blocks(w, 256), (unsigned)h, (unsigned)batch), dim3(256), 0, s, (const int*)g2, out, h, w);
    return ada_check_launch("ada_edt_fwd");
}

extern "C" int ada_edge_metric_fwd(const uint8_t* pred_edges, const uint8_t* gt_edges, const uint8_t* valid, const double* d_target,
                                   const double* d_pred, int32_t batch, int32_t h, int32_t w, double th_acc, double* sums, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(pred_edges && gt_edges && d_target && d_pred && sums, ADA_EINVAL, "ada_edge_metric_fwd: null pointer");
    if (int rc = check_maps("ada_edge_metric_fwd", batch, h, w)) return rc;
    const int64_t need = (int64_t)8 * batch * SUM_BLOCKS * 4;
    ADA_REQUIRE(workspace && workspace_bytes >= need, ADA_EINVAL, "ada_edge_metric_fwd: the workspace needs %ld bytes, got %ld", (long)need,
                (long)(workspace ? workspace_bytes : 0));
    const long n = (long)h * w;
    const int rows = sum_rows(n);
    hipLaunchKernelGGL(edge_sum_kernel, dim3((unsigned)rows, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, pred_edges, gt_edges, valid, d_target,
                       d_pred, th_acc, n, (double*)workspace);
    hipLaunchKernelGGL(final_sum_kernel<4>, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, rows, sums);
    return ada_check_launch("ada_edge_metric_fwd");
}

extern "C" int ada_soft_edge_fwd(const float* pred, const float* gt, const uint8_t* valid, int32_t batch, int32_t h, int32_t w, int32_t radius,
                                 double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(pred && gt && sums, ADA_EINVAL, "ada_soft_edge_fwd: null pointer");
    if (int rc = check_maps("ada_soft_edge_fwd", batch, h, w)) return rc;
    ADA_REQUIRE(radius >= 0 && radius <= ADA_SOFT_EDGE_MAX_RADIUS, ADA_EUNSUPPORTED, "ada_soft_edge_fwd: radius %d outside 0 .. %d", radius,
                ADA_SOFT_EDGE_MAX_RADIUS);
    const int64_t need = (int64_t)8 * batch * SUM_BLOCKS * 2;
    ADA_REQUIRE(workspace && workspace_bytes >= need, ADA_EINVAL, "ada_soft_edge_fwd: the workspace needs %ld bytes, got %ld", (long)need,
                (long)(workspace ? workspace_bytes : 0));
    const long n = (long)h * w;
    const int rows = sum_rows(n);
    hipLaunchKernelGGL(soft_edge_kernel, dim3((unsigned)rows, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, pred, gt, valid, h, w, radius,
                       (double*)workspace);
    hipLaunchKernelGGL(final_sum_kernel<2>, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, rows, sums);
    return ada_check_launch("ada_soft_edge_fwd");
}
