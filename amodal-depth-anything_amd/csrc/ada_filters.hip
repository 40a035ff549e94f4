// Rank filters on the device: the windowed order statistic of the valid samples (include/ada_hip.h, "Rank filters").  Median, minimum (erosion) and
// maximum (dilation) are ranks of it.  Two kernel families:
//   rank_kernel                     any rank of a window of up to ADA_FILTER_MAX_WINDOW samples: tile + halo staged into LDS once as order-preserving
//                                   keys, then a bitwise selection per thread -- the largest key v such that at most r keys of the window lie below v
//                                   is s[r]; every bit is decided by one pass over the window in LDS.
//   ext_row_kernel, ext_col_kernel  minimum / maximum of windows up to ADA_FILTER_MAX_EXTREME on a side, separably: the minimum of minima is exact and
//                                   the box sum of the validity bits is an integer sum.
//
// KEYS.  An fp32 becomes its bits with the sign bit flipped (all bits flipped when negative): unsigned comparison of keys is IEEE comparison of the
// values, with -0 just below +0.  A uint8 is its own key.  RF_NONE = 0xffffffff marks a sample that does not vote (invalid, NaN, dropped by the
// border rule); it is the key of a NaN pattern, so no voting fp32 and no uint8 maps to it, and it compares above every candidate of the selection.
// The maximum runs as the minimum of the complemented keys: all 32 bits of an fp32's key (~key == RF_NONE would need key == 0, again a NaN's), the low
// eight of a uint8's (255 - v; all 32 would turn v == 0 into RF_NONE).
//
// Nothing here is rounded: values are only compared and copied.  No atomics, no host read, nothing allocated, one fixed grid per launch derived from
// the shapes.  Trip counts depend on (kh, kw) alone.  No per-thread array: the window lives in LDS (NO_SCRATCH).
#include "ada_common.h"

namespace {

constexpr int RF_TW = ADA_FILTER_TILE_W;         // outputs per workgroup: RF_TH rows of RF_TW, one per thread; a wave reads 64 consecutive LDS words
constexpr int RF_TH = ADA_FILTER_TILE_H;
constexpr int RF_CH = ADA_FILTER_COL_TILE_H;     // rows per workgroup of the column pass, RF_CH / RF_TH per thread
constexpr int RF_KMAX = ADA_FILTER_MAX_EXTREME;
constexpr uint32_t RF_NONE = 0xffffffffu;

// LDS words of the rank kernel: the largest (RF_TH - 1 + kh) (RF_TW - 1 + kw) over the odd windows with kh kw <= ADA_FILTER_MAX_WINDOW
constexpr int rf_lds_words() {
    int best = 0;
    for (int kh = 1; kh <= ADA_FILTER_MAX_WINDOW; kh += 2)
        for (int kw = 1; kh * kw <= ADA_FILTER_MAX_WINDOW; kw += 2) {
            const int n = (RF_TH - 1 + kh) * (RF_TW - 1 + kw);
            best = n > best ? n : best;
        }
    return best;
}
constexpr int RF_LDS = rf_lds_words();
static_assert(RF_TW * RF_TH == 256 && RF_TW == 64 && RF_CH % RF_TH == 0, "one output per thread, one tile row per wave");
static_assert(RF_LDS * 4 <= 64 * 1024, "the rank kernel's tile must fit a workgroup's LDS");

ADA_DEV uint32_t rf_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return v != v ? RF_NONE : u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
ADA_DEV uint32_t rf_key(uint8_t v) { return v; }
ADA_DEV void rf_store(float* p, uint32_t k) { *p = __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }
ADA_DEV void rf_store(uint8_t* p, uint32_t k) { *p = (uint8_t)k; }
ADA_DEV void rf_store_bits(float* p, uint32_t bits) { *p = __uint_as_float(bits); }
ADA_DEV void rf_store_bits(uint8_t* p, uint32_t bits) { *p = (uint8_t)bits; }
template <typename T> struct RfTop;
template <> struct RfTop<float> { static constexpr uint32_t bit = 0x80000000u, all = 0xffffffffu; };      // the key's top bit, all of its bits
template <> struct RfTop<uint8_t> { static constexpr uint32_t bit = 0x80u, all = 0xffu; };

// the image index a window position maps to along one axis of n samples, -1 when the border rule drops it
ADA_DEV int rf_map(int i, int n, int border) {
    if ((unsigned)i < (unsigned)n) return i;
    if (border == ADA_BORDER_IGNORE) return -1;
    if (border == ADA_BORDER_NEAREST) return i < 0 ? 0 : n - 1;
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

struct FilterArgs {
    const void* x;
    const uint8_t* valid;
    void* out;
    int32_t* count;
    uint32_t* tmp_key;      // the extremes' row pass -> column pass
    uint8_t* tmp_n;
    int h, w, kh, kw, rank, border, tiles_x, flip;
    uint32_t fill_bits;
};

// the key of image position (gy, gx), both already mapped (-1: dropped); flip complements a voting key (the maximum as a minimum)
template <typename T>
ADA_DEV uint32_t rf_fetch(const T* x, const uint8_t* valid, int gy, int gx, int w, uint32_t flip) {
    if (gy < 0 || gx < 0) return RF_NONE;
    const int64_t o = (int64_t)gy * w + gx;
    if (valid && !valid[o]) return RF_NONE;
    const uint32_t k = rf_key(x[o]);
    return k == RF_NONE ? k : k ^ flip;
}

// KW: the window's width when it is one of the instantiated ones (the inner loop unrolls), 0 = a.kw
template <typename T, int KW>
__global__ __launch_bounds__(256) void rank_kernel(FilterArgs a) {
    __shared__ uint32_t sK[RF_LDS];
    const int kh = a.kh, kw = KW ? KW : a.kw;
    const int rh = kh >> 1, rw = kw >> 1;
    const int ty0 = ((int)blockIdx.x / a.tiles_x) * RF_TH, tx0 = ((int)blockIdx.x % a.tiles_x) * RF_TW;
    const int64_t base = (int64_t)blockIdx.y * a.h * a.w;
    const T* x = (const T*)a.x + base;
    const uint8_t* valid = a.valid ? a.valid + base : nullptr;
    const int sw = RF_TW + kw - 1, sh = RF_TH + kh - 1;      // sw * sh <= RF_LDS: the launcher checked kh * kw
    for (int i = threadIdx.x; i < sw * sh; i += 256) {
        const int ly = i / sw, lx = i - ly * sw;
        sK[i] = rf_fetch(x, valid, rf_map(ty0 - rh + ly, a.h, a.border), rf_map(tx0 - rw + lx, a.w, a.border), a.w, 0u);
    }
    __syncthreads();
    const int lx = threadIdx.x & (RF_TW - 1), ly = threadIdx.x / RF_TW;
    const uint32_t* win = sK + ly * sw + lx;      // the window's top-left sample; every thread's window lies inside the staged tile
    int n = 0;
    for (int dy = 0; dy < kh; ++dy)
        for (int dx = 0; dx < kw; ++dx) n += win[dy * sw + dx] != RF_NONE;
    const int r = a.rank == ADA_RANK_MIN ? 0 : a.rank == ADA_RANK_MAX ? n - 1 : a.rank == ADA_RANK_MEDIAN ? n / 2 : (a.rank * (n - 1)) / 100;
    uint32_t sel = 0;
    for (uint32_t bit = RfTop<T>::bit; bit; bit >>= 1) {
        const uint32_t cand = sel | bit;
        int below = 0;
        for (int dy = 0; dy < kh; ++dy)
            for (int dx = 0; dx < kw; ++dx) below += win[dy * sw + dx] < cand;
        if (below <= r) sel = cand;
    }
    const int gy = ty0 + ly, gx = tx0 + lx;
    if (gy < a.h && gx < a.w) {
        const int64_t o = base + (int64_t)gy * a.w + gx;
        if (n) rf_store((T*)a.out + o, sel);
        else rf_store_bits((T*)a.out + o, a.fill_bits);
        if (a.count) a.count[o] = n;
    }
}

// rows: per pixel the minimum key (complemented keys for the maximum) and the number of voting samples among its kw row neighbours
template <typename T>
__global__ __launch_bounds__(256) void ext_row_kernel(FilterArgs a) {
    __shared__ uint32_t sK[RF_TH * (RF_TW + RF_KMAX - 1)];
    const int kw = a.kw, rw = kw >> 1;
    const int ty0 = ((int)blockIdx.x / a.tiles_x) * RF_TH, tx0 = ((int)blockIdx.x % a.tiles_x) * RF_TW;
    const int64_t base = (int64_t)blockIdx.y * a.h * a.w;
    const T* x = (const T*)a.x + base;
    const uint8_t* valid = a.valid ? a.valid + base : nullptr;
    const int sw = RF_TW + kw - 1;
    const uint32_t flip = a.flip ? RfTop<T>::all : 0u;
    for (int i = threadIdx.x; i < sw * RF_TH; i += 256) {
        const int ly = i / sw, lx = i - ly * sw;
        const int gy = ty0 + ly;
        sK[i] = rf_fetch(x, valid, gy < a.h ? gy : -1, rf_map(tx0 - rw + lx, a.w, a.border), a.w, flip);
    }
    __syncthreads();
    const int lx = threadIdx.x & (RF_TW - 1), ly = threadIdx.x / RF_TW;
    const uint32_t* win = sK + ly * sw + lx;
    uint32_t best = RF_NONE;
    int n = 0;
    for (int dx = 0; dx < kw; ++dx) {
        const uint32_t k = win[dx];
        best = k < best ? k : best;
        n += k != RF_NONE;
    }
    const int gy = ty0 + ly, gx = tx0 + lx;
    if (gy < a.h && gx < a.w) {
        const int64_t o = base + (int64_t)gy * a.w + gx;
        a.tmp_key[o] = best;
        a.tmp_n[o] = (uint8_t)n;      // n <= kw <= 63
    }
}

// columns: the minimum of kh row minima and the sum of their counts, rows mapped by the border rule (a clamped or mirrored row counts once per
// position, as the contract's multiset does)
template <typename T>
__global__ __launch_bounds__(256) void ext_col_kernel(FilterArgs a) {
    __shared__ uint32_t sK[(RF_CH + RF_KMAX - 1) * RF_TW];
    __shared__ uint8_t sN[(RF_CH + RF_KMAX - 1) * RF_TW];
    const int kh = a.kh, rh = kh >> 1;
    const int ty0 = ((int)blockIdx.x / a.tiles_x) * RF_CH, tx0 = ((int)blockIdx.x % a.tiles_x) * RF_TW;
    const int64_t base = (int64_t)blockIdx.y * a.h * a.w;
    const int sh = RF_CH + kh - 1;
    const int lx = threadIdx.x & (RF_TW - 1), q = threadIdx.x / RF_TW;
    const int gx = tx0 + lx;
    for (int ly = q; ly < sh; ly += RF_TH) {
        const int gy = rf_map(ty0 - rh + ly, a.h, a.border);
        uint32_t k = RF_NONE;
        uint8_t c = 0;
        if (gy >= 0 && gx < a.w) {
            const int64_t o = base + (int64_t)gy * a.w + gx;
            k = a.tmp_key[o];
            c = a.tmp_n[o];
        }
        sK[ly * RF_TW + lx] = k;
        sN[ly * RF_TW + lx] = c;
    }
    __syncthreads();
    const uint32_t flip = a.flip ? RfTop<T>::all : 0u;
    for (int ly = q; ly < RF_CH; ly += RF_TH) {
        uint32_t best = RF_NONE;
        int n = 0;
        for (int dy = 0; dy < kh; ++dy) {
            const uint32_t k = sK[(ly + dy) * RF_TW + lx];
            best = k < best ? k : best;
            n += sN[(ly + dy) * RF_TW + lx];
        }
        const int gy = ty0 + ly;
        if (gy < a.h && gx < a.w) {
            const int64_t o = base + (int64_t)gy * a.w + gx;
            if (n) rf_store((T*)a.out + o, best ^ flip);
            else rf_store_bits((T*)a.out + o, a.fill_bits);
            if (a.count) a.count[o] = n;
        }
    }
}

// the arguments both entry points share; fills everything of FilterArgs but the temporaries
int filter_args(const char* who, const void* x, const uint8_t* valid, int32_t dtype, int32_t batch, int32_t h, int32_t w, int32_t kh, int32_t kw,
                int32_t rank, int32_t border, double fill, void* out, int32_t* count, FilterArgs& a) {
    ADA_REQUIRE(x && out, ADA_EINVAL, "%s: null pointer", who);
    ADA_REQUIRE(dtype == ADA_DT_F32 || dtype == ADA_DT_U8, ADA_EINVAL, "%s: dtype %d (ADA_DT_F32 or ADA_DT_U8)", who, dtype);
    ADA_REQUIRE(batch > 0 && h > 0 && w > 0, ADA_EINVAL, "%s: bad shape batch=%d %dx%d", who, batch, h, w);
    ADA_REQUIRE((int64_t)h * w < ((int64_t)1 << 31) && batch <= 65535, ADA_EUNSUPPORTED, "%s: h * w must stay below 2^31 and batch within 65535", who);
    ADA_REQUIRE(kh > 0 && kw > 0 && (kh & 1) && (kw & 1), ADA_EINVAL, "%s: the window must have odd positive sides, got %dx%d", who, kh, kw);
    ADA_REQUIRE(border == ADA_BORDER_MIRROR || border == ADA_BORDER_NEAREST || border == ADA_BORDER_IGNORE, ADA_EINVAL, "%s: border rule %d", who, border);
    ADA_REQUIRE((rank >= 0 && rank <= 100) || rank == ADA_RANK_MIN || rank == ADA_RANK_MEDIAN || rank == ADA_RANK_MAX, ADA_EINVAL,
                "%s: rank %d (a percent 0 .. 100 or ADA_RANK_MIN / _MEDIAN / _MAX)", who, rank);
    a.x = x; a.valid = valid; a.out = out; a.count = count; a.tmp_key = nullptr; a.tmp_n = nullptr;
    a.h = h; a.w = w; a.kh = kh; a.kw = kw; a.rank = rank; a.border = border; a.tiles_x = (w + RF_TW - 1) / RF_TW; a.flip = 0;
    if (dtype == ADA_DT_U8) {
        ADA_REQUIRE(fill >= 0.0 && fill <= 255.0 && fill == (double)(int)fill, ADA_EINVAL, "%s: the fill of a uint8 map must be an integer in 0 .. 255", who);
        a.fill_bits = (uint32_t)(int)fill;
    } else {
        const float f = (float)fill;
        __builtin_memcpy(&a.fill_bits, &f, 4);
    }
    return ADA_OK;
}

template <typename T>
void launch_rank(const FilterArgs& a, dim3 grid, hipStream_t s) {
    switch (a.kw) {
        case 3: hipLaunchKernelGGL((rank_kernel<T, 3>), grid, dim3(256), 0, s, a); break;
        case 5: hipLaunchKernelGGL((rank_kernel<T, 5>), grid, dim3(256), 0, s, a); break;
        case 7: hipLaunchKernelGGL((rank_kernel<T, 7>), grid, dim3(256), 0, s, a); break;
        case 9: hipLaunchKernelGGL((rank_kernel<T, 9>), grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((rank_kernel<T, 0>), grid, dim3(256), 0, s, a); break;
    }
}

}  // namespace

extern "C" int ada_rank_filter_fwd(const void* x, const uint8_t* valid, int32_t dtype, int32_t batch, int32_t h, int32_t w, int32_t kh, int32_t kw,
                                   int32_t rank, int32_t border, double fill, void* out, int32_t* count, void* stream) {
    FilterArgs a;
    if (int rc = filter_args("ada_rank_filter_fwd", x, valid, dtype, batch, h, w, kh, kw, rank, border, fill, out, count, a)) return rc;
    ADA_REQUIRE((int64_t)kh * kw <= ADA_FILTER_MAX_WINDOW, ADA_EINVAL, "ada_rank_filter_fwd: a window of %dx%d holds more than %d samples", kh, kw,
                ADA_FILTER_MAX_WINDOW);
    const dim3 grid((unsigned)(a.tiles_x * ((h + RF_TH - 1) / RF_TH)), (unsigned)batch);
    if (dtype == ADA_DT_U8) launch_rank<uint8_t>(a, grid, (hipStream_t)stream);
    else launch_rank<float>(a, grid, (hipStream_t)stream);
    return ada_check_launch("ada_rank_filter_fwd");
}

extern "C" int ada_extreme_filter_fwd(const void* x, const uint8_t* valid, int32_t dtype, int32_t batch, int32_t h, int32_t w, int32_t kh, int32_t kw,
                                      int32_t rank, int32_t border, double fill, void* out, int32_t* count, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
    FilterArgs a;
    if (int rc = filter_args("ada_extreme_filter_fwd", x, valid, dtype, batch, h, w, kh, kw, rank, border, fill, out, count, a)) return rc;
    ADA_REQUIRE(rank == ADA_RANK_MIN || rank == ADA_RANK_MAX, ADA_EINVAL, "ada_extreme_filter_fwd: rank %d (ADA_RANK_MIN or ADA_RANK_MAX)", rank);
    ADA_REQUIRE(kh <= RF_KMAX && kw <= RF_KMAX, ADA_EINVAL, "ada_extreme_filter_fwd: a window of %dx%d exceeds %d on a side", kh, kw, RF_KMAX);
    const int64_t n = (int64_t)batch * h * w;
    ADA_REQUIRE(workspace && workspace_bytes >= 5 * n && ((uintptr_t)workspace & 3) == 0, ADA_EINVAL,
                "ada_extreme_filter_fwd: the workspace needs %ld bytes, 4-byte aligned, got %ld", (long)(5 * n), (long)(workspace ? workspace_bytes : 0));
    a.tmp_key = (uint32_t*)workspace;
    a.tmp_n = (uint8_t*)(a.tmp_key + n);
    a.flip = rank == ADA_RANK_MAX;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 rows((unsigned)(a.tiles_x * ((h + RF_TH - 1) / RF_TH)), (unsigned)batch), cols((unsigned)(a.tiles_x * ((h + RF_CH - 1) / RF_CH)), (unsigned)batch);
    if (dtype == ADA_DT_U8) {
        hipLaunchKernelGGL(ext_row_kernel<uint8_t>, rows, dim3(256), 0, s, a);
        hipLaunchKernelGGL(ext_col_kernel<uint8_t>, cols, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(ext_row_kernel<float>, rows, dim3(256), 0, s, a);
        hipLaunchKernelGGL(ext_col_kernel<float>, cols, dim3(256), 0, s, a);
    }
    return ada_check_launch("ada_extreme_filter_fwd");
}
