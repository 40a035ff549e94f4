// Exact per-image order statistics of an fp32 map on the device: the k-th values that numpy.percentile (reference src/scripts/colorize_depth.py:55-56,
// the colorize() repeated in four more scripts) and torch.quantile (reference src/util/depth_transform.py:81-84) take from a sorted copy, selected
// without sorting and without a host read.
//
// A float's order-preserving key (sign bit flipped for positives, every bit for negatives) is resolved 8 bits at a time, most significant digit first.
// Pass p histograms digit p of the elements whose higher digits equal the prefix chosen so far; the prologue of pass p + 1 (every workgroup, redundantly)
// finds in the 256 global bins the bucket that holds the rank, and what is left of the rank inside it.  After four passes the prefix is the key.  Up
// to eight ranks -- the two neighbours of four quantiles -- are followed at once; ranks that still share a prefix share a histogram ("slot").  The
// ranks themselves depend on the population count, which pass 0 produces, so they are computed in the prologue of pass 1.
//
// Histograms: LDS per workgroup, flushed to the per-image global bins, integer atomics throughout -- order-free, so the result is the same bits every
// run.  Before a wave touches LDS it aggregates equal bins with ballots: one add per distinct bin per wave-step.  A depth map is mostly large constant
// regions (a saturated sigmoid, a clipped ReLU); unaggregated, their 64 adds to one LDS word serialise.
//
// Launches: one clear of the workspace (a kernel, not a memset node: every node of a capture is then a kernel of this file), four passes, one finish -- fixed by (batch, n) alone, nothing read back: legal inside a stream capture.
#include "ada_scan.h"

namespace {

constexpr int Q_CHUNK = ADA_QUANTILE_CHUNK;    // elements per workgroup
constexpr int Q_THREADS = 256;
constexpr int Q_PER_THREAD = Q_CHUNK / Q_THREADS;
constexpr int Q_RANKS = 2 * ADA_QUANTILE_MAX_Q;
constexpr int Q_HIST_WORDS = 4 * Q_RANKS * 256;          // [pass][slot][bin]
constexpr int Q_WS_WORDS = ADA_QUANTILE_WS_BYTES_PER_IMAGE / 4;
// the words behind the bins: [0] NaNs in the population, [1] the population count (NaNs included), then per decided pass s the ranks' state at
// 16 + 32 s: prefix[8], rank left inside the prefix[8], slot[8]
constexpr int Q_ST_NAN = 0, Q_ST_COUNT = 1, Q_ST_STAGE = 16, Q_ST_STRIDE = 32;
static_assert(Q_CHUNK % (4 * Q_THREADS) == 0 && Q_RANKS == 8, "layout");
static_assert(Q_WS_WORDS >= Q_HIST_WORDS + Q_ST_STAGE + 3 * Q_ST_STRIDE, "workspace rule");

struct QArgs {
    const float* x;          // [batch, n]
    const uint8_t* valid;    // [batch, n] or NULL
    uint32_t* ws;            // [batch, Q_WS_WORDS]
    int n, flags, mode, nq;
    double exclude;          // compared in double, as ada_depth_colorize_fwd compares invalid_val: one rule for the population and the paint
    double q[ADA_QUANTILE_MAX_Q];
    double* out;             // [batch, nq]
    float* out_f32;          // [batch, nq] or NULL
    int64_t* count;          // [batch] or NULL
};

struct QShared {
    uint32_t prefix[Q_RANKS];       // per rank, after the decided pass
    uint32_t left[Q_RANKS];
    uint32_t slot[Q_RANKS];
    uint32_t slot_prefix[Q_RANKS];  // the distinct prefixes
    uint32_t nslots;
};

// order-preserving key: a < b  <=>  key(a) < key(b) for all non-NaN floats (-0 sorts just below +0; the two are equal values)
ADA_DEV uint32_t key_of(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
ADA_DEV float value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

ADA_DEV bool included(const QArgs& a, bool valid, float v) {
    if (!valid) return false;
    if ((a.flags & ADA_Q_EXCLUDE_VALUE) && !((double)v != a.exclude)) return false;     // NaN != x holds: a NaN is not the excluded value
    if ((a.flags & ADA_Q_POSITIVE_ONLY) && !(v > 0.f)) return false;           // NaN > 0 does not hold
    return true;
}

// The two neighbours of quantile q in a population of cnt (> 0) sorted values.
//   numpy 'linear':   v = (cnt - 1) * q in double, j = floor(v), neighbours j and min(j + 1, cnt - 1)
//   torch.quantile:   r = fp32(q) * fp32(cnt - 1) in fp32, neighbours floor(r) and ceil(r) (clamped: fp32(cnt - 1) may round up past 2^24)
ADA_DEV void rank_pair(int mode, double q, uint32_t cnt, uint32_t& j0, uint32_t& j1) {
#pragma clang fp contract(off)
    const uint32_t last = cnt ? cnt - 1 : 0;
    if (mode == ADA_Q_NUMPY) {
        const double v = (double)last * q;
        uint32_t j = (uint32_t)__builtin_floor(v);
        j = j < last ? j : last;
        j0 = j;
        j1 = j < last ? j + 1 : last;
    } else {
        const float r = (float)q * (float)last;
        const uint32_t lo = (uint32_t)__builtin_floorf(r), hi = (uint32_t)__builtin_ceilf(r);
        j0 = lo < last ? lo : last;
        j1 = hi < last ? hi : last;
    }
}

// Decides pass s (its bins are complete: the kernel before this one wrote them) for every rank: the bucket that holds the rank and the rank's offset
// inside it.  Wave w takes ranks w and w + 4; a lane owns four consecutive bins, the wave scans the 64 sums (ada_scan.h's wave_incl_scan).  Leaves the state in `sh`, the distinct
// prefixes as slots; both barriers are in here.  Pass 0 has no earlier state: its ranks come from the count it produced.
__device__ void decide(const QArgs& a, uint32_t* wsb, int s, QShared& sh, bool publish) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* st = wsb + Q_HIST_WORDS;
    const int nr = 2 * a.nq;
    for (int r = wave; r < nr; r += 4) {
        uint32_t prev = 0, left = 0, slot = 0;
        if (s > 0) {
            const uint32_t* ps = st + Q_ST_STAGE + Q_ST_STRIDE * (s - 1);
            prev = ps[r]; left = ps[8 + r]; slot = ps[16 + r];
            slot = slot < (uint32_t)Q_RANKS ? slot : 0;
        }
        const uint4 h = *reinterpret_cast<const uint4*>(wsb + ((s * Q_RANKS + (int)slot) * 256 + 4 * lane));
        const uint32_t sum = h.x + h.y + h.z + h.w;
        const uint32_t incl = wave_incl_scan(sum);
        if (s == 0) {
            const uint32_t cnt = __shfl(incl, 63) + st[Q_ST_NAN];
            uint32_t j0, j1;
            rank_pair(a.mode, a.q[r >> 1], cnt, j0, j1);
            left = (r & 1) ? j1 : j0;
            if (publish && r == 0 && lane == 0) st[Q_ST_COUNT] = cnt;
        }
        if (lane == 0) {            // an empty population (or a NaN-shortened one) has no bucket for the rank: a defined state, the result is NaN anyway
            sh.prefix[r] = prev << 8;
            sh.left[r] = 0;
        }
        uint32_t c = incl - sum;
        if (left >= c && left < incl) {
            uint32_t bin = 4 * lane;
            if (left >= c + h.x) { c += h.x; ++bin;
                if (left >= c + h.y) { c += h.y; ++bin;
                    if (left >= c + h.z) { c += h.z; ++bin; } } }
            sh.prefix[r] = (prev << 8) | bin;
            sh.left[r] = left - c;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t ns = 0;
        for (int r = 0; r < nr; ++r) {
            uint32_t f = ns;
            for (uint32_t j = 0; j < ns; ++j)
                if (sh.slot_prefix[j] == sh.prefix[r]) f = j;
            if (f == ns) sh.slot_prefix[ns++] = sh.prefix[r];
            sh.slot[r] = f;
        }
        sh.nslots = ns;
    }
    __syncthreads();
    if (publish && (int)threadIdx.x < nr) {
        uint32_t* ps = st + Q_ST_STAGE + Q_ST_STRIDE * s;
        ps[threadIdx.x] = sh.prefix[threadIdx.x];
        ps[8 + threadIdx.x] = sh.left[threadIdx.x];
        ps[16 + threadIdx.x] = sh.slot[threadIdx.x];
    }
}

// One add per distinct bin per wave: the first lane that still holds a bin names it, a ballot finds its equals, it adds their number.  idx < 0: no bin.
ADA_DEV void wave_add(uint32_t* hist, int idx) {
    const int lane = threadIdx.x & 63;
    uint64_t todo = __ballot(idx >= 0);
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const int v = __builtin_amdgcn_readlane(idx, lead);
        const uint64_t same = __ballot(idx == v);
        if (lane == lead) atomicAdd(&hist[v], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// Grid (ceil(n / Q_CHUNK), batch), 256 threads, Q_PER_THREAD elements each.  VEC: n % 4 == 0 and aligned bases, 16-byte loads of four consecutive
// elements; else element e0 + k * 256 + tid, any n, any alignment.  The loads are issued before any bin is touched.
template <bool VEC>
__global__ __launch_bounds__(Q_THREADS) void quantile_pass_kernel(QArgs a, int pass) {
    __shared__ uint32_t hist[Q_RANKS * 256];
    __shared__ QShared sh;
    const int tid = threadIdx.x, b = blockIdx.y;
    uint32_t* wsb = a.ws + (long)b * Q_WS_WORDS;
    for (int i = tid; i < Q_RANKS * 256; i += Q_THREADS) hist[i] = 0;
    uint32_t nslots = 1;
    if (pass > 0) {
        decide(a, wsb, pass - 1, sh, blockIdx.x == 0);
        nslots = sh.nslots;
    } else {
        __syncthreads();
    }
    const long base = (long)b * a.n;
    const uint32_t e0 = blockIdx.x * (uint32_t)Q_CHUNK, n = (uint32_t)a.n;
    float v[Q_PER_THREAD];
    bool ok[Q_PER_THREAD];
    if (VEC) {
#pragma unroll
        for (int k = 0; k < Q_PER_THREAD / 4; ++k) {
            const uint32_t e = e0 + (uint32_t)(k * Q_THREADS + tid) * 4;
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            uint32_t m = 0;
            if (e < n) {        // n % 4 == 0: all four or none
                f = *reinterpret_cast<const float4*>(a.x + base + e);
                m = a.valid ? *reinterpret_cast<const uint32_t*>(a.valid + base + e) : 0x01010101u;
            }
            v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
#pragma unroll
            for (int j = 0; j < 4; ++j) ok[4 * k + j] = ((m >> (8 * j)) & 0xffu) != 0;
        }
    } else {
#pragma unroll
        for (int k = 0; k < Q_PER_THREAD; ++k) {
            const uint32_t e = e0 + (uint32_t)(k * Q_THREADS + tid);
            v[k] = 0.f;
            ok[k] = false;
            if (e < n) {
                v[k] = a.x[base + e];
                ok[k] = a.valid ? a.valid[base + e] != 0 : true;
            }
        }
    }
    const int shift = 24 - 8 * pass;
    uint32_t nans = 0;
#pragma unroll
    for (int k = 0; k < Q_PER_THREAD; ++k) {
        int idx = -1;
        bool nan = false;
        if (included(a, ok[k], v[k])) {
            nan = v[k] != v[k];
            if (!nan) {
                const uint32_t key = key_of(v[k]);
                if (pass == 0) {
                    idx = (int)(key >> 24);
                } else {
                    const uint32_t pre = key >> (shift + 8);
                    for (uint32_t s = 0; s < nslots; ++s)
                        if (sh.slot_prefix[s] == pre) idx = (int)(s * 256 + ((key >> shift) & 255u));
                }
            }
        }
        if (pass == 0) nans += (uint32_t)__popcll(__ballot(nan));
        wave_add(hist, idx);
    }
    if (pass == 0 && nans && (tid & 63) == 0) atomicAdd(wsb + Q_HIST_WORDS + Q_ST_NAN, nans);
    __syncthreads();
    uint32_t* g = wsb + pass * Q_RANKS * 256;
    for (uint32_t s = 0; s < nslots; ++s) {
        const uint32_t c = hist[s * 256 + tid];
        if (c) atomicAdd(g + s * 256 + tid, c);
    }
}

__global__ __launch_bounds__(Q_THREADS) void quantile_clear_kernel(uint4* ws, long n16) {
    const long i = (long)blockIdx.x * Q_THREADS + threadIdx.x;
    if (i < n16) ws[i] = make_uint4(0u, 0u, 0u, 0u);
}

// Grid (batch): decides the last pass -- the prefixes are now the keys -- and interpolates.
//   numpy (_lerp):        a + (b - a) * g, and b - (b - a) * (1 - g) where g >= 0.5, in double, every step rounded
//   torch (ATen's lerp):  lo + w * d where w < 0.5, else hi - d * (1 - w), in fp32 with the product fused into the sum -- what the CPU kernel of
//                         torch.quantile computes where the host has FMA (its lerp is an fmadd; ATen's DEFAULT capability without FMA rounds
//                         twice and is NOT what this reproduces); d = hi - lo and 1 - w are rounded on their own
__global__ __launch_bounds__(Q_THREADS) void quantile_finish_kernel(QArgs a) {
#pragma clang fp contract(off)
    __shared__ QShared sh;
    const int b = blockIdx.x;
    uint32_t* wsb = a.ws + (long)b * Q_WS_WORDS;
    decide(a, wsb, 3, sh, false);
    const uint32_t* st = wsb + Q_HIST_WORDS;
    const uint32_t cnt = st[Q_ST_COUNT];
    const int i = threadIdx.x;
    if (i == 0 && a.count) a.count[b] = (int64_t)cnt;
    if (i >= a.nq) return;
    double res = __builtin_nan("");
    if (cnt != 0 && st[Q_ST_NAN] == 0) {
        const float lo = value_of(sh.prefix[2 * i]), hi = value_of(sh.prefix[2 * i + 1]);
        if (a.mode == ADA_Q_NUMPY) {
            const double v = (double)(cnt - 1) * a.q[i];
            const double g = v - __builtin_floor(v);
            const double d = (double)hi - (double)lo;
            res = g >= 0.5 ? (double)hi - d * (1.0 - g) : (double)lo + d * g;
        } else {
            const float r = (float)a.q[i] * (float)(cnt - 1);
            const float w = r - __builtin_floorf(r);
            const float d = hi - lo;
            const float omw = 1.0f - w;
            res = (double)(w < 0.5f ? __builtin_fmaf(w, d, lo) : __builtin_fmaf(-d, omw, hi));
        }
    }
    a.out[(long)b * a.nq + i] = res;
    if (a.out_f32) a.out_f32[(long)b * a.nq + i] = (float)res;
}

}  // namespace

extern "C" int ada_quantile_fwd(const float* x, const uint8_t* valid, int32_t batch, int64_t n_per_image, const double* q, int32_t nq, int32_t mode,
                                int32_t flags, double exclude_value, double* out, float* out_f32, int64_t* count, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(x && q && out && workspace, ADA_EINVAL, "ada_quantile_fwd: null pointer");
    ADA_REQUIRE(batch > 0 && n_per_image > 0, ADA_EINVAL, "ada_quantile_fwd: bad shape batch=%d n=%ld", batch, (long)n_per_image);
    ADA_REQUIRE(n_per_image < ((int64_t)1 << 31) && batch <= 65535, ADA_EUNSUPPORTED, "ada_quantile_fwd: n=%ld / batch=%d exceed 2^31 - 1 / 65535", (long)n_per_image, batch);
    ADA_REQUIRE(nq >= 1 && nq <= ADA_QUANTILE_MAX_Q, ADA_EINVAL, "ada_quantile_fwd: %d quantiles (1..%d per call)", nq, ADA_QUANTILE_MAX_Q);
    ADA_REQUIRE(mode == ADA_Q_NUMPY || mode == ADA_Q_TORCH, ADA_EINVAL, "ada_quantile_fwd: mode %d (ADA_Q_NUMPY, ADA_Q_TORCH)", mode);
    ADA_REQUIRE((flags & ~(ADA_Q_EXCLUDE_VALUE | ADA_Q_POSITIVE_ONLY)) == 0, ADA_EINVAL, "ada_quantile_fwd: unknown flags 0x%x", flags);
    for (int i = 0; i < nq; ++i)     // host pointer
        ADA_REQUIRE(q[i] >= 0.0 && q[i] <= 1.0, ADA_EINVAL, "ada_quantile_fwd: q[%d] = %g outside [0, 1]", i, q[i]);
    const int64_t need = (int64_t)batch * ADA_QUANTILE_WS_BYTES_PER_IMAGE;
    ADA_REQUIRE(workspace_bytes >= need && (uintptr_t)workspace % 16 == 0, ADA_EINVAL,
                "ada_quantile_fwd: workspace of %ld bytes (16-byte aligned) needed, got %ld", (long)need, (long)workspace_bytes);
    const hipStream_t s = (hipStream_t)stream;
    QArgs a;
    a.x = x; a.valid = valid; a.ws = (uint32_t*)workspace;
    a.n = (int)n_per_image; a.flags = flags; a.mode = mode; a.nq = nq; a.exclude = exclude_value;
    for (int i = 0; i < ADA_QUANTILE_MAX_Q; ++i) a.q[i] = i < nq ? q[i] : 0.0;
    a.out = out; a.out_f32 = out_f32; a.count = count;
    const long n16 = (long)(need / 16);
    hipLaunchKernelGGL(quantile_clear_kernel, dim3((unsigned)((n16 + Q_THREADS - 1) / Q_THREADS)), dim3(Q_THREADS), 0, s, (uint4*)workspace, n16);
    const dim3 grid((unsigned)((n_per_image + Q_CHUNK - 1) / Q_CHUNK), (unsigned)batch);
    const bool vec = n_per_image % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)valid % 4 == 0;
    for (int pass = 0; pass < 4; ++pass) {
        if (vec) hipLaunchKernelGGL(quantile_pass_kernel<true>, grid, dim3(Q_THREADS), 0, s, a, pass);
        else hipLaunchKernelGGL(quantile_pass_kernel<false>, grid, dim3(Q_THREADS), 0, s, a, pass);
    }
    hipLaunchKernelGGL(quantile_finish_kernel, dim3((unsigned)batch), dim3(Q_THREADS), 0, s, a);
    return ada_check_launch("ada_quantile_fwd");
}
