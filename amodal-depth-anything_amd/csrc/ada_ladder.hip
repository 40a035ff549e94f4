// The precision ladder's decision and paste on the device (hip_ext/engine.py; no reference counterpart).
//   ada_ladder_select_fwd   reads the per-image statistics the ladder's three reductions left on the device (ada_depth_stats_fwd, ada_token_diversity_fwd
//                           twice), takes hip_ext.ladder.ladder_decide's decision for a first-rung run (ran = 1: no guard band) per image, and copies the
//                           rows of every image that leaves the first rung from the output of its rung into the first rung's output.
// Two kernels, no atomics, one fixed order: `ladder_decide_kernel` is ONE workgroup (an image per thread: the chunk pairs added in index order in fp64,
// the clamp written as a comparison so that a NaN passes through it as it passes through torch's clamp_min, the correctly rounded fp64 division --
// this file is built without any fast-math flag), whose thread 0 then adds the call's tallies to the caller's running counts; `ladder_select_kernel`
// is a memory-bound copy, 16 bytes per lane, in which a workgroup of a first-rung image leaves after reading its image's rung.  The launch sequence
// depends on no device value: it can be captured into a HIP graph.
#include "ada_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int UNROLL = 4;          // independent 16-byte loads in flight per lane
constexpr int MAX_BLOCKS_X = 256;  // per image; the rest of a large image is walked grid-stride

struct LadderArgs {
    const float* stat_sums;   // [B, chunks, 2]
    const float* stat_div;    // [B, groups, 2] or NULL
    const float* stat_in;     // [B, groups_in, 2] or NULL
    int chunks, groups, groups_in, batch;
    double thr, thr3, div, div_in;
    int has2, has3, has_r;
    uint32_t* out;            // [B, n]
    const uint32_t* src2;
    const uint32_t* src3;
    int64_t n;
    int32_t* rung;
    double* ratio;
    int64_t* counts;
};

// torch's clamp_min(1e-300): NaN stays NaN (fmax would return the bound)
ADA_DEV double clamp_min_tiny(double x) { return x < 1e-300 ? 1e-300 : x; }

// (sum of p[2 c], sum of p[2 c + 1]) over c = 0 .. n - 1 in index order, fp64, starting from +0 as the host's reduction does
ADA_DEV void pair_sums(const float* __restrict__ p, int n, double& s0, double& s1) {
    s0 = 0.0;
    s1 = 0.0;
    for (int c = 0; c < n; ++c) {
        s0 += (double)p[2 * c];
        s1 += (double)p[2 * c + 1];
    }
}

// one workgroup; thread t decides images t, t + THREADS, ...
__global__ __launch_bounds__(THREADS) void ladder_decide_kernel(LadderArgs a) {
    for (int b = threadIdx.x; b < a.batch; b += THREADS) {
        double s0, s1, r = 0.0;
        if (a.has_r) {
            pair_sums(a.stat_sums + (int64_t)b * a.chunks * 2, a.chunks, s0, s1);
            r = s1 / clamp_min_tiny(s0);
        }
        bool flat = false;
        if (a.stat_div) {      // (sum of variances, sum of mean squares)
            pair_sums(a.stat_div + (int64_t)b * a.groups * 2, a.groups, s0, s1);
            flat = s0 / clamp_min_tiny(s1) < a.div;
        }
        if (a.stat_in) {
            pair_sums(a.stat_in + (int64_t)b * a.groups_in * 2, a.groups_in, s0, s1);
            flat = flat || (s0 / clamp_min_tiny(s1) < a.div_in);
        }
        const bool to3 = a.has3 && (flat || r > a.thr3);
        const bool to2 = a.has2 && (flat || r > a.thr);
        a.rung[b] = to3 ? 3 : to2 ? 2 : 1;
        a.ratio[b] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {      // the call's tallies, images in index order
        int64_t n2 = 0, n3 = 0, unserved = 0;
        for (int b = 0; b < a.batch; ++b) {
            const int k = a.rung[b];
            n2 += k >= 2;
            n3 += k == 3;
            unserved += (k == 3 && !a.src3) || (k == 2 && !a.src2);
        }
        a.counts[0] += 1;
        a.counts[1] += n2;
        a.counts[2] += n3;
        a.counts[3] += unserved;
    }
}

// grid (blocks, batch): image blockIdx.y's row from the output of its rung.  Words are moved as bits (a NaN keeps its payload).
__global__ __launch_bounds__(THREADS) void ladder_select_kernel(LadderArgs a) {
    const int b = blockIdx.y;
    const int k = a.rung[b];
    const uint32_t* from = k == 3 ? (a.src3 ? a.src3 : a.src2) : k == 2 ? a.src2 : nullptr;
    if (!from) return;
    const int64_t n = a.n;
    uint32_t* __restrict__ dst = a.out + (int64_t)b * n;
    const uint32_t* __restrict__ src = from + (int64_t)b * n;
    // words in front of the row's first 16-byte boundary (n need not be a multiple of 4: rows start anywhere); a source row that is not
    // congruent to the destination's goes word by word
    int64_t head = (4 - (int64_t)(((uintptr_t)dst >> 2) & 3)) & 3;
    if ((((uintptr_t)dst ^ (uintptr_t)src) & 15) != 0 || head > n) head = n;
    const int64_t nvec = (n - head) >> 2;
    const int64_t body_end = head + 4 * nvec;
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x, T = (int64_t)gridDim.x * THREADS;
    for (int64_t i = t; i < head; i += T) dst[i] = src[i];
    for (int64_t i = body_end + t; i < n; i += T) dst[i] = src[i];
    const u32x4* __restrict__ sv = (const u32x4*)(src + head);
    u32x4* __restrict__ dv = (u32x4*)(dst + head);
    int64_t i = t;
    for (; i + (UNROLL - 1) * T < nvec; i += UNROLL * T) {
        u32x4 v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) v[u] = sv[i + u * T];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) dv[i + u * T] = v[u];
    }
    for (; i < nvec; i += T) dv[i] = sv[i];
}

bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int ada_ladder_select_fwd(const float* stat_sums, int32_t chunks, const float* stat_div, int32_t groups, const float* stat_in, int32_t groups_in,
                                     int32_t batch, double thr, double thr3, double div, double div_in, int32_t has2, int32_t has3, int32_t has_r,
                                     float* out, const float* src2, const float* src3, int64_t n_per_image, int32_t* rung, double* ratio,
                                     int64_t* counts, void* stream) {
    ADA_REQUIRE(out && rung && ratio && counts, ADA_EINVAL, "ada_ladder_select_fwd: null pointer");
    ADA_REQUIRE(batch > 0 && batch <= 65535 && n_per_image > 0, ADA_EINVAL, "ada_ladder_select_fwd: bad shape batch=%d n_per_image=%ld", batch, (long)n_per_image);
    ADA_REQUIRE(!has_r || (stat_sums && chunks > 0), ADA_EINVAL, "ada_ladder_select_fwd: has_r without stat_sums (chunks=%d)", chunks);
    ADA_REQUIRE((!stat_div || groups > 0) && (!stat_in || groups_in > 0), ADA_EINVAL, "ada_ladder_select_fwd: a statistics block with no columns (groups=%d groups_in=%d)",
                groups, groups_in);
    ADA_REQUIRE(src2 != out && src3 != out, ADA_EINVAL, "ada_ladder_select_fwd: a source aliases out");
    ADA_REQUIRE(aligned_to(out, 4) && aligned_to(src2, 4) && aligned_to(src3, 4) && aligned_to(ratio, 8) && aligned_to(counts, 8) && aligned_to(rung, 4), ADA_EINVAL,
                "ada_ladder_select_fwd: misaligned pointer");
    LadderArgs a;
    a.stat_sums = stat_sums; a.stat_div = stat_div; a.stat_in = stat_in;
    a.chunks = chunks; a.groups = groups; a.groups_in = groups_in; a.batch = batch;
    a.thr = thr; a.thr3 = thr3; a.div = div; a.div_in = div_in;
    a.has2 = has2 != 0; a.has3 = has3 != 0; a.has_r = has_r != 0;
    a.out = (uint32_t*)out; a.src2 = (const uint32_t*)src2; a.src3 = (const uint32_t*)src3; a.n = n_per_image;
    a.rung = rung; a.ratio = ratio; a.counts = counts;
    hipLaunchKernelGGL(ladder_decide_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, a);
    if (src2 || src3) {      // known on the host: with neither source every row stays (the decision and the tallies are still taken)
        const int64_t per_block = (int64_t)THREADS * 4 * UNROLL;
        int64_t gx = (n_per_image + per_block - 1) / per_block;
        if (gx > MAX_BLOCKS_X) gx = MAX_BLOCKS_X;
        hipLaunchKernelGGL(ladder_select_kernel, dim3((unsigned)gx, (unsigned)batch), dim3(THREADS), 0, (hipStream_t)stream, a);
    }
    return ada_check_launch("ada_ladder_select_fwd");
}
