// The paper's evaluation protocol on the device (reference: src/trainer/discriminative_trainer.py:496-613, src/scripts/pix2gestalt_eval.py:200-297).
//   ada_protocol_fit_fwd   one pass over (prediction, observation, visible, whole): the five sums of the least-squares fit of the prediction onto
//                          the OBSERVATION over the VISIBLE mask, min / max of the prediction there, the two pixel counts of the difficulty bucket,
//                          and the fit itself, solved in fp64 on the device.
//   ada_protocol_eval_fwd  one pass over (prediction, gt, region, valid, fit rows): the ADA_EVAL_* sums of the raw and of the aligned prediction
//                          over region && valid, with + eps on both sides and no clamp.
// The prediction may be smaller or larger than the evaluation grid: it is gathered by ATen's legacy nearest rule inside both passes.
// Both kernels are memory-bound reductions and neither uses an atomic: an image is cut into chunks of ADA_PROTOCOL_CHUNK pixels -- a function of
// h * w alone, not of the batch -- one workgroup reduces one chunk in a fixed order (per-thread partials over a fixed pixel assignment, wave
// butterfly, the four waves through LDS), the chunk partials go to the caller's workspace, and a second small kernel adds them in index order.  So
// the result of an image is the same bits from run to run, alone or inside any batch, on the vector and on the scalar load path.
#include "ada_common.h"

// every product and sum below is rounded on its own: the aligned value is torch's `pred * scale + shift` (no FMA), as in ada_blend_ex
#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int VEC = 4;
constexpr int CHUNK = ADA_PROTOCOL_CHUNK;
constexpr int ITERS = CHUNK / (THREADS * VEC);
static_assert(ITERS * THREADS * VEC == CHUNK, "a chunk is a whole number of 4-pixel groups per thread");
constexpr int NSUM = ADA_EVAL_NSUM;
constexpr int FIT_NPART = 8;     // n, sum p, sum o, sum pp, sum po, min p, max p, #whole
static_assert(FIT_NPART <= ADA_PROTOCOL_WS_DOUBLES && 2 * NSUM <= ADA_PROTOCOL_WS_DOUBLES, "workspace row");

// ATen's legacy nearest rule (UpSample.h nearest_idx with the scale computed from the sizes), per axis
struct Gather {
    int h, w, hp, wp;
    float sy, sx;
    int identity;
};
ADA_DEV int src_index(int dst, float scale, int in) {
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}
ADA_DEV float gather_pred(const float* __restrict__ pred, const Gather& g, int i) {
    if (g.identity) return pred[i];
    const int y = i / g.w, x = i - y * g.w;
    return pred[(long)src_index(y, g.sy, g.hp) * g.wp + src_index(x, g.sx, g.wp)];
}

// four consecutive pixels from i0 (i0 % 4 == 0): one 16-byte / 4-byte load when VECL (n % 4 == 0 and aligned bases), else guarded scalars
template <bool VECL>
ADA_DEV void load4f(const float* __restrict__ p, int i0, int n, float v[4]) {
    if (VECL) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + i0);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = i0 + j < n ? p[i0 + j] : 0.0f;
    }
}
template <bool VECL>
ADA_DEV uint32_t load4b(const unsigned char* __restrict__ p, int i0, int n) {
    if (VECL) return *reinterpret_cast<const uint32_t*>(p + i0);
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        if (i0 + j < n) r |= (uint32_t)p[i0 + j] << (8 * j);
    return r;
}
template <bool VECL>
ADA_DEV void load4pred(const float* __restrict__ pred, const Gather& g, int i0, int n, uint32_t need, float v[4]) {
    if (g.identity) {
        load4f<VECL>(pred, i0, n, v);
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = ((need >> (8 * j)) & 0xff) ? gather_pred(pred, g, i0 + j) : 0.0f;
    }
}

ADA_DEV double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
ADA_DEV float wave_min(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = __builtin_fminf(v, __shfl_xor(v, o));
    return v;
}
ADA_DEV float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// fit
// ------------------------------------------------------------------------------------------------------------------------------------
struct FitArgs {
    const float* pred;
    const float* obs;
    const unsigned char* visible;
    const unsigned char* whole;
    Gather g;
    int n, chunks;
    double* part;     // [B][chunks][FIT_NPART]
    double* fit;      // [B][ADA_FIT_NCOL]
};

// grid (chunks, batch), 256 threads
template <bool VECL>
__global__ __launch_bounds__(THREADS) void protocol_fit_partial_kernel(FitArgs a) {
    __shared__ double part[THREADS / 64][FIT_NPART];
    const int b = blockIdx.y, c = blockIdx.x;
    const float* pred = a.pred + (long)b * a.g.hp * a.g.wp;
    const float* obs = a.obs + (long)b * a.n;
    const unsigned char* vis = a.visible + (long)b * a.n;
    const unsigned char* whole = a.whole + (long)b * a.n;
    double cnt = 0.0, sp = 0.0, so = 0.0, spp = 0.0, spo = 0.0, nw = 0.0;
    float lo = __builtin_inff(), hi = -__builtin_inff();
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int i0 = c * CHUNK + (it * THREADS + (int)threadIdx.x) * VEC;
        if (i0 >= a.n) continue;
        const uint32_t v4 = load4b<VECL>(vis, i0, a.n), w4 = load4b<VECL>(whole, i0, a.n);
#pragma unroll
        for (int j = 0; j < VEC; ++j) nw += ((w4 >> (8 * j)) & 0xff) ? 1.0 : 0.0;
        if (!v4) continue;
        float p4[4], o4[4];
        load4pred<VECL>(pred, a.g, i0, a.n, v4, p4);
        load4f<VECL>(obs, i0, a.n, o4);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (!((v4 >> (8 * j)) & 0xff)) continue;
            const double p = (double)p4[j], o = (double)o4[j];
            cnt += 1.0;
            sp += p;
            so += o;
            spp += p * p;
            spo += p * o;
            lo = __builtin_fminf(lo, p4[j]);
            hi = __builtin_fmaxf(hi, p4[j]);
        }
    }
    cnt = wave_sum(cnt); sp = wave_sum(sp); so = wave_sum(so); spp = wave_sum(spp); spo = wave_sum(spo); nw = wave_sum(nw);
    lo = wave_min(lo); hi = wave_max(hi);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wv][0] = cnt; part[wv][1] = sp; part[wv][2] = so; part[wv][3] = spp; part[wv][4] = spo;
        part[wv][5] = (double)lo; part[wv][6] = (double)hi; part[wv][7] = nw;
    }
    __syncthreads();
    if (threadIdx.x < FIT_NPART) {
        const int k = threadIdx.x;
        double t = part[0][k];
#pragma unroll
        for (int i = 1; i < THREADS / 64; ++i) t = k == 5 ? __builtin_fmin(t, part[i][k]) : k == 6 ? __builtin_fmax(t, part[i][k]) : t + part[i][k];
        a.part[((long)b * a.chunks + c) * FIT_NPART + k] = t;
    }
}

// grid (batch), 64 threads: chunk partials in index order, then the 2x2 solve
__global__ __launch_bounds__(64) void protocol_fit_final_kernel(FitArgs a) {
    __shared__ double s[FIT_NPART];
    const int b = blockIdx.x, k = threadIdx.x;
    if (k < FIT_NPART) {
        const double* p = a.part + (long)b * a.chunks * FIT_NPART + k;
        double t = p[0];
        for (int c = 1; c < a.chunks; ++c) {
            const double v = p[(long)c * FIT_NPART];
            t = k == 5 ? __builtin_fmin(t, v) : k == 6 ? __builtin_fmax(t, v) : t + v;
        }
        s[k] = t;
    }
    __syncthreads();
    if (k == 0) {
        const double n = s[0], sp = s[1], so = s[2], spp = s[3], spo = s[4], lo = s[5], hi = s[6];
        double scale, shift;
        if (n == 0.0) {                      // no support: lstsq's minimum-norm answer of the empty system
            scale = 0.0; shift = 0.0;
        } else if (lo == hi) {               // rank one (every visible prediction equals c): minimum norm along (c, 1)
            const double c = lo, obar = so / n, q = c * c + 1.0;
            scale = c * obar / q; shift = obar / q;
        } else {                             // normal equations (src/util/alignment.py scale_shift_least_square)
            const double den = n * spp - sp * sp;
            scale = (n * spo - sp * so) / den;
            shift = (so - scale * sp) / n;
        }
        double* row = a.fit + (long)b * ADA_FIT_NCOL;
        row[ADA_FIT_N] = n; row[ADA_FIT_SUM_P] = sp; row[ADA_FIT_SUM_O] = so; row[ADA_FIT_SUM_PP] = spp; row[ADA_FIT_SUM_PO] = spo;
        row[ADA_FIT_MIN_P] = lo; row[ADA_FIT_MAX_P] = hi; row[ADA_FIT_N_VISIBLE] = n; row[ADA_FIT_N_WHOLE] = s[7];
        row[ADA_FIT_SCALE] = scale; row[ADA_FIT_SHIFT] = shift; row[ADA_FIT_NCOL - 1] = 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// eval
// ------------------------------------------------------------------------------------------------------------------------------------
struct ProtoEvalArgs {
    const float* pred;
    const float* gt;
    const unsigned char* region;
    const unsigned char* valid;   // may be null: every pixel valid
    const double* fit;            // [B][ADA_FIT_NCOL]
    Gather g;
    float eps;
    int n, chunks;
    double* part;     // [B][chunks][2][NSUM]
    double* out;      // [B][2][NSUM]
};

// the per-pixel terms of ada_depth_eval_fwd (ada_eval.hip), unclamped: a non-positive p makes the log terms NaN and nothing else
ADA_DEV void accumulate(double s[NSUM - 1], float p, float g, float lg) {
    constexpr float T1 = 1.25f, T2 = 1.25f * 1.25f, T3 = 1.25f * 1.25f * 1.25f;
    const float d = p - g;
    const float dl = __logf(p) - lg;
    const float ratio = __builtin_fmaxf(p / g, g / p);
    const float di = 1.0f / p - 1.0f / g;
    s[ADA_EVAL_N] += 1.0;
    s[ADA_EVAL_SUM_P] += (double)p;
    s[ADA_EVAL_SUM_G] += (double)g;
    s[ADA_EVAL_SUM_PP] += (double)p * (double)p;
    s[ADA_EVAL_SUM_PG] += (double)p * (double)g;
    s[ADA_EVAL_ABS_REL] += (double)(__builtin_fabsf(d) / g);
    s[ADA_EVAL_SQ_REL] += (double)(d * d / g);
    s[ADA_EVAL_SQ] += (double)(d * d);
    s[ADA_EVAL_LOG_SQ] += (double)(dl * dl);
    s[ADA_EVAL_LOG] += (double)dl;
    s[ADA_EVAL_LOG10_ABS] += (double)(__builtin_fabsf(dl) * 0.43429448190325176f);
    s[ADA_EVAL_D1] += ratio < T1 ? 1.0 : 0.0;
    s[ADA_EVAL_D2] += ratio < T2 ? 1.0 : 0.0;
    s[ADA_EVAL_D3] += ratio < T3 ? 1.0 : 0.0;
    s[ADA_EVAL_INV_SQ] += (double)(di * di);
}

// grid (chunks, batch), 256 threads
template <bool VECL>
__global__ __launch_bounds__(THREADS) void protocol_eval_partial_kernel(ProtoEvalArgs a) {
    __shared__ double part[THREADS / 64][2 * NSUM];
    const int b = blockIdx.y, c = blockIdx.x;
    const float* pred = a.pred + (long)b * a.g.hp * a.g.wp;
    const float* gt = a.gt + (long)b * a.n;
    const unsigned char* region = a.region + (long)b * a.n;
    const unsigned char* valid = a.valid ? a.valid + (long)b * a.n : nullptr;
    const float sc = (float)a.fit[(long)b * ADA_FIT_NCOL + ADA_FIT_SCALE], sh = (float)a.fit[(long)b * ADA_FIT_NCOL + ADA_FIT_SHIFT];
    double raw[NSUM - 1], al[NSUM - 1];
#pragma unroll
    for (int i = 0; i < NSUM - 1; ++i) raw[i] = al[i] = 0.0;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int i0 = c * CHUNK + (it * THREADS + (int)threadIdx.x) * VEC;
        if (i0 >= a.n) continue;
        uint32_t m4 = load4b<VECL>(region, i0, a.n);
        if (!m4) continue;
        if (valid) {                      // byte-wise region != 0 && valid != 0
            const uint32_t v4 = load4b<VECL>(valid, i0, a.n);
            uint32_t both = 0;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (((m4 >> (8 * j)) & 0xff) && ((v4 >> (8 * j)) & 0xff)) both |= 1u << (8 * j);
            m4 = both;
            if (!m4) continue;
        }
        float p4[4], g4[4];
        load4pred<VECL>(pred, a.g, i0, a.n, m4, p4);
        load4f<VECL>(gt, i0, a.n, g4);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (!((m4 >> (8 * j)) & 0xff)) continue;
            const float g = g4[j] + a.eps;
            const float lg = __logf(g);
            accumulate(raw, p4[j] + a.eps, g, lg);
            accumulate(al, p4[j] * sc + sh + a.eps, g, lg);
        }
    }
    // a wave without a single counted pixel holds exact zeros: its butterfly would add zeros to zeros
    const bool any = __ballot(raw[ADA_EVAL_N] != 0.0) != 0;
    if (any) {
#pragma unroll
        for (int i = 0; i < NSUM - 1; ++i) { raw[i] = wave_sum(raw[i]); al[i] = wave_sum(al[i]); }
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NSUM - 1; ++i) { part[wv][i] = raw[i]; part[wv][NSUM + i] = al[i]; }
        part[wv][NSUM - 1] = 0.0; part[wv][2 * NSUM - 1] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < 2 * NSUM) {
        const int k = threadIdx.x;
        double t = part[0][k];
#pragma unroll
        for (int i = 1; i < THREADS / 64; ++i) t += part[i][k];
        a.part[((long)b * a.chunks + c) * (2 * NSUM) + k] = t;
    }
}

// grid (batch), 64 threads: chunk partials in index order
__global__ __launch_bounds__(64) void protocol_eval_final_kernel(ProtoEvalArgs a) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= 2 * NSUM) return;
    const double* p = a.part + (long)b * a.chunks * (2 * NSUM) + k;
    double t = p[0];
    for (int c = 1; c < a.chunks; ++c) t += p[(long)c * (2 * NSUM)];
    a.out[(long)b * (2 * NSUM) + k] = t;
}

bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int make_gather(const char* who, int32_t hp, int32_t wp, int32_t batch, int32_t h, int32_t w, Gather* g, int* n, int* chunks) {
    ADA_REQUIRE(batch > 0 && batch <= 65535 && h > 0 && w > 0 && hp > 0 && wp > 0, ADA_EINVAL, "%s: bad shape batch=%d h=%d w=%d hp=%d wp=%d", who, batch, h, w, hp, wp);
    ADA_REQUIRE((int64_t)h * w < (int64_t)1 << 30 && (int64_t)hp * wp < (int64_t)1 << 30, ADA_EUNSUPPORTED, "%s: more than 2^30 pixels per image", who);
    g->h = h; g->w = w; g->hp = hp; g->wp = wp;
    g->sy = (float)hp / (float)h;
    g->sx = (float)wp / (float)w;
    g->identity = hp == h && wp == w;
    *n = h * w;
    *chunks = (*n + CHUNK - 1) / CHUNK;
    return ADA_OK;
}

}  // namespace

extern "C" int ada_protocol_fit_fwd(const float* pred, int32_t hp, int32_t wp, const float* observation, const uint8_t* visible, const uint8_t* whole,
                                    int32_t batch, int32_t h, int32_t w, double* fit, void* workspace, int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(pred && observation && visible && whole && fit && workspace, ADA_EINVAL, "ada_protocol_fit_fwd: null pointer");
    FitArgs a;
    if (int rc = make_gather("ada_protocol_fit_fwd", hp, wp, batch, h, w, &a.g, &a.n, &a.chunks)) return rc;
    const int64_t need = (int64_t)batch * a.chunks * ADA_PROTOCOL_WS_DOUBLES * 8;
    ADA_REQUIRE(workspace_bytes >= need && aligned_to(workspace, 8), ADA_EINVAL, "ada_protocol_fit_fwd: workspace of %ld bytes, %ld needed (8-byte aligned)",
                (long)workspace_bytes, (long)need);
    a.pred = pred; a.obs = observation; a.visible = visible; a.whole = whole; a.part = (double*)workspace; a.fit = fit;
    const bool vec = a.n % VEC == 0 && aligned_to(observation, 16) && aligned_to(visible, 4) && aligned_to(whole, 4) && (!a.g.identity || aligned_to(pred, 16));
    const dim3 grid((unsigned)a.chunks, (unsigned)batch);
    if (vec) hipLaunchKernelGGL(protocol_fit_partial_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(protocol_fit_partial_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(protocol_fit_final_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, a);
    return ada_check_launch("ada_protocol_fit_fwd");
}

extern "C" int ada_protocol_eval_fwd(const float* pred, int32_t hp, int32_t wp, const float* gt, const uint8_t* region, const uint8_t* valid,
                                     const double* fit, float eps, int32_t batch, int32_t h, int32_t w, double* sums, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(pred && gt && region && fit && sums && workspace, ADA_EINVAL, "ada_protocol_eval_fwd: null pointer");
    ProtoEvalArgs a;
    if (int rc = make_gather("ada_protocol_eval_fwd", hp, wp, batch, h, w, &a.g, &a.n, &a.chunks)) return rc;
    const int64_t need = (int64_t)batch * a.chunks * ADA_PROTOCOL_WS_DOUBLES * 8;
    ADA_REQUIRE(workspace_bytes >= need && aligned_to(workspace, 8), ADA_EINVAL, "ada_protocol_eval_fwd: workspace of %ld bytes, %ld needed (8-byte aligned)",
                (long)workspace_bytes, (long)need);
    a.pred = pred; a.gt = gt; a.region = region; a.valid = valid; a.fit = fit; a.eps = eps; a.part = (double*)workspace; a.out = sums;
    const bool vec = a.n % VEC == 0 && aligned_to(gt, 16) && aligned_to(region, 4) && (!valid || aligned_to(valid, 4)) && (!a.g.identity || aligned_to(pred, 16));
    const dim3 grid((unsigned)a.chunks, (unsigned)batch);
    if (vec) hipLaunchKernelGGL(protocol_eval_partial_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(protocol_eval_partial_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(protocol_eval_final_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, a);
    return ada_check_launch("ada_protocol_eval_fwd");
}
