// Membrane solve on the device: the discrete harmonic extension of the known pixels of a map over a masked 4-neighbour grid, by conjugate gradients in
// fp64 (include/ada_hip.h, "Membrane solve"; DESIGN.md, "Membrane solve"; restated in numpy by tests/_membrane_ref.py).  One solver, three uses: the
// exact counterpart of the push-pull fill, seamless cloning (the correction u of dst - src is extended and src is added back) and a seam-free amodal blend.
//
// STATE.  Everything between two calls lives in the workspace: per plane the fp64 vectors u (the known pixels' data included), r, q and a double-buffered
// direction p, per image one code byte per pixel (unknown / known / which of the four edges exist), per plane and workgroup three partial sums, and per
// plane two slots of scalars (r.r, tol, frozen, steps).  begin writes every cell that a later kernel reads; nothing depends on what the workspace held.
//
// ONE STEP = TWO LAUNCHES, every one a plain fixed grid of (tiles, channels, batch) workgroups of 256 threads, a workgroup per ADA_MEMBRANE_TILE_H x
// ADA_MEMBRANE_TILE_W tile of one plane:
//   direction   reduces the tiles' partial r.r and max |r| (every workgroup for itself, in one fixed order), freezes the plane at max |r| <= tol, forms
//               p' = r + beta p for its tile and a one-pixel halo in LDS, writes its tile of p' to the OTHER direction buffer (a neighbour may still be
//               reading the old one), q = A p' and the tile's partial p'.q;
//   update      reduces the partial p'.q the same way, freezes the plane unless p'.q > 0 and alpha is finite, u += alpha p', r -= alpha q and the tile's
//               partial r.r and max |r|.
// A kernel reads scalars only from the slot the launch before it wrote, and writes only the other slot, so no workgroup waits for another one.  A frozen
// plane's workgroups return at once: its state stays as it is, whatever the number of steps still issued.  The direction buffer in use is picked by the
// plane's own step count, so begin -> iterate(a) -> iterate(b) is iterate(a + b).
//
// No float atomics, no grid-wide barrier, no cooperative launch.  Every sum has one order: a thread adds its four pixels top down, the workgroup's 256
// values meet in a binary tree in LDS, the tiles' partials are added by thread t for the tiles t, t + 256, ... and meet in the same tree.  The order depends
// on (h, w) alone, so a plane's bytes are the same from run to run and in any batch.  The products that two workgroups both form (p' in a tile and in its
// neighbours' halos) are written as explicit fma, so contraction cannot make them differ.  No scratch (NO_SCRATCH).
#include "ada_common.h"

namespace {

constexpr int TH = ADA_MEMBRANE_TILE_H, TW = ADA_MEMBRANE_TILE_W;
constexpr int PX = TH * TW / 256;      // pixels of a column per thread: rows ty, ty + 4, ...
static_assert(TW == 64 && TH % 4 == 0 && PX * 256 == TH * TW, "a workgroup is 4 rows of 64 threads");

constexpr int C_UNKNOWN = 1, C_KNOWN = 2, C_UP = 4, C_DOWN = 8, C_LEFT = 16, C_RIGHT = 32, C_EDGES = C_UP | C_DOWN | C_LEFT | C_RIGHT;

struct Scalars {      // one slot: written by workgroup 0 of a plane, read by every workgroup of the plane's next launch
    double rr;        // r.r of the residual the current direction was formed from
    double tol;
    int frozen;
    int steps;
};

struct Layout {      // the workspace, 8-byte aligned pieces first
    double *u, *r, *q, *p0, *p1, *part;
    Scalars* scal;
    uint8_t* code;
    int64_t bytes;
};

int64_t n_tiles(int32_t h, int32_t w) { return (int64_t)((h + TH - 1) / TH) * ((w + TW - 1) / TW); }

Layout layout(void* ws, int64_t batch, int64_t channels, int32_t h, int32_t w) {
    const int64_t hw = (int64_t)h * w, planes = batch * channels, vec = planes * hw;
    const int64_t part = 8 * 5 * vec;                                      // after the five vectors: [plane][3][tiles] of r.r, max |r|, p.q
    const int64_t scal = part + 8 * planes * 3 * n_tiles(h, w);            // [plane][2]
    const int64_t code = scal + (int64_t)sizeof(Scalars) * planes * 2;     // [batch][h w]
    Layout L{};
    L.bytes = (code + batch * hw + 7) / 8 * 8;
    if (!ws) return L;      // the size alone
    uint8_t* base = (uint8_t*)ws;
    L.u = (double*)base;
    L.r = L.u + vec;
    L.q = L.r + vec;
    L.p0 = L.q + vec;
    L.p1 = L.p0 + vec;
    L.part = (double*)(base + part);
    L.scal = (Scalars*)(base + scal);
    L.code = base + code;
    return L;
}

// NaN wins: a residual that is not a number must never look small
ADA_DEV double nan_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// the workgroup's 256 values in one binary tree; every thread returns the total.  ``s`` is free for the next use on return.
ADA_DEV double block_sum(double v, double* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) s[t] = s[t] + s[t + k];
        __syncthreads();
    }
    const double total = s[0];
    __syncthreads();
    return total;
}

ADA_DEV double block_max(double v, double* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) s[t] = nan_max(s[t], s[t + k]);
        __syncthreads();
    }
    const double total = s[0];
    __syncthreads();
    return total;
}

// the tiles' partials of one plane, thread t taking the tiles t, t + 256, ...
ADA_DEV double tiles_sum(const double* part, int tiles, double* s) {
    double v = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 256) v = v + part[i];
    return block_sum(v, s);
}

ADA_DEV double tiles_max(const double* part, int tiles, double* s) {
    double v = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 256) v = nan_max(v, part[i]);
    return block_max(v, s);
}

ADA_DEV long plane_of() { return (long)blockIdx.z * gridDim.y + blockIdx.y; }

// sum over the existing edges of (v_q - v_p), in the order up, down, left, right: b - A u at an unknown pixel when v holds the data on the known pixels
ADA_DEV double edge_residual(const double* v, long o, int w, int code) {
    const double c = v[o];
    double s = 0.0;
    if (code & C_UP) s = s + (v[o - w] - c);
    if (code & C_DOWN) s = s + (v[o + w] - c);
    if (code & C_LEFT) s = s + (v[o - 1] - c);
    if (code & C_RIGHT) s = s + (v[o + 1] - c);
    return s;
}

// ---- begin -----------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(h w / 256), channels, batch): the code byte of every pixel (written by channel 0) and the start vector: the data on a known pixel, the
// guess on an unknown one.  Selects only: what lies under a pixel that is not known is never loaded into an arithmetic operation.
__global__ __launch_bounds__(256) void mb_setup_kernel(const float* x, const float* minus, const uint8_t* known, const uint8_t* domain, const float* guess, int h,
                                                       int w, uint8_t* code, double* u) {
    const long hw = (long)h * w;
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= hw) return;
    const long img = (long)blockIdx.z * hw;
    const uint8_t* d = domain ? domain + img : nullptr;
    const int y = (int)(o / w), xx = (int)(o - (long)y * w);
    const bool in = !d || d[o] != 0;
    int c = 0;
    if (in) {
        c = known[img + o] != 0 ? C_KNOWN : C_UNKNOWN;
        if (y > 0 && (!d || d[o - w] != 0)) c |= C_UP;
        if (y + 1 < h && (!d || d[o + w] != 0)) c |= C_DOWN;
        if (xx > 0 && (!d || d[o - 1] != 0)) c |= C_LEFT;
        if (xx + 1 < w && (!d || d[o + 1] != 0)) c |= C_RIGHT;
    }
    if (blockIdx.y == 0) code[img + o] = (uint8_t)c;
    const long po = plane_of() * hw + o;
    double v = 0.0;
    if (c & C_KNOWN) v = minus ? (double)x[po] - (double)minus[po] : (double)x[po];
    else if ((c & C_UNKNOWN) && guess) v = (double)guess[po];
    u[po] = v;      // outside the domain: a zero nobody reads
}

// grid (tiles, channels, batch): r = b - A u, the tile's partial r.r and max |r|, and the plane's first slot of scalars
__global__ __launch_bounds__(256) void mb_residual0_kernel(const uint8_t* code, const double* u, int h, int w, int tiles_x, double tol, double* r, double* part,
                                                           Scalars* scal) {
    __shared__ double s[256];
    const long hw = (long)h * w, plane = plane_of();
    const int tiles = gridDim.x;
    const int x = (int)(blockIdx.x % tiles_x) * TW + (threadIdx.x & 63);
    const int y0 = (int)(blockIdx.x / tiles_x) * TH + (threadIdx.x >> 6);
    const uint8_t* cd = code + (long)blockIdx.z * hw;
    const double* up = u + plane * hw;
    double rr = 0.0, mx = 0.0;
    for (int j = 0; j < PX; ++j) {
        const int y = y0 + 4 * j;
        if (x < w && y < h) {
            const long o = (long)y * w + x;
            const int c = cd[o];
            const double v = (c & C_UNKNOWN) ? edge_residual(up, o, w, c) : 0.0;
            r[plane * hw + o] = v;
            rr = fma(v, v, rr);
            mx = nan_max(mx, fabs(v));
        }
    }
    rr = block_sum(rr, s);
    mx = block_max(mx, s);
    if (threadIdx.x == 0) {
        double* pp = part + plane * 3 * tiles;
        pp[blockIdx.x] = rr;
        pp[tiles + blockIdx.x] = mx;
        if (blockIdx.x == 0) scal[plane * 2] = Scalars{0.0, tol, 0, 0};
    }
}

// ---- one step --------------------------------------------------------------------------------------------------------------------------------
// p' of a pixel from the residual and the old direction; the one expression every workgroup uses, for its own pixels and for its halo
ADA_DEV double next_direction(const double* r, const double* p_old, long o, bool first, double beta) { return first ? r[o] : fma(beta, p_old[o], r[o]); }

__global__ __launch_bounds__(256) void mb_direction_kernel(const uint8_t* code, const double* r, double* p0, double* p1, double* q, int h, int w, int tiles_x,
                                                           double* part, Scalars* scal) {
    __shared__ double s[256];
    __shared__ double sp[(TH + 2) * (TW + 2)];
    const long hw = (long)h * w, plane = plane_of();
    const int tiles = gridDim.x;
    double* pp = part + plane * 3 * tiles;
    const Scalars in = scal[plane * 2];
    if (in.frozen) {
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[plane * 2 + 1] = in;
        return;
    }
    const double rr = tiles_sum(pp, tiles, s);
    const double mx = tiles_max(pp + tiles, tiles, s);
    const bool stop = !(mx > in.tol) || !(fabs(rr) <= 1.7976931348623157e308);      // reached tol (or a NaN), or r.r is not finite
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[plane * 2 + 1] = Scalars{rr, in.tol, stop ? 1 : 0, in.steps};
    if (stop) return;
    const bool first = in.steps == 0;
    const double beta = first ? 0.0 : rr / in.rr;
    const uint8_t* cd = code + (long)blockIdx.z * hw;
    const double* rp = r + plane * hw;
    const double* p_old = ((in.steps & 1) ? p1 : p0) + plane * hw;
    double* p_new = ((in.steps & 1) ? p0 : p1) + plane * hw;
    const int tx0 = (int)(blockIdx.x % tiles_x) * TW, ty0 = (int)(blockIdx.x / tiles_x) * TH;
    for (int i = threadIdx.x; i < (TH + 2) * (TW + 2); i += 256) {
        const int ly = i / (TW + 2), lx = i - ly * (TW + 2);
        const int y = ty0 + ly - 1, x = tx0 + lx - 1;
        double v = 0.0;      // outside the image, outside the domain and on a known pixel the direction is zero
        if (x >= 0 && x < w && y >= 0 && y < h) {
            const long o = (long)y * w + x;
            if (cd[o] & C_UNKNOWN) v = next_direction(rp, p_old, o, first, beta);
        }
        sp[i] = v;
    }
    __syncthreads();
    const int lx = (threadIdx.x & 63) + 1, x = tx0 + lx - 1;
    double pq = 0.0;
    for (int j = 0; j < PX; ++j) {
        const int ly = (threadIdx.x >> 6) + 4 * j + 1, y = ty0 + ly - 1;
        if (x < w && y < h) {
            const long o = (long)y * w + x;
            const int c = cd[o];
            if (c & C_UNKNOWN) {
                const double* t = sp + ly * (TW + 2) + lx;
                const double pc = t[0];
                const double deg = (double)__popc(c & C_EDGES);
                const double nb = ((t[-(TW + 2)] + t[TW + 2]) + t[-1]) + t[1];      // a missing edge's neighbour contributes the zero above
                const double a = fma(deg, pc, -nb);
                p_new[o] = pc;
                q[plane * hw + o] = a;
                pq = fma(pc, a, pq);
            }
        }
    }
    pq = block_sum(pq, s);
    if (threadIdx.x == 0) pp[2 * tiles + blockIdx.x] = pq;
}

__global__ __launch_bounds__(256) void mb_update_kernel(const uint8_t* code, double* u, double* r, const double* p0, const double* p1, const double* q, int h,
                                                        int w, int tiles_x, double* part, Scalars* scal) {
    __shared__ double s[256];
    const long hw = (long)h * w, plane = plane_of();
    const int tiles = gridDim.x;
    double* pp = part + plane * 3 * tiles;
    const Scalars in = scal[plane * 2 + 1];
    if (in.frozen) {
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[plane * 2] = in;
        return;
    }
    const double pq = tiles_sum(pp + 2 * tiles, tiles, s);
    const double alpha = in.rr / pq;
    const bool stop = !(pq > 0.0) || !(fabs(alpha) <= 1.7976931348623157e308);
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[plane * 2] = Scalars{in.rr, in.tol, stop ? 1 : 0, in.steps + (stop ? 0 : 1)};
    if (stop) return;
    const uint8_t* cd = code + (long)blockIdx.z * hw;
    const double* p = ((in.steps & 1) ? p0 : p1) + plane * hw;      // the buffer the direction kernel of this step wrote
    const int x = (int)(blockIdx.x % tiles_x) * TW + (threadIdx.x & 63);
    const int y0 = (int)(blockIdx.x / tiles_x) * TH + (threadIdx.x >> 6);
    double rr = 0.0, mx = 0.0;
    for (int j = 0; j < PX; ++j) {
        const int y = y0 + 4 * j;
        if (x < w && y < h) {
            const long o = (long)y * w + x;
            if (cd[o] & C_UNKNOWN) {
                const long po = plane * hw + o;
                u[po] = fma(alpha, p[o], u[po]);
                const double v = fma(-alpha, q[po], r[po]);
                r[po] = v;
                rr = fma(v, v, rr);
                mx = nan_max(mx, fabs(v));
            }
        }
    }
    rr = block_sum(rr, s);
    mx = block_max(mx, s);
    if (threadIdx.x == 0) {
        pp[blockIdx.x] = rr;
        pp[tiles + blockIdx.x] = mx;
    }
}

// grid (ceil(planes / 256)): the planes' frozen flags as bytes, for a caller that wants to stop issuing steps
__global__ __launch_bounds__(256) void mb_frozen_kernel(const Scalars* scal, long planes, uint8_t* frozen) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < planes) frozen[i] = scal[i * 2].frozen ? 1 : 0;
}

// ---- end -------------------------------------------------------------------------------------------------------------------------------------
// grid (tiles, channels, batch): the outputs and the tile's max of the TRUE residual |b - A u|, evaluated from u itself
__global__ __launch_bounds__(256) void mb_output_kernel(const uint8_t* code, const double* u, const uint32_t* x, const float* plus, int h, int w, int tiles_x,
                                                        uint32_t* out, double* out64, double* part) {
    __shared__ double s[256];
    const long hw = (long)h * w, plane = plane_of();
    const int tiles = gridDim.x;
    const int xx = (int)(blockIdx.x % tiles_x) * TW + (threadIdx.x & 63);
    const int y0 = (int)(blockIdx.x / tiles_x) * TH + (threadIdx.x >> 6);
    const uint8_t* cd = code + (long)blockIdx.z * hw;
    const double* up = u + plane * hw;
    double mx = 0.0;
    for (int j = 0; j < PX; ++j) {
        const int y = y0 + 4 * j;
        if (xx < w && y < h) {
            const long o = (long)y * w + xx, po = plane * hw + o;
            const int c = cd[o];
            if (c & C_UNKNOWN) {
                mx = nan_max(mx, fabs(edge_residual(up, o, w, c)));
                const double v = plus ? up[o] + (double)plus[po] : up[o];
                if (out) out[po] = __builtin_bit_cast(uint32_t, (float)v);
                if (out64) out64[po] = v;
            } else {
                const uint32_t bits = x[po];      // moved as a word: every bit stays
                if (out) out[po] = bits;
                if (out64) out64[po] = (double)__builtin_bit_cast(float, bits);
            }
        }
    }
    mx = block_max(mx, s);
    if (threadIdx.x == 0) part[plane * 3 * tiles + tiles + blockIdx.x] = mx;      // the recurrence's max |r| is of no use any more
}

// grid (channels, batch), one workgroup per plane: the plane's report
__global__ __launch_bounds__(256) void mb_report_kernel(const double* part, const Scalars* scal, int tiles, double* residual, int32_t* iterations,
                                                        uint8_t* converged) {
    __shared__ double s[256];
    const long plane = (long)blockIdx.y * gridDim.x + blockIdx.x;
    const double mx = tiles_max(part + plane * 3 * tiles + tiles, tiles, s);
    if (threadIdx.x == 0) {
        const Scalars in = scal[plane * 2];
        residual[plane] = mx;
        iterations[plane] = in.steps;
        converged[plane] = mx <= in.tol ? 1 : 0;
    }
}

int check_shape(const char* who, int32_t batch, int32_t channels, int32_t h, int32_t w) {
    ADA_REQUIRE(batch > 0 && channels > 0 && h > 0 && w > 0, ADA_EINVAL, "%s: bad shape batch=%d channels=%d %dx%d", who, batch, channels, h, w);
    ADA_REQUIRE(h <= 32767 && w <= 32767, ADA_EUNSUPPORTED, "%s: h and w must stay within 32767, got %dx%d", who, h, w);
    ADA_REQUIRE(batch <= 65535 && channels <= 65535, ADA_EUNSUPPORTED, "%s: batch and channels must stay within 65535, got %d and %d", who, batch, channels);
    return ADA_OK;
}

int check_workspace(const char* who, int32_t batch, int32_t channels, int32_t h, int32_t w, void* workspace, int64_t workspace_bytes, Layout* L) {
    *L = layout(workspace, batch, channels, h, w);
    ADA_REQUIRE(workspace && workspace_bytes >= L->bytes, ADA_EINVAL, "%s: the workspace needs %ld bytes, got %ld", who, (long)L->bytes,
                (long)(workspace ? workspace_bytes : 0));
    ADA_REQUIRE(((uintptr_t)workspace & 7) == 0, ADA_EINVAL, "%s: the workspace must be 8-byte aligned", who);
    return ADA_OK;
}

}  // namespace

extern "C" int ada_membrane_workspace_bytes(int32_t batch, int32_t channels, int32_t h, int32_t w, int64_t* bytes) {
    ADA_REQUIRE(bytes, ADA_EINVAL, "ada_membrane_workspace_bytes: null pointer");
    if (int rc = check_shape("ada_membrane_workspace_bytes", batch, channels, h, w)) return rc;
    *bytes = layout(nullptr, batch, channels, h, w).bytes;
    return ADA_OK;
}

extern "C" int ada_membrane_begin_fwd(const float* x, const float* minus, const uint8_t* known, const uint8_t* domain, const float* guess, int32_t batch,
                                      int32_t channels, int32_t h, int32_t w, double tol, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "ada_membrane_begin_fwd";
    ADA_REQUIRE(x && known, ADA_EINVAL, "%s: null pointer", who);
    if (int rc = check_shape(who, batch, channels, h, w)) return rc;
    ADA_REQUIRE(tol >= 0.0 && tol <= 1.7976931348623157e308, ADA_EINVAL, "%s: tol must be finite and not negative, got %g", who, tol);
    Layout L;
    if (int rc = check_workspace(who, batch, channels, h, w, workspace, workspace_bytes, &L)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const int tiles_x = (w + TW - 1) / TW;
    const unsigned tiles = (unsigned)n_tiles(h, w);
    hipLaunchKernelGGL(mb_setup_kernel, dim3((unsigned)(((long)h * w + 255) / 256), (unsigned)channels, (unsigned)batch), dim3(256), 0, s, x, minus, known, domain,
                       guess, h, w, L.code, L.u);
    hipLaunchKernelGGL(mb_residual0_kernel, dim3(tiles, (unsigned)channels, (unsigned)batch), dim3(256), 0, s, (const uint8_t*)L.code, (const double*)L.u, h, w,
                       tiles_x, tol, L.r, L.part, L.scal);
    return ada_check_launch(who);
}

extern "C" int ada_membrane_iterate_fwd(int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t iterations, uint8_t* frozen, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    const char* who = "ada_membrane_iterate_fwd";
    if (int rc = check_shape(who, batch, channels, h, w)) return rc;
    ADA_REQUIRE(iterations >= 0, ADA_EINVAL, "%s: iterations must not be negative, got %d", who, iterations);
    Layout L;
    if (int rc = check_workspace(who, batch, channels, h, w, workspace, workspace_bytes, &L)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const int tiles_x = (w + TW - 1) / TW;
    const dim3 grid((unsigned)n_tiles(h, w), (unsigned)channels, (unsigned)batch);
    for (int i = 0; i < iterations; ++i) {
        hipLaunchKernelGGL(mb_direction_kernel, grid, dim3(256), 0, s, (const uint8_t*)L.code, (const double*)L.r, L.p0, L.p1, L.q, h, w, tiles_x, L.part, L.scal);
        hipLaunchKernelGGL(mb_update_kernel, grid, dim3(256), 0, s, (const uint8_t*)L.code, L.u, L.r, (const double*)L.p0, (const double*)L.p1,
                           (const double*)L.q, h, w, tiles_x, L.part, L.scal);
    }
    if (frozen) {
        const long planes = (long)batch * channels;
        hipLaunchKernelGGL(mb_frozen_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, s, (const Scalars*)L.scal, planes, frozen);
    }
    return ada_check_launch(who);
}

extern "C" int ada_membrane_end_fwd(const float* x, const float* plus, int32_t batch, int32_t channels, int32_t h, int32_t w, float* out, double* out64,
                                    double* residual, int32_t* iterations, uint8_t* converged, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "ada_membrane_end_fwd";
    ADA_REQUIRE(x && (out || out64) && residual && iterations && converged, ADA_EINVAL, "%s: null pointer", who);
    if (int rc = check_shape(who, batch, channels, h, w)) return rc;
    Layout L;
    if (int rc = check_workspace(who, batch, channels, h, w, workspace, workspace_bytes, &L)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const int tiles_x = (w + TW - 1) / TW;
    const unsigned tiles = (unsigned)n_tiles(h, w);
    hipLaunchKernelGGL(mb_output_kernel, dim3(tiles, (unsigned)channels, (unsigned)batch), dim3(256), 0, s, (const uint8_t*)L.code, (const double*)L.u,
                       (const uint32_t*)x, plus, h, w, tiles_x, (uint32_t*)out, out64, L.part);
    hipLaunchKernelGGL(mb_report_kernel, dim3((unsigned)channels, (unsigned)batch), dim3(256), 0, s, (const double*)L.part, (const Scalars*)L.scal, (int)tiles,
                       residual, iterations, converged);
    return ada_check_launch(who);
}
