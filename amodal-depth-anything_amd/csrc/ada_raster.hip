// Meshes seen from a camera on the device: a z-buffer rasteriser for the meshes of ada_geometry.hip.  The reference hands its meshes to a third-party
// renderer, so the arithmetic is this library's own; include/ada_hip.h states it exactly and tests/_raster_ref.py restates it in numpy.
//
// Vertex stage.  One thread per vertex, fp64 with every product, sum and quotient rounded on its own (__dmul_rn / __dadd_rn, and the file is built with
// -ffp-contract=off): optional pose, pinhole projection, validity, the snap to 1/256 pixel (round half to even) and w = 1 / z.  The records are three
// arrays (X, Y, w), so the triangle setup's gathers touch 4- and 8-byte words of lines that neighbouring triangles share.  w == 0 marks an invalid vertex.
//
// Coverage.  Integer edge functions on the snapped coordinates (int64; the guard band keeps every product below 2^47), inclusive edges.  The winner at a
// sample is decided by ONE 64-bit unsigned maximum: bits(float32(w)) << 32 | (0xFFFFFFFF - id).  w > 0, so the float's bits order as the float does, and
// the low word makes the lowest id win a tie.  A maximum does not depend on the order of arrival: the outputs are the same bytes every run.  A candidate
// is first compared with a plain (L1-bypassing) load of the key: the word only grows, so whatever that load returns is a value the key really had, and a
// candidate not above it can never win.
//
// Work distribution, three classes by the number of samples in the triangle's screen-clipped box:
//   <= ADA_RASTER_SMALL_MAX   the triangle's own thread walks the box in the binning launch: at most that many iterations, whatever the mesh
//   <= ADA_RASTER_WAVE_MAX    appended to the front of a device list; one WAVE of the walking launch takes the whole box in tiles of 8 x 8 samples
//   larger                    appended to the back of the same list; a team of workgroups of the walking launch shares the box in tiles of
//                             ADA_RASTER_TILE_W x ADA_RASTER_TILE_H samples, t = rank, rank + team, ...  The launch's ADA_RASTER_WALK_BLOCKS workgroups
//                             form min(largest power of two <= entries, WALK_BLOCKS / ADA_RASTER_WALK_SHARE) teams and team k takes the entries
//                             k, k + teams, ...: two screen-filling triangles get half the device each, and among thousands of large triangles no
//                             workgroup reads more than its team's share of setups and none has a whole screen to itself.
// A tile is one sample per thread and is rejected as a whole when one edge function is negative at all four of its corners (the functions are linear).
// Appending is one ballot per class and wave and one counter add by its first flagged lane (wave_append, on ada_scan.h's lanes_below).  The
// walking launch has a fixed grid; no launch's running time depends on one thread's triangle.
//
// Resolve.  One thread per pixel recomputes the winner's edge functions and fp64 interpolants from its id and writes index, depth and colour.
//
// Clear, bin, walk, resolve: four launches fixed by the shapes alone, nothing read back: legal inside a stream capture.
#include "ada_scan.h"

namespace {

constexpr int RAST_THREADS = 256;
constexpr int RAST_WAVE = ADA_WAVE;
constexpr int SMALL_MAX = ADA_RASTER_SMALL_MAX;
constexpr int WAVE_MAX = ADA_RASTER_WAVE_MAX;
constexpr int TILE_W = ADA_RASTER_TILE_W, TILE_H = ADA_RASTER_TILE_H;      // a workgroup's tile
constexpr int WAVE_TILE = 8;                                               // a wave's tile: 8 x 8
constexpr int WALK_BLOCKS = ADA_RASTER_WALK_BLOCKS;
constexpr int WALK_SHARE = ADA_RASTER_WALK_SHARE;
constexpr int RAST_WAVES = RAST_THREADS / RAST_WAVE;
constexpr int SUB = 256;                 // snapped units per pixel
static_assert(TILE_W * TILE_H == RAST_THREADS && WAVE_TILE * WAVE_TILE == RAST_WAVE && SMALL_MAX >= 1 && WAVE_MAX > SMALL_MAX, "layout");
static_assert(WALK_BLOCKS % WALK_SHARE == 0 && ((WALK_BLOCKS / WALK_SHARE) & (WALK_BLOCKS / WALK_SHARE - 1)) == 0, "the teams are a power of two");

// ------------------------------------------------------------------ vertex stage
struct ProjectArgs {
    const void* points;      // [n][3] fp32 or fp64
    int point_bytes;
    int n;
    int pose;                // 0: q = p exactly
    double fx, fy, cx, cy;
    double rot[9], t[3];
    int32_t* X;
    int32_t* Y;
    double* W;
};

ADA_DEV bool finite64(double v) { return __builtin_fabs(v) < __builtin_inf(); }     // false for NaN

__global__ __launch_bounds__(RAST_THREADS) void project_kernel(ProjectArgs a) {
    const long v = (long)blockIdx.x * RAST_THREADS + threadIdx.x;
    if (v >= a.n) return;
    double p0, p1, p2;
    if (a.point_bytes == 4) {
        const float* p = (const float*)a.points + 3 * v;
        p0 = (double)p[0]; p1 = (double)p[1]; p2 = (double)p[2];
    } else {
        const double* p = (const double*)a.points + 3 * v;
        p0 = p[0]; p1 = p[1]; p2 = p[2];
    }
    double q0 = p0, q1 = p1, q2 = p2;
    if (a.pose) {
        q0 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.rot[0], p0), __dmul_rn(a.rot[1], p1)), __dmul_rn(a.rot[2], p2)), a.t[0]);
        q1 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.rot[3], p0), __dmul_rn(a.rot[4], p1)), __dmul_rn(a.rot[5], p2)), a.t[1]);
        q2 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.rot[6], p0), __dmul_rn(a.rot[7], p1)), __dmul_rn(a.rot[8], p2)), a.t[2]);
    }
    bool ok = finite64(q0) && finite64(q1) && finite64(q2) && q2 >= 0x1p-64 && q2 <= 0x1p64;
    double u = 0.0, w = 0.0, vv = 0.0;
    if (ok) {
        u = __dadd_rn(__dmul_rn(a.fx, (-q0) / q2), a.cx);      // the correctly rounded quotient: no fast-math flag in this build
        vv = __dadd_rn(__dmul_rn(a.fy, (-q1) / q2), a.cy);
        ok = __builtin_fabs(u) <= 16384.0 && __builtin_fabs(vv) <= 16384.0;      // false for NaN (a non-finite K)
        w = 1.0 / q2;
    }
    a.X[v] = ok ? (int32_t)__builtin_rint(__dmul_rn(256.0, u)) : 0;      // round half to even; |256 u| <= 2^22
    a.Y[v] = ok ? (int32_t)__builtin_rint(__dmul_rn(256.0, vv)) : 0;
    a.W[v] = ok ? w : 0.0;
}

// ------------------------------------------------------------------ triangles
struct RasterArgs {
    const int32_t* X;
    const int32_t* Y;
    const double* W;
    const uint8_t* colors;   // [nvert][3] or NULL
    int nvert;
    const int32_t* tri;      // [ntri][3]
    int ntri;
    int h, w;
    int mode;                // ADA_RASTER_OUT_*
    double a, b;
    float fill;
    uint32_t fill_rgb;       // r | g << 8 | b << 16
    float* depth;            // [h][w]
    int32_t* index;          // [h][w]
    uint8_t* color;          // [h][w][3] or NULL
    unsigned long long* keys;      // [h w]
    int32_t* counters;       // [0] triangles of the middle class, [1] of the large class
    int32_t* list;           // [ntri]: the middle class from the front, the large class from the back
};

struct Tri {
    int X0, Y0, X1, Y1, X2, Y2;
    double w0, w1, w2;
    long A;                  // signed doubled area in snapped units
    int jmin, jmax, imin, imax;      // the screen-clipped box of samples; empty when jmin > jmax or imin > imax
};

// false: the triangle is dropped (an index outside [0, nvert), an invalid vertex, no area)
ADA_DEV bool tri_setup(const RasterArgs& a, int id, Tri& t) {
    const int32_t* ix = a.tri + 3l * id;
    const int i0 = ix[0], i1 = ix[1], i2 = ix[2];
    if ((uint32_t)i0 >= (uint32_t)a.nvert || (uint32_t)i1 >= (uint32_t)a.nvert || (uint32_t)i2 >= (uint32_t)a.nvert) return false;
    t.w0 = a.W[i0]; t.w1 = a.W[i1]; t.w2 = a.W[i2];
    if (!(t.w0 > 0.0 && t.w1 > 0.0 && t.w2 > 0.0)) return false;
    t.X0 = a.X[i0]; t.Y0 = a.Y[i0]; t.X1 = a.X[i1]; t.Y1 = a.Y[i1]; t.X2 = a.X[i2]; t.Y2 = a.Y[i2];
    t.A = (long)(t.X1 - t.X0) * (t.Y2 - t.Y0) - (long)(t.X2 - t.X0) * (t.Y1 - t.Y0);
    if (t.A == 0) return false;
    const int xlo = min(t.X0, min(t.X1, t.X2)), xhi = max(t.X0, max(t.X1, t.X2));
    const int ylo = min(t.Y0, min(t.Y1, t.Y2)), yhi = max(t.Y0, max(t.Y1, t.Y2));
    t.jmin = max(0, (xlo + SUB - 1) >> 8); t.jmax = min(a.w - 1, xhi >> 8);      // arithmetic shifts: ceiling and floor, also below zero
    t.imin = max(0, (ylo + SUB - 1) >> 8); t.imax = min(a.h - 1, yhi >> 8);
    return true;
}

// the three edge functions at the sample of column j, row i, signed so that inside is >= 0; true when the sample is covered.  Samples are only ever
// taken within a tile of the triangle's box, where |256 j - X| < 2^24: the differences fit int32 and the products int64.
ADA_DEV bool tri_edges(const Tri& t, int j, int i, long& e0, long& e1, long& e2) {
    const int sx = SUB * j, sy = SUB * i;
    e0 = (long)(t.X2 - t.X1) * (sy - t.Y1) - (long)(t.Y2 - t.Y1) * (sx - t.X1);
    e1 = (long)(t.X0 - t.X2) * (sy - t.Y2) - (long)(t.Y0 - t.Y2) * (sx - t.X2);
    e2 = t.A - e0 - e1;
    if (t.A < 0) { e0 = -e0; e1 = -e1; e2 = -e2; }
    return (e0 | e1 | e2) >= 0;
}

ADA_DEV double tri_w(const Tri& t, long e1, long e2) {
    const double area = (double)(t.A < 0 ? -t.A : t.A);
    const double num = __dadd_rn(__dmul_rn((double)e1, __dsub_rn(t.w1, t.w0)), __dmul_rn((double)e2, __dsub_rn(t.w2, t.w0)));
    return __dadd_rn(t.w0, num / area);
}

ADA_DEV void candidate(const RasterArgs& a, const Tri& t, int id, int j, int i) {
    long e0, e1, e2;
    if (!tri_edges(t, j, i, e0, e1, e2)) return;
    const float wf = (float)tri_w(t, e1, e2);      // round to nearest even
    const unsigned long long key = ((unsigned long long)__float_as_uint(wf) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)id);
    unsigned long long* p = a.keys + ((long)i * a.w + j);
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= key) return;
    __hip_atomic_fetch_max(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one ballot, one counter add by the wave's first flagged lane; returns this lane's position in the class (meaningful where flag is set).  An atomic
// append on purpose, unlike the ordered compaction of ada_scan.h, from which it takes only lanes_below: the order of the list cannot reach the output
ADA_DEV int wave_append(int32_t* counter, bool flag) {
    const uint64_t bal = __ballot(flag);
    if (bal == 0) return 0;
    const int leader = __builtin_ctzll(bal);
    int base = 0;
    if ((int)(threadIdx.x & (RAST_WAVE - 1)) == leader) base = atomicAdd(counter, (int32_t)__popcll(bal));
    base = __shfl(base, leader, RAST_WAVE);
    return base + lanes_below(bal);
}

__global__ __launch_bounds__(RAST_THREADS) void clear_kernel(unsigned long long* keys, long n, int32_t* counters) {
    const long i = 2 * ((long)blockIdx.x * RAST_THREADS + threadIdx.x);      // keys is 16-byte aligned (checked on the host)
    if (i + 1 < n) *reinterpret_cast<ulonglong2*>(keys + i) = make_ulonglong2(0ull, 0ull);
    else if (i < n) keys[i] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x < 2) counters[threadIdx.x] = 0;
}

__global__ __launch_bounds__(RAST_THREADS) void bin_kernel(RasterArgs a) {
    const long gid = (long)blockIdx.x * RAST_THREADS + threadIdx.x;
    const int id = (int)gid;
    Tri t;
    long count = 0;
    if (gid < a.ntri && tri_setup(a, id, t) && t.jmin <= t.jmax && t.imin <= t.imax) count = (long)(t.jmax - t.jmin + 1) * (t.imax - t.imin + 1);
    const bool middle = count > SMALL_MAX && count <= WAVE_MAX, large = count > WAVE_MAX;
    const int pm = wave_append(a.counters, middle);
    const int pl = wave_append(a.counters + 1, large);
    if (middle) a.list[pm] = id;                     // the two classes together hold at most ntri entries: they never meet
    if (large) a.list[a.ntri - 1 - pl] = id;
    if (count >= 1 && count <= SMALL_MAX) {
        int j = t.jmin, i = t.imin;
        for (int s = 0; s < (int)count; ++s) {
            candidate(a, t, id, j, i);
            if (++j > t.jmax) { j = t.jmin; ++i; }
        }
    }
}

// the tiles first, first + step, ... of the triangle's box, each TW x TH samples, one per thread of the team (``t``: this thread's place in it)
template <int TW, int TH>
ADA_DEV void walk_box(const RasterArgs& a, int id, int first, int step, int t_in_team) {
    Tri t;
    if (!tri_setup(a, id, t)) return;                // never taken: the binning launch listed it
    const int tiles_x = (t.jmax - t.jmin) / TW + 1, tiles_y = (t.imax - t.imin) / TH + 1;
    const int ntiles = tiles_x * tiles_y;            // <= (2^14 / 8 + 1)^2
    const int tx = t_in_team % TW, ty = t_in_team / TW;
    for (int tile = first; tile < ntiles; tile += step) {
        const int row = tile / tiles_x, col = tile - row * tiles_x;
        const int j0 = t.jmin + col * TW, i0 = t.imin + row * TH;
        const int j1 = min(j0 + TW - 1, t.jmax), i1 = min(i0 + TH - 1, t.imax);
        long p0, p1, p2, q0, q1, q2, r0, r1, r2, s0, s1, s2;
        tri_edges(t, j0, i0, p0, p1, p2); tri_edges(t, j1, i0, q0, q1, q2); tri_edges(t, j0, i1, r0, r1, r2); tri_edges(t, j1, i1, s0, s1, s2);
        if ((p0 & q0 & r0 & s0) < 0 || (p1 & q1 & r1 & s1) < 0 || (p2 & q2 & r2 & s2) < 0) continue;      // one edge has the whole tile outside
        const int j = j0 + tx, i = i0 + ty;
        if (j <= j1 && i <= i1) candidate(a, t, id, j, i);
    }
}

__global__ __launch_bounds__(RAST_THREADS) void walk_kernel(RasterArgs a) {
    const int n_middle = min(max(a.counters[0], 0), a.ntri), n_large = min(max(a.counters[1], 0), a.ntri - n_middle);
    const int wave = blockIdx.x * RAST_WAVES + threadIdx.x / RAST_WAVE, nwaves = gridDim.x * RAST_WAVES;      // no barrier below: the waves go their own ways
    for (int e = wave; e < n_middle; e += nwaves) walk_box<WAVE_TILE, WAVE_TILE>(a, a.list[e], 0, 1, threadIdx.x & (RAST_WAVE - 1));
    if (n_large == 0) return;
    const int teams = min(1 << (31 - __clz(n_large)), (int)gridDim.x / WALK_SHARE), team_size = gridDim.x / teams;      // both powers of two
    const int team = blockIdx.x / team_size, rank = blockIdx.x - team * team_size;
    for (int e = team; e < n_large; e += teams) walk_box<TILE_W, TILE_H>(a, a.list[a.ntri - 1 - e], rank, team_size, threadIdx.x);
}

__global__ __launch_bounds__(RAST_THREADS) void resolve_kernel(RasterArgs a) {
    const long pix = (long)blockIdx.x * RAST_THREADS + threadIdx.x;
    if (pix >= (long)a.h * a.w) return;
    const unsigned long long key = a.keys[pix];
    int id = -1;
    float d = a.fill;
    uint32_t r = a.fill_rgb & 255u, g = (a.fill_rgb >> 8) & 255u, bl = (a.fill_rgb >> 16) & 255u;
    Tri t;
    if (key != 0ull) {
        id = (int)(0xFFFFFFFFu - (uint32_t)key);
        if ((uint32_t)id >= (uint32_t)a.ntri || !tri_setup(a, id, t)) id = -1;      // never taken: only listed triangles write keys
    }
    if (id >= 0) {
        const int i = (int)(pix / a.w), j = (int)(pix - (long)i * a.w);
        long e0, e1, e2;
        tri_edges(t, j, i, e0, e1, e2);
        const double w = tri_w(t, e1, e2);
        d = a.mode == ADA_RASTER_OUT_W ? (float)w : a.mode == ADA_RASTER_OUT_Z ? (float)(1.0 / w) : (float)(__dsub_rn(w, a.b) / a.a);
        if (a.color) {
            const int32_t* ix = a.tri + 3l * id;
            const uint8_t* c0 = a.colors + 3l * ix[0];
            const uint8_t* c1 = a.colors + 3l * ix[1];
            const uint8_t* c2 = a.colors + 3l * ix[2];
            const double n0 = __dmul_rn((double)e0, t.w0), n1 = __dmul_rn((double)e1, t.w1), n2 = __dmul_rn((double)e2, t.w2);
            const double den = __dadd_rn(__dadd_rn(n0, n1), n2);
            uint32_t out[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double ch = __dadd_rn(__dadd_rn(__dmul_rn(n0, (double)c0[k]), __dmul_rn(n1, (double)c1[k])), __dmul_rn(n2, (double)c2[k])) / den;
                out[k] = (uint32_t)fmin(255.0, __builtin_floor(__dadd_rn(ch, 0.5)));
            }
            r = out[0]; g = out[1]; bl = out[2];
        }
    }
    a.index[pix] = id;
    a.depth[pix] = d;
    if (a.color) { a.color[3 * pix] = (uint8_t)r; a.color[3 * pix + 1] = (uint8_t)g; a.color[3 * pix + 2] = (uint8_t)bl; }
}

}  // namespace

extern "C" int ada_mesh_project_fwd(const void* points, int32_t point_bytes, int32_t n_vertices, const double* camera, int32_t pose, int32_t* x,
                                    int32_t* y, double* w, void* stream) {
    ADA_REQUIRE(n_vertices >= 0, ADA_EINVAL, "ada_mesh_project_fwd: n_vertices=%d", n_vertices);
    ADA_REQUIRE(camera && (n_vertices == 0 || (points && x && y && w)), ADA_EINVAL, "ada_mesh_project_fwd: null pointer");
    ADA_REQUIRE(point_bytes == 4 || point_bytes == 8, ADA_EINVAL, "ada_mesh_project_fwd: point_bytes=%d (4: fp32, 8: fp64)", point_bytes);
    ADA_REQUIRE(pose == 0 || pose == 1, ADA_EINVAL, "ada_mesh_project_fwd: pose=%d (0 or 1)", pose);
    if (n_vertices == 0) return 0;
    ProjectArgs p;
    p.points = points; p.point_bytes = point_bytes; p.n = n_vertices; p.pose = pose;
    p.fx = camera[0]; p.fy = camera[1]; p.cx = camera[2]; p.cy = camera[3];      // host pointer, taken by value here
    for (int i = 0; i < 9; ++i) p.rot[i] = camera[4 + i];
    for (int i = 0; i < 3; ++i) p.t[i] = camera[13 + i];
    p.X = x; p.Y = y; p.W = w;
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((n_vertices + RAST_THREADS - 1) / RAST_THREADS)), dim3(RAST_THREADS), 0, (hipStream_t)stream, p);
    return ada_check_launch("ada_mesh_project_fwd");
}

extern "C" int ada_mesh_raster_fwd(const int32_t* x, const int32_t* y, const double* w, const uint8_t* colors, int32_t n_vertices,
                                   const int32_t* triangles, int32_t n_triangles, int32_t height, int32_t width, int32_t mode, double a, double b,
                                   float fill, uint32_t fill_rgb, float* depth, int32_t* index, uint8_t* color, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(n_vertices >= 0 && n_triangles >= 0, ADA_EINVAL, "ada_mesh_raster_fwd: n_vertices=%d n_triangles=%d", n_vertices, n_triangles);
    ADA_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width < ((int64_t)1 << 30), ADA_EINVAL,
                "ada_mesh_raster_fwd: height=%d width=%d outside h, w >= 1 / h * w < 2^30", height, width);
    ADA_REQUIRE(depth && index && workspace && (n_triangles == 0 || (triangles && n_vertices > 0)) && (n_vertices == 0 || (x && y && w)), ADA_EINVAL,
                "ada_mesh_raster_fwd: null pointer");
    ADA_REQUIRE(!color || colors || n_triangles == 0, ADA_EINVAL, "ada_mesh_raster_fwd: a color output needs the vertex colors");
    ADA_REQUIRE(mode == ADA_RASTER_OUT_W || mode == ADA_RASTER_OUT_Z || mode == ADA_RASTER_OUT_NORMALISED, ADA_EINVAL, "ada_mesh_raster_fwd: mode=%d", mode);
    ADA_REQUIRE(mode != ADA_RASTER_OUT_NORMALISED || (a == a && b == b && a != 0.0), ADA_EINVAL, "ada_mesh_raster_fwd: normalised output needs a != 0");
    const int64_t hw = (int64_t)height * width;
    const int64_t hw2 = hw + (hw & 1);      // the counters and the list start 16-byte aligned
    const int64_t need = 8 * hw2 + 16 + 4 * (int64_t)n_triangles;
    ADA_REQUIRE(workspace_bytes >= need && (uintptr_t)workspace % 16 == 0, ADA_EINVAL,
                "ada_mesh_raster_fwd: a 16-byte aligned workspace of %ld bytes needed, got %ld", (long)need, (long)workspace_bytes);
    const hipStream_t s = (hipStream_t)stream;
    RasterArgs r;
    r.X = x; r.Y = y; r.W = w; r.colors = colors; r.nvert = n_vertices; r.tri = triangles; r.ntri = n_triangles; r.h = height; r.w = width;
    r.mode = mode; r.a = a; r.b = b; r.fill = fill; r.fill_rgb = fill_rgb; r.depth = depth; r.index = index; r.color = color;
    r.keys = (unsigned long long*)workspace;
    r.counters = (int32_t*)((char*)workspace + 8 * hw2);
    r.list = r.counters + 4;
    const unsigned pixel_blocks = (unsigned)((hw + RAST_THREADS - 1) / RAST_THREADS);
    hipLaunchKernelGGL(clear_kernel, dim3((unsigned)((hw + 2 * RAST_THREADS - 1) / (2 * RAST_THREADS))), dim3(RAST_THREADS), 0, s, r.keys, (long)hw, r.counters);
    if (n_triangles > 0) {
        hipLaunchKernelGGL(bin_kernel, dim3((unsigned)((n_triangles + RAST_THREADS - 1) / RAST_THREADS)), dim3(RAST_THREADS), 0, s, r);
        hipLaunchKernelGGL(walk_kernel, dim3(WALK_BLOCKS), dim3(RAST_THREADS), 0, s, r);
    }
    hipLaunchKernelGGL(resolve_kernel, dim3(pixel_blocks), dim3(RAST_THREADS), 0, s, r);
    return ada_check_launch("ada_mesh_raster_fwd");
}
