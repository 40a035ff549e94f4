// Depth maps to geometry on the device: the unprojection, the masked triangle list and the vertex compaction that the reference does on the host
// in numpy (reference src/models/amodalsynthdrive/zoedepth/utils/geometry.py: depth_to_points, create_triangles).
//
// Points.  One thread per pixel, x from the thread's index, y from the block's: no division.  All arithmetic is fp64 with every product and sum rounded
// (__dmul_rn / __dadd_rn, and the file is built with -ffp-contract=off): for the default pose this is numpy's result bit for bit, see include/ada_hip.h.
// A workgroup owns 256 consecutive pixels of one row; their 768 coordinates go through LDS so that the stores are 16 bytes per lane over one contiguous
// span (a lane's own three coordinates are 12 or 24 bytes, which no store instruction covers without splitting lines between lanes).
//
// Triangles.  The candidates are two per pixel cell in raster order; a kept one is a predicate of its three vertices (tri_flags, ONE function used
// by the counting and the writing pass; the depth -> z rule is ada_mesh_rule.h's).  Order-preserving compaction with the pieces of ada_scan.h, in three
// launches, none waiting on another workgroup:
//   count    a workgroup owns GEOM_CHUNK consecutive cells and sums their kept candidates into sums[image][workgroup]
//   scan     scan_sums_kernel<1>, one workgroup per image: exclusive offsets in place, the total to count[image]
//   scatter  the count pass again: a round of 256 cells takes two ballots per lane (a cell's first and second triangle) and waves_before; a lane's
//            position = offset + the rounds before + the waves before + the lanes below; rows at or beyond `capacity` are dropped
//
// Compaction of the vertices: clear, mark (every referenced vertex gets a 1: a plain store of one value, order-free), the same count / scan over chunks of
// vertices, gather (new index = offset + block_excl_flag of the marks; the point and the colour move there) and remap of the triangle indices in place.
//
// Every launch sequence is fixed by the shapes alone; nothing is read back: all three calls are legal inside a stream capture.
#include "ada_mesh_rule.h"
#include "ada_scan.h"

namespace {

constexpr int GEOM_WAVE = ADA_GEOM_WAVE;
constexpr int GEOM_THREADS = 256;
constexpr int GEOM_CHUNK = ADA_GEOM_CHUNK;             // cells (or vertices) per workgroup of the count / scatter passes
constexpr int GEOM_SUB = GEOM_CHUNK / GEOM_THREADS;    // a thread's cells: t, t + 256, ...
constexpr int GEOM_WAVES = GEOM_THREADS / GEOM_WAVE;
// the published step of the scan is scan_sums_kernel<1>'s: one sum per thread
static_assert(GEOM_WAVE == ADA_WAVE && GEOM_CHUNK % GEOM_THREADS == 0 && ADA_GEOM_SCAN_BLOCK == SCAN_THREADS * 1, "layout");

// ------------------------------------------------------------------ points
struct PointArgs {
    const float* depth;      // [batch][h][w]
    double* out64;           // [batch][h][w][3] or NULL
    float* out32;            // [batch][h][w][3] or NULL
    uint8_t* valid;          // [batch][h][w] or NULL
    int h, w;
    ZRule z;
    double kinv[9], rot[9], t[3];
};

// the span [base, base + n) of out <- lds[0, n): head elements up to the first 16-byte boundary one per lane, then 16 bytes per lane, then the tail
template <typename T>
ADA_DEV void store_span(T* out, long base, int n, const T* lds) {
    constexpr int V = 16 / (int)sizeof(T);
    int head = (int)((V - (base % V)) % V);      // out itself is 16-byte aligned (checked on the host)
    if (head > n) head = n;
    const int nvec = (n - head) / V;
    const int t = threadIdx.x;
    if (t < head) out[base + t] = lds[t];
    for (int v = t; v < nvec; v += GEOM_THREADS) {
        const int e = head + v * V;
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(out + base + e) = make_float4(lds[e], lds[e + 1], lds[e + 2], lds[e + 3]);
        } else {
            *reinterpret_cast<double2*>(out + base + e) = make_double2(lds[e], lds[e + 1]);
        }
    }
    const int done = head + nvec * V;
    if (t < n - done) out[base + done + t] = lds[done + t];
}

__global__ __launch_bounds__(GEOM_THREADS) void points_kernel(PointArgs a) {
    __shared__ double s64[GEOM_THREADS * 3];
    float* s32 = reinterpret_cast<float*>(s64);          // the fp32 form reuses the words once the fp64 form is stored
    const int x0 = blockIdx.x * GEOM_THREADS;
    const int x = x0 + threadIdx.x;
    const int n = min(GEOM_THREADS, a.w - x0);
    const long image = (long)blockIdx.z * a.h * a.w;
    for (int y = blockIdx.y; y < a.h; y += gridDim.y) {
        const long row = image + (long)y * a.w;
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;
        if (x < a.w) {
            const double z = z_of(a.z, a.depth[row + x]);
            const double fx = (double)x, fy = (double)y;
            double p[3];
#pragma unroll
            for (int i = 0; i < 3; ++i)      // ((z K[i,0]) x + (z K[i,1]) y) + (z K[i,2]) 1, every operation rounded
                p[i] = __dadd_rn(__dadd_rn(__dmul_rn(__dmul_rn(z, a.kinv[3 * i]), fx), __dmul_rn(__dmul_rn(z, a.kinv[3 * i + 1]), fy)),
                                 __dmul_rn(z, a.kinv[3 * i + 2]));
            const double q0 = -p[0], q1 = -p[1], q2 = p[2];
            r0 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.rot[0], q0), __dmul_rn(a.rot[1], q1)), __dmul_rn(a.rot[2], q2)), a.t[0]);
            r1 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.rot[3], q0), __dmul_rn(a.rot[4], q1)), __dmul_rn(a.rot[5], q2)), a.t[1]);
            r2 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.rot[6], q0), __dmul_rn(a.rot[7], q1)), __dmul_rn(a.rot[8], q2)), a.t[2]);
            if (!(__builtin_fabs(z) < __builtin_inf())) r0 = r1 = r2 = __builtin_nan("");     // z = +-inf or NaN: numpy's inf * 0
            if (a.valid) a.valid[row + x] = z_valid(z) ? 1 : 0;
        }
        if (a.out64) {
            s64[3 * threadIdx.x] = r0; s64[3 * threadIdx.x + 1] = r1; s64[3 * threadIdx.x + 2] = r2;
            __syncthreads();
            store_span<double>(a.out64, (row + x0) * 3, n * 3, s64);
            __syncthreads();
        }
        if (a.out32) {
            s32[3 * threadIdx.x] = (float)r0; s32[3 * threadIdx.x + 1] = (float)r1; s32[3 * threadIdx.x + 2] = (float)r2;     // one rounding to nearest
            __syncthreads();
            store_span<float>(a.out32, (row + x0) * 3, n * 3, s32);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------ triangles
struct TriArgs {
    const uint8_t* mask;     // or NULL: every vertex inside
    long mask_pitch, mask_stride;
    const float* depth;      // [batch][h][w] or NULL
    ZRule z;
    double max_ratio;        // <= 0: off
    int h, w;
    uint32_t ncells;         // (h - 1) (w - 1)
    int32_t* sums;           // [batch][nblk]
    int nblk;
    int32_t* tri;            // [batch][capacity][3]
    int capacity;
};

// THE predicate: bit 0 = (tl, bl, tr) kept, bit 1 = (br, tr, bl) kept, for the cell whose top-left vertex is (cy, cx) of image b
ADA_DEV int tri_flags(const TriArgs& a, int b, int cy, int cx) {
    bool in[4] = {true, true, true, true};     // tl, tr, bl, br
    double z[4] = {1.0, 1.0, 1.0, 1.0};
    if (a.mask) {
        const uint8_t* m = a.mask + (long)b * a.mask_stride + (long)cy * a.mask_pitch + cx;
        in[0] = m[0] != 0; in[1] = m[1] != 0; in[2] = m[a.mask_pitch] != 0; in[3] = m[a.mask_pitch + 1] != 0;
    }
    if (a.depth) {
        const float* d = a.depth + ((long)b * a.h + cy) * a.w + cx;
        z[0] = z_of(a.z, d[0]); z[1] = z_of(a.z, d[1]); z[2] = z_of(a.z, d[a.w]); z[3] = z_of(a.z, d[a.w + 1]);
#pragma unroll
        for (int i = 0; i < 4; ++i) in[i] = in[i] && z_valid(z[i]);
    }
    bool k0 = in[0] && in[2] && in[1], k1 = in[3] && in[1] && in[2];
    if (a.depth && a.max_ratio > 0.0) {
        const double lo12 = fmin(z[1], z[2]), hi12 = fmax(z[1], z[2]);
        k0 = k0 && fmax(hi12, z[0]) <= __dmul_rn(a.max_ratio, fmin(lo12, z[0]));
        k1 = k1 && fmax(hi12, z[3]) <= __dmul_rn(a.max_ratio, fmin(lo12, z[3]));
    }
    return (k0 ? 1 : 0) | (k1 ? 2 : 0);
}

template <bool SCATTER>
__global__ __launch_bounds__(GEOM_THREADS) void tri_kernel(TriArgs a, FastDiv cells_per_row) {
    __shared__ int lds[GEOM_WAVES];
    const int b = blockIdx.y;
    const uint32_t c0 = blockIdx.x * (uint32_t)GEOM_CHUNK;
    long pos = SCATTER ? (long)a.sums[(long)b * a.nblk + blockIdx.x] : 0;     // triangles of this image before the workgroup's (then: before the round's)
    int mine = 0;
    int32_t* out = a.tri + (long)b * a.capacity * 3;
#pragma unroll
    for (int j = 0; j < GEOM_SUB; ++j) {
        const uint32_t c = c0 + j * GEOM_THREADS + threadIdx.x;
        int f = 0;
        uint32_t cy = 0, cx = 0;
        if (c < a.ncells) {
            if (a.ncells < (1u << 24)) fast_divmod(c, cells_per_row, cy, cx);      // the float reciprocal is exact below 2^24
            else { cy = c / cells_per_row.d; cx = c - cy * cells_per_row.d; }
            f = tri_flags(a, b, (int)cy, (int)cx);
        }
        if (!SCATTER) {
            mine += __popc(f);
        } else {
            const uint64_t b0 = __ballot(f & 1), b1 = __ballot(f & 2);
            // candidates in order: lane 0's first, lane 0's second, lane 1's first, ...
            const int below = lanes_below(b0) + lanes_below(b1);
            int round_total;
            const int before = waves_before<GEOM_WAVES>(lds, __popcll(b0) + __popcll(b1), round_total);
            long p = pos + before + below;
            const int tl = (int)cy * a.w + (int)cx, tr = tl + 1, bl = tl + a.w, br = bl + 1;
            if ((f & 1) && p < a.capacity) { out[3 * p] = tl; out[3 * p + 1] = bl; out[3 * p + 2] = tr; }
            p += f & 1;
            if ((f & 2) && p < a.capacity) { out[3 * p] = br; out[3 * p + 1] = tr; out[3 * p + 2] = bl; }
            pos += round_total;
        }
    }
    if (!SCATTER) {
        int total;
        waves_before<GEOM_WAVES>(lds, wave_total(mine), total);
        if (threadIdx.x == 0) a.sums[(long)b * a.nblk + blockIdx.x] = total;
    }
}

// ------------------------------------------------------------------ vertex compaction
struct CompactArgs {
    int32_t* tri;            // [batch][capacity][3], rewritten in place
    const int32_t* count;    // [batch]
    int capacity;
    int hw;                  // vertices per image
    int32_t* index;          // [batch][hw]: 0 / 1 marks, then the new index or -1
    int32_t* sums;           // [batch][nblk]
    int nblk;
    const void* points;      // [batch][hw][3]
    void* points_out;        // [batch][vertex_capacity][3]
    const uint8_t* colors;   // [batch][hw][3] or NULL
    uint8_t* colors_out;     // [batch][vertex_capacity][3] or NULL
    int vertex_capacity;
};

__global__ __launch_bounds__(GEOM_THREADS) void clear_kernel(int32_t* p, int n) {
    const long i = (long)blockIdx.x * GEOM_THREADS + threadIdx.x;
    if (i < n) p[(long)blockIdx.y * n + i] = 0;
}

// one thread per index of the triangle list; MARK: index[v] = 1, else v <- index[v]
template <bool MARK>
__global__ __launch_bounds__(GEOM_THREADS) void tri_index_kernel(CompactArgs a) {
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * GEOM_THREADS + threadIdx.x;
    const long n = 3l * min(max(a.count[b], 0), a.capacity);
    if (i >= n) return;
    int32_t* t = a.tri + (long)b * a.capacity * 3 + i;
    const int v = *t;
    if ((uint32_t)v >= (uint32_t)a.hw) return;      // not an index of this grid: left alone, never dereferenced
    int32_t* idx = a.index + (long)b * a.hw + v;
    if (MARK) *idx = 1;
    else *t = *idx;
}

template <bool GATHER, typename T>
__global__ __launch_bounds__(GEOM_THREADS) void vertex_kernel(CompactArgs a) {
    __shared__ int lds[GEOM_WAVES];
    const int b = blockIdx.y;
    const long v0 = (long)blockIdx.x * GEOM_CHUNK;
    int32_t* index = a.index + (long)b * a.hw;
    long pos = GATHER ? (long)a.sums[(long)b * a.nblk + blockIdx.x] : 0;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < GEOM_SUB; ++j) {
        const long v = v0 + j * GEOM_THREADS + threadIdx.x;
        const bool m = v < a.hw && index[v] != 0;
        if (!GATHER) {
            mine += m;
        } else {
            int round_total;
            const long p = pos + block_excl_flag<GEOM_WAVES>(m, lds, round_total);
            if (v < a.hw) index[v] = m ? (int32_t)p : -1;
            if (m && p < a.vertex_capacity) {
                const T* src = (const T*)a.points + ((long)b * a.hw + v) * 3;
                T* dst = (T*)a.points_out + ((long)b * a.vertex_capacity + p) * 3;
                dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
                if (a.colors) {
                    const uint8_t* cs = a.colors + ((long)b * a.hw + v) * 3;
                    uint8_t* cd = a.colors_out + ((long)b * a.vertex_capacity + p) * 3;
                    cd[0] = cs[0]; cd[1] = cs[1]; cd[2] = cs[2];
                }
            }
            pos += round_total;
        }
    }
    if (!GATHER) {
        int total;
        waves_before<GEOM_WAVES>(lds, wave_total(mine), total);
        if (threadIdx.x == 0) a.sums[(long)b * a.nblk + blockIdx.x] = total;
    }
}

bool geom_shape_ok(int32_t batch, int32_t h, int32_t w) {
    return batch >= 1 && batch <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 30);
}

}  // namespace

extern "C" int ada_depth_points_fwd(const float* depth, int32_t batch, int32_t h, int32_t w, const double* camera, int32_t inverse, double a,
                                    double b, double* out_f64, float* out_f32, uint8_t* valid, void* stream) {
    ADA_REQUIRE(depth && camera && (out_f64 || out_f32), ADA_EINVAL, "ada_depth_points_fwd: null pointer (depth, camera and one output are needed)");
    ADA_REQUIRE(geom_shape_ok(batch, h, w), ADA_EINVAL, "ada_depth_points_fwd: batch=%d h=%d w=%d outside 1..65535 / h * w < 2^30", batch, h, w);
    ADA_REQUIRE(inverse == 0 || inverse == 1, ADA_EINVAL, "ada_depth_points_fwd: inverse=%d (0 or 1)", inverse);
    ADA_REQUIRE((uintptr_t)out_f64 % 16 == 0 && (uintptr_t)out_f32 % 16 == 0, ADA_EINVAL, "ada_depth_points_fwd: the outputs must be 16-byte aligned");
    PointArgs p;
    p.depth = depth; p.out64 = out_f64; p.out32 = out_f32; p.valid = valid; p.h = h; p.w = w;
    p.z.inverse = inverse; p.z.a = a; p.z.b = b;
    for (int i = 0; i < 9; ++i) { p.kinv[i] = camera[i]; p.rot[i] = camera[9 + i]; }     // host pointer, taken by value here
    for (int i = 0; i < 3; ++i) p.t[i] = camera[18 + i];
    const dim3 grid((unsigned)((w + GEOM_THREADS - 1) / GEOM_THREADS), (unsigned)(h < 65535 ? h : 65535), (unsigned)batch);
    hipLaunchKernelGGL(points_kernel, grid, dim3(GEOM_THREADS), 0, (hipStream_t)stream, p);
    return ada_check_launch("ada_depth_points_fwd");
}

extern "C" int ada_mesh_triangles_fwd(const uint8_t* mask, int64_t row_pitch_bytes, int64_t image_stride_bytes, const float* depth, int32_t inverse,
                                      double a, double b, double max_ratio, int32_t batch, int32_t h, int32_t w, int32_t* triangles,
                                      int32_t capacity, int32_t* count, void* workspace, int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(count && workspace && (triangles || capacity == 0), ADA_EINVAL, "ada_mesh_triangles_fwd: null pointer");
    ADA_REQUIRE(geom_shape_ok(batch, h, w), ADA_EINVAL, "ada_mesh_triangles_fwd: batch=%d h=%d w=%d outside 1..65535 / h * w < 2^30", batch, h, w);
    const int rc = mesh_rule_check("ada_mesh_triangles_fwd", mask, row_pitch_bytes, image_stride_bytes, inverse, max_ratio, batch, h, w, capacity);
    if (rc != ADA_OK) return rc;
    ADA_REQUIRE(!(max_ratio > 0.0) || depth, ADA_EINVAL, "ada_mesh_triangles_fwd: max_ratio needs the depth map");      // a NaN ratio never gets here
    const int64_t ncells = (int64_t)(h - 1) * (w - 1);
    const int64_t nblk = (ncells + GEOM_CHUNK - 1) / GEOM_CHUNK;
    const int64_t need = 4 * (int64_t)batch * (nblk > 0 ? nblk : 1);
    ADA_REQUIRE(workspace_bytes >= need && (uintptr_t)workspace % 4 == 0, ADA_EINVAL, "ada_mesh_triangles_fwd: workspace of %ld bytes needed, got %ld",
                (long)need, (long)workspace_bytes);
    const hipStream_t s = (hipStream_t)stream;
    TriArgs t;
    t.mask = mask; t.mask_pitch = (long)row_pitch_bytes; t.mask_stride = (long)image_stride_bytes; t.depth = depth;
    t.z.inverse = inverse; t.z.a = a; t.z.b = b; t.max_ratio = max_ratio; t.h = h; t.w = w; t.ncells = (uint32_t)ncells;
    t.sums = (int32_t*)workspace; t.nblk = (int)nblk; t.tri = triangles; t.capacity = capacity;
    const FastDiv per_row = make_fastdiv((uint32_t)(w - 1));
    const dim3 grid((unsigned)nblk, (unsigned)batch);
    if (nblk > 0) hipLaunchKernelGGL(tri_kernel<false>, grid, dim3(GEOM_THREADS), 0, s, t, per_row);
    hipLaunchKernelGGL(scan_sums_kernel<1>, dim3((unsigned)batch), dim3(SCAN_THREADS), 0, s, t.sums, (long)nblk, (long)nblk, count);
    if (nblk > 0 && capacity > 0) hipLaunchKernelGGL(tri_kernel<true>, grid, dim3(GEOM_THREADS), 0, s, t, per_row);
    return ada_check_launch("ada_mesh_triangles_fwd");
}

extern "C" int ada_mesh_compact_fwd(int32_t* triangles, const int32_t* count, int32_t capacity, int32_t batch, int32_t h, int32_t w,
                                    const void* points, int32_t point_bytes, const uint8_t* colors, void* points_out, uint8_t* colors_out,
                                    int32_t vertex_capacity, int32_t* vertex_count, void* workspace, int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(count && points && vertex_count && workspace && (triangles || capacity == 0) && (points_out || vertex_capacity == 0), ADA_EINVAL,
                "ada_mesh_compact_fwd: null pointer");
    ADA_REQUIRE(!colors == !colors_out || vertex_capacity == 0, ADA_EINVAL, "ada_mesh_compact_fwd: colors and colors_out come together");
    ADA_REQUIRE(geom_shape_ok(batch, h, w), ADA_EINVAL, "ada_mesh_compact_fwd: batch=%d h=%d w=%d outside 1..65535 / h * w < 2^30", batch, h, w);
    ADA_REQUIRE(capacity >= 0 && vertex_capacity >= 0 && (int64_t)batch * capacity * 3 < ((int64_t)1 << 40), ADA_EINVAL,
                "ada_mesh_compact_fwd: capacity=%d vertex_capacity=%d", capacity, vertex_capacity);
    ADA_REQUIRE(point_bytes == 4 || point_bytes == 8, ADA_EINVAL, "ada_mesh_compact_fwd: point_bytes=%d (4: fp32, 8: fp64)", point_bytes);
    const int64_t hw = (int64_t)h * w;
    const int64_t nblk = (hw + GEOM_CHUNK - 1) / GEOM_CHUNK;
    const int64_t need = 4 * (int64_t)batch * (hw + nblk);
    ADA_REQUIRE(workspace_bytes >= need && (uintptr_t)workspace % 4 == 0, ADA_EINVAL, "ada_mesh_compact_fwd: workspace of %ld bytes needed, got %ld",
                (long)need, (long)workspace_bytes);
    const hipStream_t s = (hipStream_t)stream;
    CompactArgs c;
    c.tri = triangles; c.count = count; c.capacity = capacity; c.hw = (int)hw;
    c.index = (int32_t*)workspace; c.sums = c.index + (int64_t)batch * hw; c.nblk = (int)nblk;
    c.points = points; c.points_out = points_out; c.colors = colors_out ? colors : nullptr; c.colors_out = colors_out; c.vertex_capacity = vertex_capacity;
    hipLaunchKernelGGL(clear_kernel, dim3((unsigned)((hw + GEOM_THREADS - 1) / GEOM_THREADS), (unsigned)batch), dim3(GEOM_THREADS), 0, s, c.index, (int)hw);
    const dim3 tgrid((unsigned)((3l * capacity + GEOM_THREADS - 1) / GEOM_THREADS), (unsigned)batch);
    const dim3 vgrid((unsigned)nblk, (unsigned)batch);
    if (capacity > 0) hipLaunchKernelGGL(tri_index_kernel<true>, tgrid, dim3(GEOM_THREADS), 0, s, c);
    hipLaunchKernelGGL((vertex_kernel<false, float>), vgrid, dim3(GEOM_THREADS), 0, s, c);
    hipLaunchKernelGGL(scan_sums_kernel<1>, dim3((unsigned)batch), dim3(SCAN_THREADS), 0, s, c.sums, (long)nblk, (long)nblk, vertex_count);
    if (point_bytes == 8) hipLaunchKernelGGL((vertex_kernel<true, double>), vgrid, dim3(GEOM_THREADS), 0, s, c);
    else hipLaunchKernelGGL((vertex_kernel<true, float>), vgrid, dim3(GEOM_THREADS), 0, s, c);
    if (capacity > 0) hipLaunchKernelGGL(tri_index_kernel<false>, tgrid, dim3(GEOM_THREADS), 0, s, c);
    return ada_check_launch("ada_mesh_compact_fwd");
}
