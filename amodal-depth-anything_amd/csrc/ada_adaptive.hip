// Adaptive depth-map meshes on the device: an error-bounded right-triangulated irregular network (RTIN: the binary tree of right isosceles triangles of
// Lindstrom's and "martini"-style terrain meshes) over a depth map, in place of the two triangles per pixel cell of ada_geometry.hip.  The contract --
// grid, tree, heap index, disparity, keepable leaf, error map, emission, order -- is include/ada_hip.h's; tests/_adaptive_ref.py restates it in numpy.
//
// Error phase.  Every vertex but the corners of the virtual grid is the hypotenuse midpoint of the up to two triangles of exactly ONE level, so the
// bottom-up pass is a gather per midpoint: E[m] = max over those triangles of F(T), each F from the (final) E of the level below.  No atomic, each E
// is stored once, and where which corner is a, b or c follows from the coordinates alone: at an odd level the hypotenuse is an edge of the level's
// cell grid and the right angles sit at the two cell centres beside it; at an even level it is a cell's diagonal (the main one when the cell's row and
// column indices have an even sum) and the right angles are the other two corners.  One launch per level while a level holds more than
// ADA_ADAPT_FOLD midpoints inside the image; the coarser levels run in one workgroup, a barrier between them.
//
// Emission phase.  A predicate per triangle (emit(), ONE function used by the counting and the writing pass) and an order-preserving compaction by heap
// index.  The tree is cut at the level whose cells are ADA_ADAPT_CELL wide: above it one workgroup walks the levels breadth first, keeping only
// triangles whose bounding box overlaps the image -- the lists stay in heap order and their sizes depend on the shapes alone; at the cut these are
// the two halves of every cell that overlaps the image, 2 ceil((h - 1) / cell) ceil((w - 1) / cell) subtrees.  Below it one workgroup per subtree
// decodes its triangles from the path bits.  Counts per (level, subtree) in heap order, one scan (scan_sums_kernel<8> of ada_scan.h, whose block
// prefixes also place the rows), then the subtrees' walk again writes the rows (the levels above the cut come first in heap order: their workgroup
// writes its rows while it counts).  The depth -> z rule of a keepable leaf is ada_mesh_rule.h's, shared with ada_geometry.hip.
// No subtree wholly outside the image is launched over or descended into, no atomic decides a position: the same bytes every run.
//
// Every launch sequence is fixed by the shapes and the flags; nothing is read back and nothing allocated: legal inside a stream capture.
#include "ada_mesh_rule.h"
#include "ada_scan.h"

namespace {

constexpr int AD_WAVE = ADA_WAVE;
constexpr int AD_THREADS = 256;                      // the per-level error launches and the per-subtree walks
constexpr int AD_TOP = 1024;                         // the one workgroup of the folded levels and of the breadth-first walk
constexpr int AD_SCAN_ITEMS = 8;                     // sums per thread and step of the scan: the 6 400 sums of a 518 x 518 map take one step
constexpr int AD_FOLD = ADA_ADAPT_FOLD;
constexpr int AD_CELL = ADA_ADAPT_CELL;
constexpr int AD_MAX_N = ADA_ADAPT_MAX_N;
static_assert(AD_TOP == 1024 && AD_FOLD <= AD_TOP && (AD_CELL & (AD_CELL - 1)) == 0, "layout");

struct Node {                // a triangle of the tree: heap index and its corners (row, column), right angle at c
    int t, ai, aj, bi, bj, ci, cj, pad;
};

struct AdArgs {
    const uint8_t* mask;     // or NULL: every vertex inside
    long mask_pitch;
    const float* depth;      // [h][w]
    ZRule z;                 // and omega = 1 / z: omega_of
    double max_ratio;        // <= 0: off
    int h, w, N, levels;     // levels = 2 log2 N + 1
    double* E;               // [h][w]
    double tau;
    int none;                // 1: every keepable leaf
    int32_t* tri;            // [capacity][3]
    int capacity;
    int lb, n_sub;           // the level of the subtree roots and their number
    Node* list0;
    Node* list1;
    int list_cap;
    int32_t* sums;           // [lb] then [levels - lb][n_sub]
};

ADA_DEV double d_inf() { return __builtin_inf(); }

ADA_DEV double omega_of(const AdArgs& p, int i, int j) {
    const double v = (double)p.depth[i * p.w + j];
    if (!p.z.inverse) return 1.0 / v;
    return __dadd_rn(__dmul_rn(p.z.a, v), p.z.b);
}

// present, inside the mask and valid: the three per-vertex tests of create_triangles; z is set when it returns true
ADA_DEV bool vertex_ok(const AdArgs& p, int i, int j, double& z) {
    if ((unsigned)i >= (unsigned)p.h || (unsigned)j >= (unsigned)p.w) return false;
    if (p.mask && p.mask[(long)i * p.mask_pitch + j] == 0) return false;
    z = z_of(p.z, p.depth[i * p.w + j]);
    return z_valid(z);
}

ADA_DEV bool keepable(const AdArgs& p, int i0, int j0, int i1, int j1, int i2, int j2) {
    double z0 = 1.0, z1 = 1.0, z2 = 1.0;
    if (!vertex_ok(p, i0, j0, z0) || !vertex_ok(p, i1, j1, z1) || !vertex_ok(p, i2, j2, z2)) return false;
    if (p.max_ratio > 0.0) return fmax(fmax(z0, z1), z2) <= __dmul_rn(p.max_ratio, fmin(fmin(z0, z1), z2));
    return true;
}

// E of a vertex of the virtual grid: +inf where the vertex is absent (every triangle that touches it holds an unkeepable leaf)
ADA_DEV double e_at(const AdArgs& p, int i, int j) {
    return ((unsigned)i < (unsigned)p.h && (unsigned)j < (unsigned)p.w) ? p.E[i * p.w + j] : d_inf();
}

// the midpoints of level l inside the image as a rows x cols lattice (a few of the last column's may fall outside: err_vertex checks)
__host__ __device__ inline void level_dims(int h, int w, int N, int l, int& half, int& rows, int& cols) {
    half = (N >> (l >> 1)) >> 1;
    const int U = (h - 1) / half, V = (w - 1) / half;
    if (l & 1) { rows = U + 1; cols = V / 2 + 1; }
    else { rows = (U + 1) / 2; cols = (V + 1) / 2; }
}

// E of one midpoint of level l: lattice position (ru, q)
ADA_DEV void err_vertex(const AdArgs& p, int l, int half, int ru, int q) {
    const bool odd = l & 1;
    const int u = odd ? ru : 2 * ru + 1;
    const int v = odd ? 2 * q + ((u + 1) & 1) : 2 * q + 1;
    const int i = u * half, j = v * half;
    if (i >= p.h || j >= p.w) return;
    int ai, aj, bi, bj, ci, cj, di, dj;      // hypotenuse a b, right angles c and d
    if (odd) {
        if (v & 1) { ai = i; aj = j - half; bi = i; bj = j + half; ci = i - half; cj = j; di = i + half; dj = j; }
        else { ai = i - half; aj = j; bi = i + half; bj = j; ci = i; cj = j - half; di = i; dj = j + half; }
    } else {
        const bool main_diag = ((((u - 1) >> 1) + ((v - 1) >> 1)) & 1) == 0;
        if (main_diag) { ai = i - half; aj = j - half; bi = i + half; bj = j + half; ci = i + half; cj = j - half; di = i - half; dj = j + half; }
        else { ai = i + half; aj = j - half; bi = i - half; bj = j + half; ci = i - half; cj = j - half; di = i + half; dj = j + half; }
    }
    const bool tc = ci >= 0 && cj >= 0 && ci <= p.N && cj <= p.N;      // the triangle on that side exists (the midpoint may lie on the grid's border)
    const bool td = di >= 0 && dj >= 0 && di <= p.N && dj <= p.N;
    double e = 0.0;
    if (l == p.levels - 2) {      // the children are leaves
        bool ok = true;
        if (tc) ok = ok && keepable(p, ci, cj, ai, aj, i, j) && keepable(p, bi, bj, ci, cj, i, j);
        if (td) ok = ok && keepable(p, di, dj, ai, aj, i, j) && keepable(p, bi, bj, di, dj, i, j);
        e = ok ? 0.0 : d_inf();
    } else {
        if (tc) e = fmax(e, fmax(e_at(p, (ci + ai) >> 1, (cj + aj) >> 1), e_at(p, (bi + ci) >> 1, (bj + cj) >> 1)));
        if (td) e = fmax(e, fmax(e_at(p, (di + ai) >> 1, (dj + aj) >> 1), e_at(p, (bi + di) >> 1, (bj + dj) >> 1)));
    }
    if (max(ai, bi) >= p.h || max(aj, bj) >= p.w) e = d_inf();      // an absent end of the hypotenuse (the level below says so too: never read past the map)
    if (e < d_inf()) {      // every leaf below is keepable: a, b and m are valid vertices, omega_m is finite and positive
        const double wa = omega_of(p, ai, aj), wb = omega_of(p, bi, bj), wm = omega_of(p, i, j);
        const double dev = __builtin_fabs(__dsub_rn(__dmul_rn(0.5, __dadd_rn(wa, wb)), wm)) / wm;
        e = fmax(e, dev);
    }
    p.E[i * p.w + j] = e;
}

__global__ __launch_bounds__(AD_THREADS) void err_level_kernel(AdArgs p, int l, int half, int cols) {
    const int q = blockIdx.x * AD_THREADS + threadIdx.x;
    if (q < cols) err_vertex(p, l, half, (int)blockIdx.y, q);
}

// levels l_start .. 0 in one workgroup, and the corners of the virtual grid (the midpoint of no triangle): E = 0
__global__ __launch_bounds__(AD_TOP) void err_fold_kernel(AdArgs p, int l_start) {
    if (threadIdx.x == 0) {
        p.E[0] = 0.0;
        if (p.w - 1 == p.N) p.E[p.N] = 0.0;
        if (p.h - 1 == p.N) p.E[p.N * p.w] = 0.0;
        if (p.w - 1 == p.N && p.h - 1 == p.N) p.E[p.N * p.w + p.N] = 0.0;
    }
    for (int l = l_start; l >= 0; --l) {
        int half, rows, cols;
        level_dims(p.h, p.w, p.N, l, half, rows, cols);
        const int n = rows * cols;
        for (int idx = threadIdx.x; idx < n; idx += AD_TOP) {
            const int ru = idx / cols;
            err_vertex(p, l, half, ru, idx - ru * cols);
        }
        __syncthreads();      // the level's E is visible to the workgroup before the next level gathers it
    }
}

// ------------------------------------------------------------------ emission
// THE predicate: is the triangle (a, b, c) of level l a row of the output
ADA_DEV bool emit(const AdArgs& p, int l, int ai, int aj, int bi, int bj, int ci, int cj) {
    // c is the parent's hypotenuse midpoint: the parent was split when E[c] > tau (an absent c: +inf)
    const bool split = l == 0 || p.none || e_at(p, ci, cj) > p.tau;
    if (!split) return false;
    if (l == p.levels - 1) return keepable(p, ai, aj, bi, bj, ci, cj);
    if (p.none) return false;
    return e_at(p, (ai + bi) >> 1, (aj + bj) >> 1) <= p.tau;
}

ADA_DEV void write_row(const AdArgs& p, long pos, int ai, int aj, int bi, int bj, int ci, int cj) {
    if (pos < p.capacity) {
        int32_t* o = p.tri + 3 * pos;
        o[0] = ai * p.w + aj; o[1] = bi * p.w + bj; o[2] = ci * p.w + cj;
    }
}

ADA_DEV bool overlaps(const AdArgs& p, int ai, int aj, int bi, int bj, int ci, int cj) {      // the bounding box and the image share area
    return min(min(ai, bi), ci) < p.h - 1 && min(min(aj, bj), cj) < p.w - 1;
}

// levels 0 .. lb - 1 breadth first in one workgroup; leaves the subtree roots (level lb) in list0, in heap order.  These levels come first in heap
// order, so a level's first row is the number of rows of the levels above it, which this workgroup has just counted: it counts (sums[l], for the scan
// that places the subtrees' rows) and writes its own rows in the same walk.  One scan per step carries both the children kept and the rows.
__global__ __launch_bounds__(AD_TOP) void top_kernel(AdArgs p) {
    __shared__ int lds[AD_TOP / AD_WAVE];
    Node* cur = p.list0;
    Node* nxt = p.list1;
    if (threadIdx.x < 2) {
        Node r;
        r.t = 2 + threadIdx.x; r.pad = 0;
        if (threadIdx.x == 0) { r.ai = p.N; r.aj = p.N; r.bi = 0; r.bj = 0; r.ci = p.N; r.cj = 0; }
        else { r.ai = 0; r.aj = 0; r.bi = p.N; r.bj = p.N; r.ci = 0; r.cj = p.N; }
        cur[threadIdx.x] = r;
    }
    __syncthreads();
    int n_cur = 2;
    long out0 = 0;      // rows of the levels above
    for (int l = 0; l < p.lb; ++l) {
        int emitted = 0, n_next = 0;
        for (int base = 0; base < n_cur; base += AD_TOP) {
            const int i = base + threadIdx.x;
            const bool have = i < n_cur;
            Node n = {0, 0, 0, 0, 0, 0, 0, 0};
            if (have) n = cur[i];
            const int mi = (n.ai + n.bi) >> 1, mj = (n.aj + n.bj) >> 1;
            const bool e = have && emit(p, l, n.ai, n.aj, n.bi, n.bj, n.ci, n.cj);
            const bool f0 = have && overlaps(p, n.ci, n.cj, n.ai, n.aj, mi, mj);      // left child (c, a, m)
            const bool f1 = have && overlaps(p, n.bi, n.bj, n.ci, n.cj, mi, mj);      // right child (b, c, m)
            // children in the low 16 bits (at most 2 AD_TOP a step), rows above them (at most AD_TOP)
            int total;
            const int before = block_excl<AD_TOP / AD_WAVE>((f0 ? 1 : 0) + (f1 ? 1 : 0) + (e ? 1 << 16 : 0), lds, total);
            int pos = n_next + (before & 0xFFFF);
            if (f0 && pos < p.list_cap) { Node c = {2 * n.t, n.ci, n.cj, n.ai, n.aj, mi, mj, 0}; nxt[pos] = c; }
            pos += f0 ? 1 : 0;
            if (f1 && pos < p.list_cap) { Node c = {2 * n.t + 1, n.bi, n.bj, n.ci, n.cj, mi, mj, 0}; nxt[pos] = c; }
            if (e) write_row(p, out0 + emitted + (before >> 16), n.ai, n.aj, n.bi, n.bj, n.ci, n.cj);
            n_next += total & 0xFFFF;
            emitted += total >> 16;
        }
        if (threadIdx.x == 0) p.sums[l] = emitted;
        out0 += emitted;
        Node* s = cur; cur = nxt; nxt = s;
        n_cur = min(n_next, p.list_cap);
        __syncthreads();      // the next level's list is complete
    }
}

// one workgroup per subtree root: sublevel d holds 2^d triangles, heap index (root << d) + q, decoded from q's bits.  E is monotone along the tree,
// so a root whose parent was not split (E[c] <= tau) has no row at all below it, and one that is not split itself (E[m] <= tau) none below level 0:
// over smooth ground most workgroups end here.  The counting pass needs no order: a ballot per wave and one LDS add per level.
template <bool SCATTER>
__global__ __launch_bounds__(AD_THREADS) void sub_kernel(AdArgs p) {
    __shared__ int lds[32];      // SCATTER: the waves' totals; counting: a counter per sublevel (at most 2 log2 ADA_ADAPT_CELL + 1)
    const int r = blockIdx.x;
    const Node root = p.list0[r];
    const int depth = p.levels - 1 - p.lb;
    int last = depth;
    bool nothing = false;
    if (!p.none) {
        if (p.lb > 0 && !(e_at(p, root.ci, root.cj) > p.tau)) nothing = true;
        else if (depth > 0 && e_at(p, (root.ai + root.bi) >> 1, (root.aj + root.bj) >> 1) <= p.tau) last = 0;
    }
    if (!SCATTER) {
        if (threadIdx.x < 32) lds[threadIdx.x] = 0;
        __syncthreads();
    }
    for (int d = 0; d <= last && !nothing; ++d) {
        const int l = p.lb + d;
        const long out0 = SCATTER ? (long)p.sums[(long)p.lb + (long)d * p.n_sub + r] : 0;
        const int cnt = 1 << d;
        int emitted = 0;
        for (int base = 0; base < cnt; base += AD_THREADS) {
            const int q = base + threadIdx.x;
            const bool have = q < cnt;
            int ai = root.ai, aj = root.aj, bi = root.bi, bj = root.bj, ci = root.ci, cj = root.cj;
            for (int bit = d - 1; bit >= 0; --bit) {
                const int mi = (ai + bi) >> 1, mj = (aj + bj) >> 1;
                if ((q >> bit) & 1) { const int ti = bi, tj = bj; bi = ci; bj = cj; ai = ti; aj = tj; }      // right child (b, c, m)
                else { const int ti = ai, tj = aj; ai = ci; aj = cj; bi = ti; bj = tj; }                      // left child (c, a, m)
                ci = mi; cj = mj;
            }
            const bool e = have && emit(p, l, ai, aj, bi, bj, ci, cj);
            if (SCATTER) {
                int total_e;
                const int pe = block_excl_flag<AD_THREADS / AD_WAVE>(e, lds, total_e);
                if (e) write_row(p, out0 + emitted + pe, ai, aj, bi, bj, ci, cj);
                emitted += total_e;
            } else {
                const uint64_t bal = __ballot(e);
                if ((threadIdx.x & (AD_WAVE - 1)) == 0 && bal) atomicAdd(&lds[d], __popcll(bal));      // an integer sum: the order cannot show
            }
        }
    }
    if (!SCATTER) {
        __syncthreads();
        if ((int)threadIdx.x <= depth) p.sums[(long)p.lb + (long)threadIdx.x * p.n_sub + r] = lds[threadIdx.x];
    }
}

struct Plan {
    int N, logN, levels, cell, lb, n_sub, list_cap;
    int64_t n_sums, off_list0, off_list1, off_sums, bytes;
};

int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }

Plan make_plan(int h, int w) {
    Plan q;
    q.N = 1; q.logN = 0;
    const int span = (h > w ? h : w) - 1;
    while (q.N < span) { q.N <<= 1; ++q.logN; }
    q.levels = 2 * q.logN + 1;
    q.cell = q.N < AD_CELL ? q.N : AD_CELL;
    int logc = 0;
    while ((1 << logc) < q.cell) ++logc;
    q.lb = 2 * (q.logN - logc);
    q.n_sub = 2 * ((h - 1 + q.cell - 1) / q.cell) * ((w - 1 + q.cell - 1) / q.cell);
    q.list_cap = 2 * q.n_sub;      // an odd level above the cut holds at most twice the triangles of the even level above it, that at most n_sub
    q.n_sums = (int64_t)q.lb + (int64_t)(q.levels - q.lb) * q.n_sub;
    q.off_list0 = up16(8 * (int64_t)h * w);
    q.off_list1 = q.off_list0 + (int64_t)sizeof(Node) * q.list_cap;
    q.off_sums = q.off_list1 + (int64_t)sizeof(Node) * q.list_cap;
    q.bytes = q.off_sums + up16(4 * q.n_sums);
    return q;
}

bool adapt_shape_ok(int32_t h, int32_t w) { return h >= 2 && w >= 2 && (int64_t)h * w < ((int64_t)1 << 30); }

}  // namespace

extern "C" int ada_mesh_adaptive_workspace_bytes(int32_t h, int32_t w, int64_t* bytes) {
    ADA_REQUIRE(bytes, ADA_EINVAL, "ada_mesh_adaptive_workspace_bytes: null pointer");
    ADA_REQUIRE(adapt_shape_ok(h, w), ADA_EINVAL, "ada_mesh_adaptive_workspace_bytes: h=%d w=%d outside h, w >= 2 / h * w < 2^30", h, w);
    ADA_REQUIRE((h > w ? h : w) - 1 <= AD_MAX_N, ADA_EUNSUPPORTED, "ada_mesh_adaptive_workspace_bytes: h=%d w=%d beyond %d + 1 on a side", h, w, AD_MAX_N);
    *bytes = make_plan(h, w).bytes;
    return ADA_OK;
}

extern "C" int ada_mesh_adaptive_fwd(const uint8_t* mask, int64_t row_pitch_bytes, int64_t image_stride_bytes, const float* depth, int32_t inverse,
                                     double a, double b, double max_ratio, double max_error, int32_t no_max_error, int32_t batch, int32_t h, int32_t w,
                                     int32_t* triangles, int32_t capacity, int32_t* count, double* error_out, int32_t error_ready, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(depth && count && workspace && (triangles || capacity == 0), ADA_EINVAL, "ada_mesh_adaptive_fwd: null pointer");
    ADA_REQUIRE(batch >= 1 && batch <= 65535 && adapt_shape_ok(h, w), ADA_EINVAL,
                "ada_mesh_adaptive_fwd: batch=%d h=%d w=%d outside 1..65535 / h, w >= 2 / h * w < 2^30", batch, h, w);
    ADA_REQUIRE((h > w ? h : w) - 1 <= AD_MAX_N, ADA_EUNSUPPORTED, "ada_mesh_adaptive_fwd: h=%d w=%d beyond %d + 1 on a side", h, w, AD_MAX_N);
    const int rc = mesh_rule_check("ada_mesh_adaptive_fwd", mask, row_pitch_bytes, image_stride_bytes, inverse, max_ratio, batch, h, w, capacity);
    if (rc != ADA_OK) return rc;
    ADA_REQUIRE(no_max_error == 0 || no_max_error == 1, ADA_EINVAL, "ada_mesh_adaptive_fwd: no_max_error=%d (0 or 1)", no_max_error);
    ADA_REQUIRE(no_max_error || (max_error >= 0.0 && max_error < __builtin_inf()), ADA_EINVAL,
                "ada_mesh_adaptive_fwd: max_error=%g must be finite and >= 0", max_error);
    ADA_REQUIRE(error_ready == 0 || (error_ready == 1 && error_out), ADA_EINVAL, "ada_mesh_adaptive_fwd: error_ready=%d (0, or 1 with error_out)", error_ready);
    const Plan q = make_plan(h, w);
    ADA_REQUIRE(workspace_bytes >= q.bytes && (uintptr_t)workspace % 16 == 0 && (uintptr_t)error_out % 8 == 0, ADA_EINVAL,
                "ada_mesh_adaptive_fwd: a 16-byte aligned workspace of %ld bytes needed, got %ld", (long)q.bytes, (long)workspace_bytes);
    const hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const bool with_error = !error_ready && (!no_max_error || error_out);
    for (int32_t img = 0; img < batch; ++img) {      // one image after the other on the stream: they share the workspace
        AdArgs p;
        p.mask = mask ? mask + (int64_t)img * image_stride_bytes : nullptr; p.mask_pitch = (long)row_pitch_bytes;
        p.depth = depth + (int64_t)img * h * w; p.z.inverse = inverse; p.z.a = a; p.z.b = b; p.max_ratio = max_ratio;
        p.h = h; p.w = w; p.N = q.N; p.levels = q.levels;
        p.E = error_out ? error_out + (int64_t)img * h * w : (double*)ws;
        p.tau = no_max_error ? 0.0 : max_error; p.none = no_max_error;
        p.tri = triangles ? triangles + (int64_t)img * capacity * 3 : nullptr; p.capacity = capacity;
        p.lb = q.lb; p.n_sub = q.n_sub; p.list0 = (Node*)(ws + q.off_list0); p.list1 = (Node*)(ws + q.off_list1); p.list_cap = q.list_cap;
        p.sums = (int32_t*)(ws + q.off_sums);
        if (with_error) {
            int l = q.levels - 2;
            for (; l >= 0; --l) {
                int half, rows, cols;
                level_dims(h, w, q.N, l, half, rows, cols);
                if ((int64_t)rows * cols <= AD_FOLD) break;
                hipLaunchKernelGGL(err_level_kernel, dim3((unsigned)((cols + AD_THREADS - 1) / AD_THREADS), (unsigned)rows), dim3(AD_THREADS), 0, s, p, l, half,
                                   cols);
            }
            hipLaunchKernelGGL(err_fold_kernel, dim3(1), dim3(AD_TOP), 0, s, p, l);
        }
        hipLaunchKernelGGL(top_kernel, dim3(1), dim3(AD_TOP), 0, s, p);
        hipLaunchKernelGGL(sub_kernel<false>, dim3((unsigned)q.n_sub), dim3(AD_THREADS), 0, s, p);
        hipLaunchKernelGGL(scan_sums_kernel<AD_SCAN_ITEMS>, dim3(1), dim3(SCAN_THREADS), 0, s, p.sums, (long)q.n_sums, (long)q.n_sums, count + img);
        if (capacity > 0) {
            hipLaunchKernelGGL(sub_kernel<true>, dim3((unsigned)q.n_sub), dim3(AD_THREADS), 0, s, p);
        }
    }
    return ada_check_launch("ada_mesh_adaptive_fwd");
}
