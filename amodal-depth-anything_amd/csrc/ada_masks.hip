// What the reference's demo does to a MASK before the networks see it (reference app.py), on the device: connected-component labelling, the
// per-component statistics of cv2.connectedComponentsWithStats, the area filter of remove_small_noise (app.py:283-293) and the grid of prompt
// points of get_points_from_components (app.py:77-99).  Labelling is the one primitive here that is neither a gather nor a reduction.
//
// Labelling = a union-find over pixel indices (raster index i = y * w + x) whose links ALWAYS point to a smaller-or-equal index: a set is joined to
// another by an integer atomicMin on the larger root's slot.  Consequences the whole file leans on:
//   * every pointer chase strictly decreases, so uf_find from index a takes at most a steps;
//   * the root of a finished component is its smallest index = its first pixel in raster order, so "number the components in the raster order of
//     their first pixel" is a prefix count over root flags, and the result is bit-reproducible although atomics built the forest;
//   * no workgroup waits for another one: inside a kernel there are only lock-free retries (see uf_union), between phases the ordering comes from
//     launch boundaries.  The launch sequence depends on the shape alone -- no host read, no flag loop -- so the call is legal inside a stream capture.
// Phases of ada_mask_label_fwd (six launches):
//   1 cc_tile_kernel     32 x 32 tiles labelled in LDS (tile-local raster order agrees with global raster order: the local root is the tile's minimum)
//   2 cc_border_kernel   unions every neighbour pair that straddles a tile border, the diagonal pairs at tile corners included (8-connectivity)
//   3 cc_resolve_kernel  every tile-local root chases to its global root (read-only: nothing is written that another thread reads); root flags
//                        are counted per chunk of 1024 consecutive pixels
//   4 scan_sums_kernel   (ada_scan.h) exclusive scan of the chunk counts, one workgroup per image; writes n_labels
//   5 cc_number_kernel   roots get base + rank inside the chunk + 1 (ada_scan.h's block_excl_flag), the background 0
//   6 cc_paint_kernel    every other pixel copies its root's number
// Integer atomics only, no scratch (csrc/build.py NO_SCRATCH), nothing allocated.
#include "ada_scan.h"

namespace {

constexpr int CC_T = 32;           // tile edge: 1024 pixels, one per thread
constexpr int CC_CHUNK = 1024;     // pixels per chunk of the root count, one per thread
constexpr int CC_WAVES = CC_CHUNK / ADA_WAVE;
constexpr int CC_SCAN_ITEMS = 1;   // chunk counts per thread and step of the scan
constexpr int CC_STRIP = 64;       // pixels of one row walked by one thread of the run kernels
#define CC_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define CC_AGENT __HIP_MEMORY_SCOPE_AGENT

// Slot encoding of the parent array `par` (int32 per pixel) after phase 1:
//   -1         background
//   <= -2      inside, not a tile-local root: -2 - (global index of its tile-local root).  Never rewritten.
//   >= 0       inside, a tile-local root: the global index of its parent (itself while it is a root).  Only these slots take part in the union-find
//              of phase 2, and they only ever receive non-negative values.
ADA_DEV int cc_node(const int* par, int j) {
    const int u = par[j];      // background / tagged slots never change after phase 1; a root slot stays >= 0 whatever its value
    return u == -1 ? -1 : (u <= -2 ? -2 - u : j);
}

// TERMINATION.  Invariant: p[i] <= i for every slot, and slots only decrease (atomic min with a smaller value).  So q < a whenever q != a below: the
// chase visits strictly decreasing indices and ends after at most a steps, stale reads included (a stale value is an earlier, larger-or-equal link
// of the same slot, still <= its index).
template <int SCOPE>
ADA_DEV int uf_find(int* p, int a) {
    for (;;) {
        const int q = __hip_atomic_load(p + a, __ATOMIC_RELAXED, SCOPE);
        if (q == a) return a;
        a = q;
    }
}

// Joins the sets of a and b.  Each pass of the loop either returns or replaces a by `old` < a (the slot of a had already been lowered by somebody
// else: a failed retry means a link decreased), and the finds never increase a or b: a + b strictly decreases from pass to pass, so there are at
// most a0 + b0 + 1 passes.  Nobody is waited for.  When the atomic min overwrites a link a -> old with a -> b (b < old), this thread goes on to join
// old and b, so the connection the overwritten link carried is re-established before the kernel ends; links only ever join pixels of one component.
template <int SCOPE>
ADA_DEV void uf_union(int* p, int a, int b) {
    for (;;) {
        a = uf_find<SCOPE>(p, a);
        b = uf_find<SCOPE>(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
}

struct TileArgs {
    const uint8_t* mask;
    long pitch, istride, hw;
    int h, w, tiles_x, conn8;
    int* par;
};

// Phase 1.  Block 1024 = one 32 x 32 tile (thread = pixel, a wave = two tile rows), grid (tiles, batch).  Start: every pixel points to the first pixel
// of its horizontal run inside the tile (a scan to the left over at most 31 LDS bytes).  Then each pixel joins the row above: with its upper
// neighbour -- unless the left and upper-left neighbours are inside too, which already carry that connection -- or, under 8-connectivity when the upper
// neighbour is outside, with the upper-left (unless the left neighbour is inside: its own upper neighbour is that pixel) and the upper-right one.
__global__ __launch_bounds__(1024) void cc_tile_kernel(TileArgs a) {
    __shared__ int p[CC_T * CC_T];
    __shared__ uint8_t m[CC_T * CC_T];
    const int tid = threadIdx.x;
    const int lx = tid & (CC_T - 1), ly = tid / CC_T;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const int x = tx * CC_T + lx, y = ty * CC_T + ly;
    const bool in_image = x < a.w && y < a.h;
    const bool inside = in_image && a.mask[(long)blockIdx.y * a.istride + (long)y * a.pitch + x] != 0;
    m[tid] = inside ? 1 : 0;
    __syncthreads();
    int s = lx;
    if (inside)
        while (s > 0 && m[ly * CC_T + s - 1]) --s;
    p[tid] = ly * CC_T + s;
    __syncthreads();
    if (inside && ly > 0) {
        const bool left = lx > 0 && m[tid - 1];
        if (m[tid - CC_T]) {
            if (!(left && m[tid - CC_T - 1])) uf_union<CC_WG>(p, tid, tid - CC_T);
        } else if (a.conn8) {
            if (lx > 0 && !left && m[tid - CC_T - 1]) uf_union<CC_WG>(p, tid, tid - CC_T - 1);
            if (lx < CC_T - 1 && m[tid - CC_T + 1]) uf_union<CC_WG>(p, tid, tid - CC_T + 1);
        }
    }
    __syncthreads();
    if (!in_image) return;
    int v = -1;
    if (inside) {
        const int r = uf_find<CC_WG>(p, tid);      // nothing is written any more: a read-only chase, at most tid steps
        const int g = (ty * CC_T + r / CC_T) * a.w + tx * CC_T + (r & (CC_T - 1));
        v = r == tid ? g : -2 - g;
    }
    a.par[(long)blockIdx.y * a.hw + (long)y * a.w + x] = v;
}

// Phase 2.  One thread per pixel, only those in the first row, the first column or (8-connectivity) the last column of a tile go on.  A pixel joins
// each inside neighbour among left, up, up-left, up-right that lies in ANOTHER tile (pairs inside one tile are phase 1's), with the same economy as
// phase 1: when the upper neighbour is inside, the diagonal ones hang on it through their own row and are skipped.  The up-left pair at a corner
// where four tiles meet (x and y both multiples of 32) and the up-right pair across it are covered by these rules like any other.
__global__ __launch_bounds__(256) void cc_border_kernel(int* par_all, int h, int w, long hw, int conn8) {
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x;
    if (i0 >= hw) return;
    const int i = (int)i0;
    const int y = i / w, x = i - y * w;
    const int mx = x & (CC_T - 1), my = y & (CC_T - 1);
    if (mx != 0 && my != 0 && !(conn8 && mx == CC_T - 1)) return;
    int* par = par_all + (long)blockIdx.y * hw;
    const int me = cc_node(par, i);
    if (me < 0) return;
    if (mx == 0 && x > 0) {
        const int n = cc_node(par, i - 1);
        if (n >= 0) uf_union<CC_AGENT>(par, me, n);
    }
    if (y == 0) return;
    const int up = cc_node(par, i - w);
    if (up >= 0) {
        if (my == 0) uf_union<CC_AGENT>(par, me, up);
    } else if (conn8) {
        if (x > 0 && (my == 0 || mx == 0)) {
            const int n = cc_node(par, i - w - 1);
            if (n >= 0) uf_union<CC_AGENT>(par, me, n);
        }
        if (x < w - 1 && (my == 0 || mx == CC_T - 1)) {
            const int n = cc_node(par, i - w + 1);
            if (n >= 0) uf_union<CC_AGENT>(par, me, n);
        }
    }
}

// Phase 3.  Block 1024 = one chunk of consecutive pixels, grid (chunks, batch).  Only tile-local roots chase (the other pixels are one hop from
// theirs); nothing the chase reads is written in this launch.  The chase strictly decreases: at most i steps.
__global__ __launch_bounds__(1024) void cc_resolve_kernel(const int* par_all, int* aux_all, int* chunk_count, long hw, int nchunks) {
    const long i = (long)blockIdx.x * CC_CHUNK + threadIdx.x;
    const int* par = par_all + (long)blockIdx.y * hw;
    bool root = false;
    if (i < hw) {
        const int v = par[i];
        if (v >= 0) {
            int r = v;
            for (int q = par[r]; q != r; q = par[r]) r = q;
            aux_all[(long)blockIdx.y * hw + i] = r;
            root = r == (int)i;
        }
    }
    __shared__ int lds[CC_WAVES];
    int total;
    block_excl_flag<CC_WAVES>(root, lds, total);
    if (threadIdx.x == 0) chunk_count[(long)blockIdx.y * nchunks + blockIdx.x] = total;
}

// Phase 5: the roots' numbers and the background's 0.  A thread writes its own pixel only.
__global__ __launch_bounds__(1024) void cc_number_kernel(const int* par_all, const int* chunk_base, int* labels_all, long hw, int nchunks) {
    const long i = (long)blockIdx.x * CC_CHUNK + threadIdx.x;
    const int v = i < hw ? par_all[(long)blockIdx.y * hw + i] : -1;
    const bool root = i < hw && v == (int)i;
    __shared__ int lds[CC_WAVES];
    int total;
    const int before = block_excl_flag<CC_WAVES>(root, lds, total);      // every thread of the workgroup: the return comes after it
    if (i >= hw) return;
    if (root) labels_all[(long)blockIdx.y * hw + i] = chunk_base[(long)blockIdx.y * nchunks + blockIdx.x] + before + 1;
    else if (v == -1) labels_all[(long)blockIdx.y * hw + i] = 0;
}

// Phase 6: every inside pixel that is not a root reads its root's number (written in phase 5, written by nobody here).
__global__ __launch_bounds__(256) void cc_paint_kernel(const int* par_all, const int* aux_all, int* labels_all, long hw) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const long img = (long)blockIdx.y * hw;
    const int v = par_all[img + i];
    if (v == -1 || v == (int)i) return;
    const int local_root = v <= -2 ? -2 - v : (int)i;
    labels_all[img + i] = labels_all[img + aux_all[img + local_root]];
}

// ---- statistics, area filter, prompt grid ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void cc_fill_kernel(int* p, long n, int v) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// rows before the accumulation: (min x, min y, max x, max y, area) = (INT_MAX, INT_MAX, -1, -1, 0), sums 0
__global__ __launch_bounds__(256) void cc_stats_init_kernel(int* stats, long long* sums, long rows) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    int* s = stats + r * 5;
    s[0] = 0x7fffffff; s[1] = 0x7fffffff; s[2] = -1; s[3] = -1; s[4] = 0;
    sums[2 * r] = 0; sums[2 * r + 1] = 0;
}

// (min x, min y, max x, max y) -> (LEFT, TOP, WIDTH, HEIGHT); a row without pixels is all zeros
__global__ __launch_bounds__(256) void cc_stats_final_kernel(int* stats, long rows) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    int* s = stats + r * 5;
    if (s[4] == 0) {
        s[0] = 0; s[1] = 0; s[2] = 0; s[3] = 0;
    } else {
        s[2] = s[2] - s[0] + 1;
        s[3] = s[3] - s[1] + 1;
    }
}

struct RunArgs {
    const int* labels;
    int h, w, strips, cap;      // strips per row; labels above cap are ignored
    long hw;
    int* stats;                 // MODE 0: [batch][cap + 1][5]
    long long* sums;            // MODE 0: [batch][cap + 1][2]
    int* area;                  // MODE 1: [batch][cap + 1]
};

// what one thread has gathered for one label along its strip
struct Acc {
    int label;                  // -1: none
    int x0, x1, y0, y1, n;
    long long sx, sy;
};

ADA_DEV void acc_reset(Acc& s, int label) {
    s.label = label; s.x0 = 0x7fffffff; s.x1 = -1; s.y0 = 0x7fffffff; s.y1 = -1; s.n = 0; s.sx = 0; s.sy = 0;
}

// the run [xa, xb] of the strip's row: sum x = (xa + xb) n / 2 (the product is even for every n)
ADA_DEV void acc_add(Acc& s, int xa, int xb) {
    const int n = xb - xa + 1;
    s.x0 = xa < s.x0 ? xa : s.x0;
    s.x1 = xb > s.x1 ? xb : s.x1;
    s.n += n;
    s.sx += (long long)(xa + xb) * n / 2;
}

template <int MODE>
ADA_DEV void acc_flush(const RunArgs& a, int b, const Acc& r) {
    if (r.label < (MODE ? 1 : 0) || r.label > a.cap || r.n <= 0) return;
    const long row = (long)b * (a.cap + 1) + r.label;
    if (MODE) {
        atomicAdd(a.area + row, r.n);
    } else {
        int* s = a.stats + row * 5;
        atomicMin(s + 0, r.x0);
        atomicMin(s + 1, r.y0);
        atomicMax(s + 2, r.x1);
        atomicMax(s + 3, r.y1);
        atomicAdd(s + 4, r.n);
        atomicAdd((unsigned long long*)a.sums + 2 * row, (unsigned long long)r.sx);
        atomicAdd((unsigned long long*)a.sums + 2 * row + 1, (unsigned long long)r.sy);
    }
}

// The wave's accumulators of one slot, merged BY LABEL before they reach memory: the first lane that still holds one names the label, every lane with
// that label joins a shuffle reduction, the naming lane issues the one set of atomics, and the round repeats with the lanes that are left.  A round
// removes at least the naming lane: at most 64 rounds, as many as there are distinct labels in the wave.  Every lane of the wave must call this.
template <int MODE>
ADA_DEV void wave_flush(const RunArgs& a, int b, const Acc& mine) {
    const int lane = threadIdx.x & 63;
    bool have = mine.label >= (MODE ? 1 : 0) && mine.n > 0;
    unsigned long long holders = __ballot(have);
    while (holders) {      // wave-uniform
        const int leader = __ffsll((long long)holders) - 1;
        const int key = __shfl(mine.label, leader);
        const bool join = have && mine.label == key;
        Acc r = mine;
        if (!join) acc_reset(r, key);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            r.n += __shfl_xor(r.n, off);
            if (!MODE) {
                const int ox0 = __shfl_xor(r.x0, off), ox1 = __shfl_xor(r.x1, off), oy0 = __shfl_xor(r.y0, off), oy1 = __shfl_xor(r.y1, off);
                r.x0 = ox0 < r.x0 ? ox0 : r.x0;
                r.x1 = ox1 > r.x1 ? ox1 : r.x1;
                r.y0 = oy0 < r.y0 ? oy0 : r.y0;
                r.y1 = oy1 > r.y1 ? oy1 : r.y1;
                r.sx += __shfl_xor(r.sx, off);
                r.sy += __shfl_xor(r.sy, off);
            }
        }
        if (lane == leader) acc_flush<MODE>(a, b, r);
        have = have && !join;
        holders = __ballot(have);
    }
}

// One thread walks a strip of 64 pixels of one row as runs of equal labels and gathers them in registers: one accumulator for the background and two
// for the two most recently met components (a third label evicts the older of the two, which goes to memory on its own).  So a solid mask, a
// checkerboard and a giant component threaded through noise all cost one accumulator per strip, not one set of atomics per run or per pixel; at the
// end of the strip the wave merges its accumulators by label (wave_flush) and each distinct label of the wave costs ONE set of integer atomics.
// Integer sums: exact, independent of the arrival order.  MODE 0: bounding box, area, sum x, sum y of labels 0..cap.  MODE 1: area of labels 1..cap.
template <int MODE>
__global__ __launch_bounds__(256) void cc_runs_kernel(RunArgs a) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    Acc bg, c1, c2;
    acc_reset(bg, MODE ? -1 : 0);
    acc_reset(c1, -1);
    acc_reset(c2, -1);
    if (s < (long)a.h * a.strips) {
        const int y = (int)(s / a.strips);
        const int xa = (int)(s - (long)y * a.strips) * CC_STRIP;
        const int xb = xa + CC_STRIP < a.w ? xa + CC_STRIP : a.w;
        const int* row = a.labels + (long)b * a.hw + (long)y * a.w;
        bool c1_newer = false;
        int x = xa;
        while (x < xb) {
            const int l = row[x];
            int e = x;
            while (e + 1 < xb && row[e + 1] == l) ++e;      // the run [x, e]
            if (l == 0) {
                if (!MODE) acc_add(bg, x, e);
            } else if (l > 0) {                             // a negative label is nobody's: ignored
                if (l == c1.label) {
                    acc_add(c1, x, e);
                    c1_newer = true;
                } else if (l == c2.label) {
                    acc_add(c2, x, e);
                    c1_newer = false;
                } else if (c1_newer) {                      // evict c2, the older one
                    c2.y0 = y; c2.y1 = y; c2.sy = (long long)y * c2.n;
                    acc_flush<MODE>(a, b, c2);
                    acc_reset(c2, l);
                    acc_add(c2, x, e);
                    c1_newer = false;
                } else {
                    c1.y0 = y; c1.y1 = y; c1.sy = (long long)y * c1.n;
                    acc_flush<MODE>(a, b, c1);
                    acc_reset(c1, l);
                    acc_add(c1, x, e);
                    c1_newer = true;
                }
            }
            x = e + 1;
        }
        bg.y0 = y; bg.y1 = y; bg.sy = (long long)y * bg.n;
        c1.y0 = y; c1.y1 = y; c1.sy = (long long)y * c1.n;
        c2.y0 = y; c2.y1 = y; c2.sy = (long long)y * c2.n;
    }
    // every lane takes part in the votes and shuffles, whether it walked a strip or not
    if (!MODE) wave_flush<MODE>(a, b, bg);
    wave_flush<MODE>(a, b, c1);
    wave_flush<MODE>(a, b, c2);
}

__global__ __launch_bounds__(256) void cc_keep_kernel(const int* labels, const int* area, long hw, int cap, int min_area, uint8_t* out_u8, float* out_f32) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const long img = (long)blockIdx.y * hw;
    const int l = labels[img + i];
    const bool keep = l > 0 && l <= cap && area[(long)blockIdx.y * (cap + 1) + l] >= min_area;
    if (out_u8) out_u8[img + i] = keep ? 1 : 0;
    if (out_f32) out_f32[img + i] = keep ? 1.f : 0.f;
}

// range(top, top + height - 1, step) x range(left, left + width - 1, step) of app.py:94-97, inside the component itself
__global__ __launch_bounds__(256) void cc_grid_kernel(const int* labels, const int* stats, int w, long hw, int cap, int thresh, int step, int* hit) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const long img = (long)blockIdx.y * hw;
    const int l = labels[img + i];
    int out = 0;
    if (l > 0 && l <= cap) {
        const int* s = stats + ((long)blockIdx.y * (cap + 1) + l) * 5;
        const int y = (int)(i / w), x = (int)(i - (long)y * w);
        const int dx = x - s[0], dy = y - s[1];
        if (s[4] >= thresh && dx >= 0 && dy >= 0 && dy % step == 0 && dy < s[3] - 1 && dx % step == 0 && dx < s[2] - 1) out = l;
    }
    hit[img + i] = out;
}

unsigned blocks_of(long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

// two int32 per pixel (parents, resolved roots) and one per chunk of 1024 pixels (root counts), per image
static int64_t label_workspace_bytes(int32_t batch, int32_t h, int32_t w) {
    const int64_t hw = (int64_t)h * w;
    return (int64_t)batch * (2 * hw + (hw + CC_CHUNK - 1) / CC_CHUNK) * 4;
}

extern "C" int ada_mask_label_fwd(const uint8_t* mask, int32_t batch, int32_t h, int32_t w, int64_t row_pitch_bytes, int64_t image_stride_bytes,
                                  int32_t connectivity, int32_t* labels, int32_t* n_labels, void* workspace, int64_t workspace_bytes, void* stream) {
    ADA_REQUIRE(mask && labels && n_labels, ADA_EINVAL, "ada_mask_label_fwd: null pointer");
    ADA_REQUIRE(batch > 0 && h > 0 && w > 0, ADA_EINVAL, "ada_mask_label_fwd: bad shape batch=%d %dx%d", batch, h, w);
    ADA_REQUIRE(connectivity == 4 || connectivity == 8, ADA_EINVAL, "ada_mask_label_fwd: connectivity %d (4 or 8)", connectivity);
    ADA_REQUIRE(row_pitch_bytes >= (int64_t)w, ADA_EINVAL, "ada_mask_label_fwd: row pitch %ld < %d pixels", (long)row_pitch_bytes, w);
    ADA_REQUIRE(batch == 1 || image_stride_bytes >= (int64_t)(h - 1) * row_pitch_bytes + w, ADA_EINVAL,
                "ada_mask_label_fwd: image stride %ld overlaps the previous image", (long)image_stride_bytes);
    const int64_t hw = (int64_t)h * w;
    ADA_REQUIRE(hw < ((int64_t)1 << 31) && batch <= 65535, ADA_EUNSUPPORTED, "ada_mask_label_fwd: h * w must stay below 2^31 and batch within 65535");
    const int64_t need = label_workspace_bytes(batch, h, w);
    ADA_REQUIRE(workspace && workspace_bytes >= need, ADA_EINVAL, "ada_mask_label_fwd: the workspace needs %ld bytes, got %ld", (long)need,
                (long)(workspace ? workspace_bytes : 0));
    const hipStream_t s = (hipStream_t)stream;
    const int nchunks = (int)((hw + CC_CHUNK - 1) / CC_CHUNK);
    int* par = (int*)workspace;
    int* aux = par + (int64_t)batch * hw;
    int* chunks = aux + (int64_t)batch * hw;
    TileArgs t;
    t.mask = mask; t.pitch = row_pitch_bytes; t.istride = batch == 1 ? 0 : (long)image_stride_bytes; t.hw = hw;
    t.h = h; t.w = w; t.tiles_x = (w + CC_T - 1) / CC_T; t.conn8 = connectivity == 8; t.par = par;
    const long tiles = (long)t.tiles_x * ((h + CC_T - 1) / CC_T);
    hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(CC_T * CC_T), 0, s, t);
    hipLaunchKernelGGL(cc_border_kernel, dim3(blocks_of(hw, 256), (unsigned)batch), dim3(256), 0, s, par, h, w, (long)hw, t.conn8);
    hipLaunchKernelGGL(cc_resolve_kernel, dim3((unsigned)nchunks, (unsigned)batch), dim3(CC_CHUNK), 0, s, par, aux, chunks, (long)hw, nchunks);
    hipLaunchKernelGGL(scan_sums_kernel<CC_SCAN_ITEMS>, dim3((unsigned)batch), dim3(SCAN_THREADS), 0, s, chunks, (long)nchunks, (long)nchunks, n_labels);
    hipLaunchKernelGGL(cc_number_kernel, dim3((unsigned)nchunks, (unsigned)batch), dim3(CC_CHUNK), 0, s, par, chunks, labels, (long)hw, nchunks);
    hipLaunchKernelGGL(cc_paint_kernel, dim3(blocks_of(hw, 256), (unsigned)batch), dim3(256), 0, s, par, aux, labels, (long)hw);
    return ada_check_launch("ada_mask_label_fwd");
}

static int check_label_map(const char* who, const void* labels, int32_t batch, int32_t h, int32_t w) {
    ADA_REQUIRE(labels, ADA_EINVAL, "%s: null pointer", who);
    ADA_REQUIRE(batch > 0 && h > 0 && w > 0, ADA_EINVAL, "%s: bad shape batch=%d %dx%d", who, batch, h, w);
    ADA_REQUIRE((int64_t)h * w < ((int64_t)1 << 31) && batch <= 65535, ADA_EUNSUPPORTED, "%s: h * w must stay below 2^31 and batch within 65535", who);
    return ADA_OK;
}

extern "C" int ada_mask_stats_fwd(const int32_t* labels, int32_t batch, int32_t h, int32_t w, int32_t max_labels, int32_t* stats, int64_t* sums,
                                  void* stream) {
    const int rc = check_label_map("ada_mask_stats_fwd", labels, batch, h, w);
    if (rc != ADA_OK) return rc;
    ADA_REQUIRE(stats && sums, ADA_EINVAL, "ada_mask_stats_fwd: null pointer");
    ADA_REQUIRE(max_labels >= 0 && max_labels < 0x7fffffff, ADA_EINVAL, "ada_mask_stats_fwd: max_labels %d", max_labels);
    const hipStream_t s = (hipStream_t)stream;
    const long rows = (long)batch * ((long)max_labels + 1);
    RunArgs a;
    a.labels = labels; a.h = h; a.w = w; a.strips = (w + CC_STRIP - 1) / CC_STRIP; a.cap = max_labels; a.hw = (long)h * w;
    a.stats = stats; a.sums = (long long*)sums; a.area = nullptr;
    hipLaunchKernelGGL(cc_stats_init_kernel, dim3(blocks_of(rows, 256)), dim3(256), 0, s, stats, (long long*)sums, rows);
    hipLaunchKernelGGL(cc_runs_kernel<0>, dim3(blocks_of((long)h * a.strips, 256), (unsigned)batch), dim3(256), 0, s, a);
    hipLaunchKernelGGL(cc_stats_final_kernel, dim3(blocks_of(rows, 256)), dim3(256), 0, s, stats, rows);
    return ada_check_launch("ada_mask_stats_fwd");
}

extern "C" int ada_mask_keep_area_fwd(const int32_t* labels, int32_t batch, int32_t h, int32_t w, int32_t min_area, uint8_t* out_u8, float* out_f32,
                                      void* workspace, int64_t workspace_bytes, void* stream) {
    const int rc = check_label_map("ada_mask_keep_area_fwd", labels, batch, h, w);
    if (rc != ADA_OK) return rc;
    ADA_REQUIRE(out_u8 || out_f32, ADA_EINVAL, "ada_mask_keep_area_fwd: null pointer (both outputs)");
    const long hw = (long)h * w;
    const long per_image = hw / 2 + 2;      // labels 0 .. ceil(hw / 2): no grid holds more components under either connectivity
    const int64_t need = (int64_t)batch * per_image * 4;
    ADA_REQUIRE(workspace && workspace_bytes >= need, ADA_EINVAL, "ada_mask_keep_area_fwd: the workspace needs %ld bytes, got %ld", (long)need,
                (long)(workspace ? workspace_bytes : 0));
    const hipStream_t s = (hipStream_t)stream;
    RunArgs a;
    a.labels = labels; a.h = h; a.w = w; a.strips = (w + CC_STRIP - 1) / CC_STRIP; a.cap = (int)(per_image - 1); a.hw = hw;
    a.stats = nullptr; a.sums = nullptr; a.area = (int*)workspace;
    hipLaunchKernelGGL(cc_fill_kernel, dim3(blocks_of((long)batch * per_image, 256)), dim3(256), 0, s, a.area, (long)batch * per_image, 0);
    hipLaunchKernelGGL(cc_runs_kernel<1>, dim3(blocks_of((long)h * a.strips, 256), (unsigned)batch), dim3(256), 0, s, a);
    hipLaunchKernelGGL(cc_keep_kernel, dim3(blocks_of(hw, 256), (unsigned)batch), dim3(256), 0, s, labels, (const int*)a.area, hw, a.cap, min_area, out_u8, out_f32);
    return ada_check_launch("ada_mask_keep_area_fwd");
}

extern "C" int ada_mask_grid_points_fwd(const int32_t* labels, const int32_t* stats, int32_t batch, int32_t h, int32_t w, int32_t max_labels,
                                        int32_t small_component_thresh, int32_t grid_step, int32_t* hit, void* stream) {
    const int rc = check_label_map("ada_mask_grid_points_fwd", labels, batch, h, w);
    if (rc != ADA_OK) return rc;
    ADA_REQUIRE(stats && hit, ADA_EINVAL, "ada_mask_grid_points_fwd: null pointer");
    ADA_REQUIRE(max_labels >= 0 && max_labels < 0x7fffffff, ADA_EINVAL, "ada_mask_grid_points_fwd: max_labels %d", max_labels);
    ADA_REQUIRE(grid_step >= 1, ADA_EINVAL, "ada_mask_grid_points_fwd: grid_step %d must be positive", grid_step);
    const long hw = (long)h * w;
    hipLaunchKernelGGL(cc_grid_kernel, dim3(blocks_of(hw, 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, labels, stats, w, hw, max_labels,
                       small_component_thresh, grid_step, hit);
    return ada_check_launch("ada_mask_grid_points_fwd");
}
