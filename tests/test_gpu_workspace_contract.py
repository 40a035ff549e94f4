"""GPU: the workspace contract of the domain kernels -- the 14 wrappers of hip_ext that take ``workspace=`` and pil_resize_u8's ``tmp=``.

Each wrapper is handed EXACTLY the bytes its ``*_workspace_bytes`` declares (not rounded up), cut out of a larger buffer whose 4096 bytes on either side
carry a guard pattern, and pre-filled three ways: with 0x00, with 0xFF, and with whatever a call on a busier input of the same shape (more valid pixels,
components, triangles, edges: every count it leaves is larger) left behind.  Each time the outputs -- pre-filled with 0xA5 bytes where the caller
allocates them -- equal the restatement the wrapper's own test file uses, to that file's standard (array_equal everywhere but the two fp64 edge sums,
which keep their counted-roundings bound), the three runs' outputs are byte-identical to each other, the guards are intact, and a workspace one byte
shorter is refused.  So a counter, histogram, flag array or z-buffer that is not cleared, a size formula that is short and a store past the declared size
each turn a test red.  Shapes: the smallest of each wrapper's own tests at a tile or chunk edge, one of them odd and across a chunk, and one pixel
high / wide where the wrapper takes it."""
import math

import numpy as np
import pytest
import torch

import _adaptive_ref as A_REF
import _components_ref as C_REF
import _edges_ref as E_REF
import _filters_ref as F_REF
import _geometry_ref as G_REF
import _pil_resample as P_REF
import _raster_ref as R_REF
import test_gpu_adaptive_mesh as T_ADAPT
import test_gpu_edges as T_EDGES
import test_gpu_filters as T_FILT
import test_gpu_geometry as T_GEOM
import test_gpu_pil_resize as T_PIL
import test_gpu_protocol as T_PROT
import test_gpu_quantile as T_QUANT
import test_gpu_raster as T_RAST

pytestmark = pytest.mark.gpu

G = 4096
GUARD, POISON = 0x5A, 0xA5
STATES = ("0x00", "0xff", "used")


def guarded(need, fill):
    """(workspace, check): ``need`` bytes filled with ``fill`` between two bands of G guard bytes, 16-byte aligned; check(what) asserts the bands untouched
    and names the first changed byte by its offset from the END of the workspace (>= 0: written past it; < -need: written in front of it)."""
    buf = torch.full((G + need + G,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    ws = buf[G:G + need]
    ws.fill_(fill)
    assert ws.is_contiguous() and ws.numel() == need and ws.data_ptr() % 16 == 0

    def check(what):
        torch.cuda.synchronize()
        for band, base in ((buf[G + need:], 0), (buf[:G], -(need + G))):
            bad = torch.nonzero(band != GUARD)
            assert bad.numel() == 0, (f"{what}: {bad.numel()} guard bytes overwritten, the first at offset {int(bad[0]) + base:+d} from the end of the "
                                      f"{need}-byte workspace")
    return ws, check


def poisoned(shape, dtype):
    """A device tensor of ``shape`` whose every byte is 0xA5."""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), POISON, dtype=torch.uint8, device="cuda").view(dtype).view(*shape)


def is_poison(t):
    return bool((t.contiguous().view(torch.uint8) == POISON).all())


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def three_states(hip, what, need, call, busier, refuse=True):
    """``call(ws)`` -> the wrapper's output tensors; ``busier(ws)``: the same wrapper on the busier input.  Runs ``call`` on the three pre-filled workspaces,
    holds the outputs of the three runs to each other byte for byte, checks the guards every time and the refusal of need - 1 bytes; returns the
    first run's outputs for the comparison with the reference."""
    assert need > 0, (what, need)
    runs = []
    for state in STATES:
        ws, check = guarded(need, 0xFF if state == "0xff" else 0x00)
        if state == "used":
            busier(ws)
            check(f"{what}: the busier call")
        outs = call(ws)
        check(f"{what}: workspace pre-filled {state}")
        runs.append([o.clone() for o in outs])
    for state, outs in zip(STATES[1:], runs[1:]):
        for k, (a, b) in enumerate(zip(runs[0], outs)):
            same = torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
            if not same:
                diff = torch.nonzero(a.contiguous().view(torch.uint8).reshape(-1) != b.contiguous().view(torch.uint8).reshape(-1))
                raise AssertionError(f"{what}: output {k} on a workspace pre-filled {state} differs from the run on zeros in {diff.numel()} bytes, the first at "
                                     f"byte {int(diff[0])} (element {int(diff[0]) // a.element_size()} of {tuple(a.shape)} {a.dtype}): the result depends on what the workspace held")
    if refuse:
        short, check = guarded(need - 1, 0x00)
        with pytest.raises(hip.HipExtError):
            call(short)
        check(f"{what}: the refused call")
    return runs[0]


# ---- protocol_fit / protocol_eval (chunk: 4096 pixels; h * w % 4 == 0 takes the vector loads) ------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 65, 67), (2, 64, 68), (1, 1, 70)], ids=str)      # odd, two chunks, scalar loads; two chunks, vector loads; one row
def test_protocol_fit_and_eval(hip, shape):
    """Exact sums on dyadic inputs, the standard of test_gpu_protocol.test_exact_sums_on_dyadic_inputs."""
    B, h, w = shape
    s, t = T_PROT._dyadic_scene(B, h, w, seed=h), T_PROT._dyadic_scene(B, h, w, seed=h + 1)
    for k in ("whole", "visible", "invisible", "valid"):      # the busier scene: every pixel in every mask
        t[k] = np.ones_like(t[k])
    eps = 2.0 ** -7
    fit = np.zeros((B, hip.FIT_NCOL))
    fit[:, hip.FIT_SCALE], fit[:, hip.FIT_SHIFT] = 2.0, 0.25
    ds, dt, dfit = {k: dev(v) for k, v in s.items()}, {k: dev(v) for k, v in t.items()}, dev(fit)
    need = hip.protocol_workspace_bytes(B, h, w)
    assert need == B * -(-h * w // hip.PROTOCOL_CHUNK) * hip.PROTOCOL_WS_DOUBLES * 8
    rows, = three_states(hip, f"protocol_fit {shape}", need, lambda ws: (hip.protocol_fit(ds["pred"], ds["obs"], ds["visible"], ds["whole"], workspace=ws),),
                         lambda ws: hip.protocol_fit(dt["pred"], dt["obs"], dt["visible"], dt["whole"], workspace=ws))
    sums, = three_states(hip, f"protocol_eval {shape}", need,
                         lambda ws: (hip.protocol_eval(ds["pred"], ds["gt"], ds["invisible"], ds["valid"], dfit, eps=eps, workspace=ws),),
                         lambda ws: hip.protocol_eval(dt["pred"], dt["gt"], dt["invisible"], dt["valid"], dfit, eps=eps, workspace=ws))
    rows, sums = rows.cpu().numpy(), sums.cpu().numpy()
    p64, g64, o64 = (s[k].astype(np.float64) for k in ("pred", "gt", "obs"))
    for b in range(B):
        v = s["visible"][b]
        assert v.any()
        want = {hip.FIT_N: v.sum(), hip.FIT_SUM_P: p64[b][v].sum(), hip.FIT_SUM_O: o64[b][v].sum(), hip.FIT_SUM_PP: (p64[b][v] ** 2).sum(),
                hip.FIT_SUM_PO: (p64[b][v] * o64[b][v]).sum(), hip.FIT_MIN_P: p64[b][v].min(), hip.FIT_MAX_P: p64[b][v].max(),
                hip.FIT_N_VISIBLE: v.sum(), hip.FIT_N_WHOLE: s["whole"][b].sum()}
        for col, val in want.items():
            assert rows[b, col].tobytes() == np.float64(val).tobytes(), (b, col, rows[b, col], val)
        m = s["invisible"][b] & s["valid"][b]
        g = g64[b][m] + eps
        for r, p in enumerate((p64[b][m] + eps, p64[b][m] * 2.0 + 0.25 + eps)):
            want = {hip.EVAL_N: m.sum(), hip.EVAL_SUM_P: p.sum(), hip.EVAL_SUM_G: g.sum(), hip.EVAL_SUM_PP: (p * p).sum(), hip.EVAL_SUM_PG: (p * g).sum(),
                    hip.EVAL_SQ: ((p - g) ** 2).sum()}
            for col, val in want.items():
                assert sums[b, r, col].tobytes() == np.float64(val).tobytes(), (b, r, col, sums[b, r, col], val)
            ratio = np.maximum(p / g, g / p)
            assert min(float(np.abs(ratio - th).min()) for th in T_PROT.THRESHOLDS) >= 1e-6      # no ratio near a threshold
            for col, th in zip((hip.EVAL_D1, hip.EVAL_D2, hip.EVAL_D3), T_PROT.THRESHOLDS):
                assert sums[b, r, col] == float((ratio < th).sum()), (b, r, col)


# ---- mask_label / mask_keep_area (32 x 32 tile, 1024-pixel chunk, 64-pixel strip) --------------------------------------------------------------

def _mask_pairs(h, w):
    masks = np.stack([C_REF.random_mask(h, w, 0.59, h * 31 + w), C_REF.random_mask(h, w, 0.3, h * 31 + w + 1)])
    board = C_REF.checkerboard(h, w)      # under 4-connectivity every set pixel is a component of its own: as many labels as a mask can have
    return masks, np.stack([board, 1 - board])


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("hw", [(65, 65), (130, 70), (1, 67), (67, 1)], ids=str)
def test_mask_label(hip, hw, conn):
    h, w = hw
    masks, busy = _mask_pairs(h, w)
    K = masks.shape[0]
    src, src_busy = dev(masks * 255), dev(busy)
    need = hip.mask_label_workspace_bytes(K, h, w)

    def call(ws, s=src):
        labels, count = poisoned((K, h, w), torch.int32), poisoned((K,), torch.int32)
        hip.mask_label(s, K, h, w, w, h * w, conn, labels, count, ws)
        return labels, count
    labels, count = three_states(hip, f"mask_label {hw} conn {conn}", need, call, lambda ws: call(ws, src_busy))
    for k in range(K):
        want, n = C_REF.label(masks[k], conn)
        assert int(count[k]) == n and np.array_equal(labels[k].cpu().numpy(), want), (k, int(count[k]), n)


@pytest.mark.parametrize("hw", [(65, 65), (37, 53), (1, 67), (67, 1)], ids=str)
def test_mask_keep_area(hip, hw):
    h, w = hw
    masks, busy = _mask_pairs(h, w)
    K, conn, min_area = masks.shape[0], 4, 3
    lab, lab_busy = (dev(np.stack([C_REF.label(m, conn)[0] for m in ms]).astype(np.int32)) for ms in (masks, busy))
    assert int(lab_busy.max()) == max(int(b.sum()) for b in busy) >= (h * w) // 2      # the highest label a map of this size can hold
    need = hip.mask_keep_area_workspace_bytes(K, h, w)

    def call(ws, labels=lab, area=min_area):
        u8, f32 = poisoned((K, h, w), torch.uint8), poisoned((K, h, w), torch.float32)
        hip.mask_keep_area(labels, area, out_u8=u8, out_f32=f32, workspace=ws)
        return u8, f32
    u8, f32 = three_states(hip, f"mask_keep_area {hw}", need, call, lambda ws: call(ws, lab_busy, 1))
    for k in range(K):
        want = C_REF.keep_area(masks[k], min_area, conn)
        assert np.array_equal(u8[k].cpu().numpy(), want) and np.array_equal(f32[k].cpu().numpy(), want.astype(np.float32)), k


# ---- quantile_select (chunk: QUANTILE_CHUNK elements) ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ["chunk+1", 257, 1], ids=str)
def test_quantile_select(hip, n):
    n = hip.QUANTILE_CHUNK + 1 if n == "chunk+1" else n
    rng = np.random.default_rng(n)
    B, qs = 3, T_QUANT.NUMPY_Q
    x = rng.standard_normal((B, n)).astype(np.float32)
    valid = np.stack([rng.random(n) < 0.7, rng.random(n) < 0.4, np.zeros(n, bool)])
    valid[0, 0] = True
    busy = (rng.standard_normal((B, n)) * 1e3).astype(np.float32)      # every element of every image in the population, other leading digits
    dx, dv, db = dev(x), dev(valid.astype(np.uint8)), dev(busy)
    need = hip.quantile_workspace_bytes(B)

    def call(ws, data=dx, v=dv):
        out, out32, count = poisoned((B, len(qs)), torch.float64), poisoned((B, len(qs)), torch.float32), poisoned((B,), torch.int64)
        hip.quantile_select(data, qs, out, out_f32=out32, count=count, valid=v, mode=hip.Q_NUMPY, workspace=ws)
        return out, out32, count
    out, out32, count = three_states(hip, f"quantile_select n={n}", need, call, lambda ws: call(ws, db, None))
    want, wcnt = T_QUANT._reference(x, qs, valid)
    T_QUANT._exact(count.cpu().numpy(), wcnt)
    T_QUANT._exact(out.cpu().numpy(), want)


# ---- mesh_triangles / mesh_compact (chunk: GEOM_CHUNK = 1024 cells / pixels) -------------------------------------------------------------------

def _mesh_masks(h, w):
    masks = np.stack([T_GEOM._mask(h, w, h + w, 0.8), T_GEOM._ellipse(h, w) if min(h, w) > 8 else T_GEOM._mask(h, w, 5, 0.5)])
    return masks, np.ones_like(masks)


@pytest.mark.parametrize("hw", [(34, 33), (70, 130), (1, 9), (9, 1)], ids=str)      # 1056 cells: odd and one past a chunk; 8901 cells; no cell at all
def test_mesh_triangles(hip, hw):
    h, w = hw
    masks, busy = _mesh_masks(h, w)
    B, cap = masks.shape[0], max(2 * (h - 1) * (w - 1), 4)
    depth = np.stack([T_GEOM._ratio_map(h, w, 21 + b) for b in range(B)]) if min(h, w) > 8 else None
    dm, dbusy, dd = dev(masks), dev(busy), dev(depth)
    need = hip.mesh_triangles_workspace_bytes(B, h, w)

    def call(ws, m=dm, d=dd, ratio=2.0):
        tri, count = poisoned((B, cap, 3), torch.int32), poisoned((B,), torch.int32)
        hip.mesh_triangles(B, h, w, tri, count, mask=m, row_pitch=w, image_stride=h * w, depth=d, max_ratio=ratio if d is not None else 0.0, workspace=ws)
        return tri, count
    tri, count = three_states(hip, f"mesh_triangles {hw}", need, call, lambda ws: call(ws, dbusy, None))
    for b in range(B):
        want = G_REF.triangles(h, w, masks[b], depth=None if depth is None else depth[b], max_ratio=None if depth is None else 2.0)
        n = want.shape[0]
        assert int(count[b]) == n <= cap and np.array_equal(tri[b, :n].cpu().numpy(), want) and is_poison(tri[b, n:]), (b, int(count[b]), n)


@pytest.mark.parametrize("hw", [(33, 31), (2, 513), (70, 130), (1, 9)], ids=str)      # 1023 pixels, odd; 1026: one past a chunk; 9100; no triangle at all
def test_mesh_compact(hip, hw):
    h, w = hw
    masks, busy = _mesh_masks(h, w)
    B, cap = masks.shape[0], max(2 * (h - 1) * (w - 1), 4)
    rng = np.random.default_rng(h * w)
    pts = np.stack([G_REF.points(T_GEOM._depth(h, w, 30 + b)) for b in range(B)]).astype(np.float32).reshape(B, h * w, 3)
    cols = rng.integers(0, 256, size=(B, h * w, 3)).astype(np.uint8)

    def lists(ms):      # the triangle lists of mesh_triangles, rows from count on poisoned
        tri = np.full((B, cap, 3), np.frombuffer(bytes([POISON] * 4), np.int32)[0], np.int32)
        count = np.zeros(B, np.int32)
        for b, m in enumerate(ms):
            t = G_REF.triangles(h, w, m)
            tri[b, :t.shape[0]], count[b] = t, t.shape[0]
        return dev(tri), dev(count)
    (tri0, count0), (tri_busy, count_busy) = lists(masks), lists(busy)
    dp, dc = dev(pts), dev(cols)
    vcap = h * w + 3
    need = hip.mesh_compact_workspace_bytes(B, h, w)

    def call(ws, t=tri0, c=count0):
        tri = t.clone()      # rewritten in place
        p_out, c_out, v_count = poisoned((B, vcap, 3), torch.float32), poisoned((B, vcap, 3), torch.uint8), poisoned((B,), torch.int32)
        hip.mesh_compact(tri, c, h, w, dp, p_out, v_count, colors=dc, colors_out=c_out, workspace=ws)
        return tri, p_out, c_out, v_count
    tri, p_out, c_out, v_count = three_states(hip, f"mesh_compact {hw}", need, call, lambda ws: call(ws, tri_busy, count_busy))
    for b in range(B):
        p, t, n, c = G_REF.compact(G_REF.triangles(h, w, masks[b]), pts[b], cols[b])
        assert int(v_count[b]) == n, (b, int(v_count[b]), n)
        assert np.array_equal(tri[b, :t.shape[0]].cpu().numpy(), t) and is_poison(tri[b, t.shape[0]:]), b
        assert T_GEOM._same(p_out[b, :n].cpu().numpy(), p[:n]) and is_poison(p_out[b, n:]), b
        assert np.array_equal(c_out[b, :n].cpu().numpy(), c[:n]) and is_poison(c_out[b, n:]), b


# ---- mesh_raster: 8 bytes per pixel rounded up to 16, 16 bytes of counters, one int32 per triangle ---------------------------------------------

@pytest.mark.parametrize("hw", [(5, 257), (7, 9), (70, 50), (1, 9), (9, 1)], ids=str)      # h * w odd three times: the alignment slack of the z-buffer is in use
def test_mesh_raster(hip, hw):
    from hip_ext import geometry as GEO
    h, w = hw
    pts, tri, colors = T_RAST.crossing_mesh(h, w, seed=h * 1000 + w)
    pts_busy, tri_busy, colors_busy = T_RAST.crossing_mesh(h, w, seed=h * 1000 + w + 1)
    # the busier mesh: every triangle covers the whole target (the list of large triangles is as long as it can be), nearer ones later in the list
    pts_busy = T_RAST.points_of(np.concatenate([[(-3.0 - k, -2.0, 30.0 - k), (2.5 * w + 4, -2.5 - k, 30.0 - k), (-3.5, 2.5 * h + 4 + k, 30.0 - k)] for k in range(tri.shape[0])]))
    tri_busy = np.arange(3 * tri.shape[0]).reshape(-1, 3)
    V, T = pts.shape[0], tri.shape[0]
    assert T % 2 == 1 and pts_busy.shape[0] == V and tri_busy.shape[0] == T      # an odd list behind the counters
    cam, pose = GEO._view_camera("test", h, w, T_RAST.UNIT_K, 55.0, None, None)
    mode, ab, fill = GEO._view_out("test", "w", None, None)

    def project(p):
        x, y, wv = poisoned((V,), torch.int32), poisoned((V,), torch.int32), poisoned((V,), torch.float64)
        hip.mesh_project(dev(p), cam, x, y, wv, pose=pose)
        return x, y, wv
    rec, rec_busy = project(pts), project(pts_busy)
    dt, dt_busy, dc, dc_busy = dev(tri.astype(np.int32)), dev(tri_busy.astype(np.int32)), dev(colors), dev(colors_busy)
    need = hip.mesh_raster_workspace_bytes(h, w, T)
    assert need == 8 * (h * w + (h * w) % 2) + 16 + 4 * T

    def call(ws, r=rec, t=dt, c=dc):
        depth, index, color = poisoned((h, w), torch.float32), poisoned((h, w), torch.int32), poisoned((h, w, 3), torch.uint8)
        hip.mesh_raster(*r, t, h, w, depth, index, colors=c, color=color, mode=mode, inverse=ab, fill=fill, workspace=ws)
        return depth, index, color
    depth, index, color = three_states(hip, f"mesh_raster {hw}", need, call, lambda ws: call(ws, rec_busy, dt_busy, dc_busy))
    want = R_REF.render(pts, tri, h, w, colors=colors, K=T_RAST.UNIT_K, out="w")
    assert np.array_equal(index.cpu().numpy(), want.index)
    assert np.array_equal(depth.cpu().numpy().view(np.int32), want.depth.view(np.int32))
    assert np.array_equal(color.cpu().numpy(), want.color)


# ---- mesh_adaptive (cell: 32) -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(12, 19), (70, 53), (2, 9)], ids=str)
def test_mesh_adaptive(hip, hw):
    h, w = hw
    B, cap = 2, 2 * (h - 1) * (w - 1)
    depth = np.stack([T_ADAPT._depth(h, w, 11 * h + w + b) for b in range(B)])
    rough = np.stack([T_ADAPT._depth(h, w, 500 + b, bad=False) for b in range(B)])
    dd, dr = dev(depth), dev(rough)
    need = hip.mesh_adaptive_workspace_bytes(h, w)

    def call(ws, d=dd, tau=0.02, ratio=1.5):
        tri, count, err = poisoned((B, cap, 3), torch.int32), poisoned((B,), torch.int32), poisoned((B, h, w), torch.float64)
        hip.mesh_adaptive(B, h, w, d, tri, count, max_ratio=ratio, max_error=tau, error=err, workspace=ws)
        return tri, count, err
    tri, count, err = three_states(hip, f"mesh_adaptive {hw}", need, call, lambda ws: call(ws, dr, 0.0, 0.0))      # the busier call: every leaf of a map without holes
    for b in range(B):
        want, E = A_REF.adaptive_triangles(depth[b], max_ratio=1.5, max_error=0.02, return_error=True)
        n = want.shape[0]
        assert int(count[b]) == n <= cap and np.array_equal(tri[b, :n].cpu().numpy(), want) and is_poison(tri[b, n:]), (b, int(count[b]), n)
        assert np.array_equal(T_ADAPT._bits(err[b].cpu().numpy()), T_ADAPT._bits(E)), b


# ---- canny_hysteresis / edt / edge_metric_sums / soft_edge --------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(65, 65), (47, 61), (1, 67), (67, 1)], ids=str)
def test_canny_hysteresis(hip, hw):
    rng = np.random.default_rng(hw[0] * 7 + hw[1])
    maps = T_EDGES._hysteresis_maps()
    lm = np.stack([maps[f"random {hw}"], maps["chain"] if hw == (65, 65) else np.where(rng.random(hw) < 0.3, rng.uniform(0.05, 0.3, hw), 0).astype(np.float32)])
    busy = np.where(rng.random(lm.shape) < 0.7, rng.uniform(0.05, 0.5, lm.shape), 0).astype(np.float32)      # more weak pixels, more components, more strong ones
    B, h, w = lm.shape
    dl, db = dev(lm), dev(busy)
    need = hip.canny_hysteresis_workspace_bytes(B, h, w)

    def call(ws, t=dl):
        edges = poisoned((B, h, w), torch.uint8)
        hip.canny_hysteresis(t, 0.2, edges, workspace=ws)
        return (edges,)
    edges, = three_states(hip, f"canny_hysteresis {hw}", need, call, lambda ws: call(ws, db))
    for b in range(B):
        assert np.array_equal(edges[b].cpu().numpy(), E_REF.hysteresis(lm[b], 0.2)), b


@pytest.mark.parametrize("hw", [(65, 65), (47, 61), (1, 67), (67, 1)], ids=str)
def test_edt(hip, hw):
    rng = np.random.default_rng(11)
    h, w = hw
    one = np.zeros(hw, np.uint8)
    one[h - 1, w - 1] = 1
    maps = np.stack([one, (rng.random(hw) < 0.01).astype(np.uint8), (rng.random(hw) < 0.3).astype(np.uint8), np.zeros(hw, np.uint8)])
    B = maps.shape[0]
    dm, db = dev(maps), dev(np.ones_like(maps))
    need = hip.edt_workspace_bytes(B, h, w)

    def call(ws, m=dm):
        out = poisoned((B, h, w), torch.float64)
        hip.edt(m, out, workspace=ws)
        return (out,)
    out, = three_states(hip, f"edt {hw}", need, call, lambda ws: call(ws, db))
    for b in range(B):
        assert np.array_equal(out[b].cpu().numpy(), E_REF.edt(maps[b])), b


@pytest.mark.parametrize("hw", [(47, 61), (65, 65), (1, 67)], ids=str)
def test_edge_metric_sums(hip, hw):
    """Counts exactly; the two fp64 sums within test_gpu_edges._close's counted-roundings bound."""
    rng = np.random.default_rng(13)
    pe, ge = (rng.random(hw) < 0.05).astype(np.uint8), (rng.random(hw) < 0.05).astype(np.uint8)
    pe[0, 0] = ge[-1, -1] = 1
    ge[0, 0] = 0
    dt_, dp_ = E_REF.edt(ge), E_REF.edt(pe)
    valids = [np.zeros(hw, np.uint8), np.ones(hw, np.uint8), (rng.random(hw) < 0.6).astype(np.uint8)]
    B, th = len(valids), 10.0
    stack = lambda a: dev(np.stack([a] * B))      # noqa: E731
    args = (stack(pe), stack(ge), dev(np.stack(valids)), stack(dt_), stack(dp_))
    full = np.ones(hw, np.uint8)      # the busier call: every pixel an edge of both maps and valid, the distances large
    args_busy = (stack(full), stack(full), stack(full), stack(dt_ + 100.0), stack(dp_ + 100.0))
    need = hip.edge_sums_workspace_bytes(B, 4)

    def call(ws, a=args, th_acc=th):
        sums = poisoned((B, 4), torch.float64)
        hip.edge_metric_sums(*a, th_acc, sums, workspace=ws)
        return (sums,)
    sums, = three_states(hip, f"edge_metric_sums {hw}", need, call, lambda ws: call(ws, args_busy, 1e9))
    s = sums.cpu().numpy()
    for b, v in enumerate(valids):
        bde = (pe > 0) & (v > 0) & (dt_ < th)
        gsel = (ge > 0) & (v > 0)
        assert s[b, hip.EDGE_N_BDE] == bde.sum() and s[b, hip.EDGE_N_GT] == gsel.sum()
        assert T_EDGES._close(s[b, hip.EDGE_SUM_DT], math.fsum(dt_[bde]), max(int(bde.sum()), 1))
        assert T_EDGES._close(s[b, hip.EDGE_SUM_DP], math.fsum(dp_[gsel]), max(int(gsel.sum()), 1))


@pytest.mark.parametrize("hw", [(33, 41), (65, 65), (5, 2)], ids=str)
def test_soft_edge(hip, hw):
    rng = np.random.default_rng(17)
    pred, gt = rng.uniform(0.05, 1.0, hw).astype(np.float32), rng.uniform(0.05, 1.0, hw).astype(np.float32)
    valids = [np.zeros(hw, np.uint8), np.ones(hw, np.uint8), (rng.random(hw) < 0.6).astype(np.uint8)]
    B, radius = len(valids), 1
    stack = lambda a: dev(np.stack([a] * B))      # noqa: E731
    args = (stack(pred), stack(gt), dev(np.stack(valids)))
    args_busy = (stack(pred + 50.0), stack(gt), None)      # every pixel valid, every term large
    need = hip.edge_sums_workspace_bytes(B, 2)

    def call(ws, a=args):
        sums = poisoned((B, 2), torch.float64)
        hip.soft_edge(*a, radius, sums, workspace=ws)
        return (sums,)
    sums, = three_states(hip, f"soft_edge {hw}", need, call, lambda ws: call(ws, args_busy))
    s = sums.cpu().numpy()
    for b, v in enumerate(valids):
        see, _ = E_REF.soft_edge_error(pred, gt, v, radius)
        n = int(v.sum())
        assert s[b, 0] == n
        assert T_EDGES._close(s[b, 1], math.fsum(see[v > 0].astype(np.float64)), max(n, 1))


# ---- extreme_filter_fwd (64-wide tiles, 16-row column tiles): a key and a one-byte count per pixel ---------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("shape", [(1, 71, 131), (3, 9, 70), (1, 17, 65), (1, 1, 7), (1, 7, 1)], ids=str)
def test_extreme_filter(hip, shape, dtype):
    B, h, w = shape
    fill = -3.0 if dtype == np.float32 else 0
    x, v = T_FILT.make_map(shape, dtype, 13), T_FILT.make_valid("random", shape, 13)
    x_busy = T_FILT.make_map(shape, dtype, 14)
    dx, dv, db = dev(x), dev(v), dev(x_busy)
    need = hip.extreme_filter_workspace_bytes(B, h, w)
    assert need == 5 * B * h * w
    for size, rank, border in (((3, 9), "max", "mirror"), (3, "min", "ignore")):
        kh, kw = F_REF.window(size)
        code = {"min": hip.RANK_MIN, "max": hip.RANK_MAX}[rank]
        bcode = {"mirror": hip.BORDER_MIRROR, "ignore": hip.BORDER_IGNORE}[border]

        def call(ws, data=dx, valid=dv):
            out, count = poisoned(shape, torch.from_numpy(x).dtype), poisoned(shape, torch.int32)
            hip.extreme_filter_fwd(data, kh, kw, code, bcode, out, valid=valid, fill=fill, count=count, workspace=ws)
            return out, count
        out, count = three_states(hip, f"extreme_filter_fwd {shape} {size} {rank} {border}", need, call, lambda ws: call(ws, db, None))      # busier: every sample votes
        lo, hi, n = F_REF.extremes(x, size, border, v)
        with np.errstate(invalid="ignore"):
            want = np.where(n > 0, lo if rank == "min" else hi, fill).astype(dtype)
        T_FILT._assert_same(out.cpu().numpy(), count.cpu().numpy(), want, n, fill, f"{shape} {size} {rank} {border}")


# ---- pil_resize_u8: tmp holds the horizontal pass, batch * hi * wo * channels bytes -------------------------------------------------------------

@pytest.mark.parametrize("case", [((1, 45, 61, 3), (28, 14)), ((2, 70, 33, 1), (28, 28)), ((1, 64, 1, 1), (14, 28)), ((1, 1, 64, 3), (28, 14))], ids=str)
def test_pil_resize_tmp(hip, case):
    from hip_ext.labels import _device_tables
    (K, h, w, c), (ho, wo) = case
    if c == 3:
        imgs = np.stack([T_PIL._pixels(h, w, c=3, seed=h * 5 + w + k) for k in range(K)])
    else:
        imgs = T_PIL._masks(h, w) if (K == 2 and min(h, w) > 2) else np.stack([T_PIL._pixels(h, w, c=1, seed=h * 5 + w + k) for k in range(K)])
    src, src_busy = dev(imgs), dev(np.full_like(imgs, 255))
    tx, ty = _device_tables(w, wo, src.device), _device_tables(h, ho, src.device)
    need = K * h * wo * c

    def call(tmp, s=src):
        out_u8 = poisoned((K, ho, wo, c), torch.uint8)
        hip.pil_resize_u8(s, K, h, w, c, w * c, h * w * c, ho, wo, hip.PIL_BICUBIC, tx, ty, tmp, out_u8=out_u8)
        return (out_u8,)
    out, = three_states(hip, f"pil_resize_u8 {case}", need, call, lambda tmp: call(tmp, src_busy))
    for k in range(K):
        want = P_REF.resize_bicubic_u8(imgs[k], (ho, wo))
        assert np.array_equal(out[k].cpu().numpy().reshape(want.shape), want), k
