"""CPU: the numpy restatement of the depth-to-geometry stage (tests/_geometry_ref.py) against goldens written from the real reference
(tests/golden/geometry/cases.npz, tools/make_geometry_golden.py), and everything of hip_ext.geometry that needs no device: the ABI surface, the
argument checks, the PLY writer and the command line."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

import _geometry_ref as R
import hip_ext
from hip_ext import geometry as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "geometry", "cases.npz"))
SHAPES = [tuple(int(v) for v in s) for s in GOLDEN["shapes"]]
NEW_EXPORTS = ("ada_depth_points_fwd", "ada_mesh_triangles_fwd", "ada_mesh_compact_fwd")


def test_golden_holds_the_six_shapes():
    assert SHAPES == [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (37, 61)]


@pytest.mark.parametrize("hw", SHAPES)
def test_default_pose_points_equal_the_reference_bit_for_bit(hw):
    name = "%dx%d" % hw
    ours = R.points(GOLDEN[name + "_depth"])
    assert ours.dtype == np.float64 and ours.shape == hw + (3,)
    assert np.array_equal(ours, GOLDEN[name + "_points"])
    assert np.array_equal(G.get_intrinsics(*hw), R.intrinsics(*hw))


@pytest.mark.parametrize("hw", SHAPES)
def test_triangles_equal_the_reference_order_included(hw):
    name = "%dx%d" % hw
    h, w = hw
    assert np.array_equal(R.triangles(h, w).astype(np.int64), GOLDEN[name + "_tri_all"].astype(np.int64))
    masked = R.triangles(h, w, GOLDEN[name + "_mask"])
    assert masked.dtype == np.int32 and masked.shape[1] == 3
    # a grid one pixel wide: the reference raises with a mask; zero triangles here, which is its unmasked answer
    assert int(GOLDEN[name + "_mask_raises"]) == (1 if min(hw) == 1 else 0)
    assert np.array_equal(masked.astype(np.int64), GOLDEN[name + "_tri"].astype(np.int64))


def test_create_triangles_2x3_is_the_documented_list():
    assert R.triangles(2, 3).tolist() == [[0, 3, 1], [4, 1, 3], [1, 4, 2], [5, 2, 4]]


@pytest.mark.parametrize("i", [0, 1])
def test_general_pose_within_the_derived_bound(i):
    h, w = (int(v) for v in GOLDEN[f"pose{i}_shape"])
    depth, Rm, t = GOLDEN[f"{h}x{w}_depth"], GOLDEN[f"pose{i}_R"], GOLDEN[f"pose{i}_t"]
    ours, ref = R.points(depth, Rm, t), GOLDEN[f"pose{i}_points"]
    bound = R.pose_bound(depth, Rm, t)
    assert bound.shape == ref.shape and (bound > 0).all() and bound.max() < 1e-12
    assert (np.abs(ours - ref) <= bound).all(), float((np.abs(ours - ref) / bound).max())


def test_inverse_mode_is_the_reference_applied_to_the_converted_map():
    a, b = GOLDEN["inv_ab"]
    assert np.array_equal(R.points(GOLDEN["inv_depth"], inverse=(a, b)), GOLDEN["inv_points"])


def test_validity_ratio_and_nan_rules_of_the_restatement():
    d = np.array([[1, 2, 0], [np.inf, 2, 3], [np.nan, 4, 4.000001]], np.float32)
    z = R.z_of(d)
    assert R.valid_of(z).tolist() == [[True, True, False], [False, True, True], [False, True, True]]
    p = R.points(d)
    assert np.isnan(p[1, 0]).all() and np.isnan(p[2, 0]).all() and np.isfinite(p[0, 2]).all() and np.isfinite(R.points(-d)[1, 2]).all()
    assert R.triangles(3, 3, depth=d).tolist() == [[4, 7, 5], [8, 5, 7]]
    e = np.array([[1, 2], [2, 4]], np.float32)
    assert R.triangles(2, 2, depth=e, max_ratio=2.0).tolist() == [[0, 2, 1], [3, 1, 2]]      # z_max == max_ratio z_min is kept
    assert R.triangles(2, 2, depth=e, max_ratio=1.9999).tolist() == []
    inv = R.z_of(np.array([[0.0, 1.0]], np.float32), inverse=(1.0, 0.0))
    assert np.isinf(inv[0, 0]) and inv[0, 1] == 1.0 and R.valid_of(inv).tolist() == [[False, True]]


def test_compaction_restatement():
    tri = np.array([[4, 7, 5], [8, 5, 7]], np.int32)
    pts = np.arange(27, dtype=np.float64).reshape(9, 3)
    p, t, n, c = R.compact(tri, pts, np.arange(27, dtype=np.uint8).reshape(9, 3))
    assert n == 4 and t.tolist() == [[0, 2, 1], [3, 1, 2]] and np.array_equal(p, pts[[4, 5, 7, 8]]) and c[:, 0].tolist() == [12, 15, 21, 24]
    assert R.compact(np.zeros((0, 3), np.int32), pts)[2] == 0


def test_new_exports_constants_and_build_lists():
    header = open(os.path.join(ROOT, "include", "ada_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in hip_ext.EXPORTS
        assert hasattr(hip_ext.load(), name)
    assert hip_ext.ABI_VERSION == 10 and re.search(r"#define\s+ADA_ABI_VERSION\s+10\b", header)
    for c in ("GEOM_WAVE", "GEOM_CHUNK", "GEOM_SCAN_BLOCK"):
        assert int(re.search(r"#define\s+ADA_%s\s+(\d+)" % c, header).group(1)) == getattr(hip_ext, c)
    import importlib.util
    spec = importlib.util.spec_from_file_location("ada_csrc_build_geometry", os.path.join(ROOT, "amodal-depth-anything_amd", "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "ada_geometry.hip" in build.SOURCES and "ada_geometry.hip" in build.NO_SCRATCH
    assert "-ffp-contract=off" in build.PER_FILE_FLAGS["ada_geometry.hip"]
    assert hip_ext.mesh_triangles_workspace_bytes(3, 1, 9) == 12 and hip_ext.mesh_triangles_workspace_bytes(1, 2, 1026) == 8
    assert hip_ext.mesh_compact_workspace_bytes(2, 32, 33) == 8 * (32 * 33 + 2)


def _read_ply(path):
    """A reader for what write_ply writes: (points, triangles or None, colours or None)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    faces = [ln for ln in lines if ln.startswith("element face")]
    props = [ln.split()[1:] for ln in lines if ln.startswith("property") and "list" not in ln]
    kinds = {"float": "<f4", "double": "<f8", "uchar": "u1"}
    vdt = np.dtype([(name, kinds[kind]) for kind, name in props])
    vert = np.frombuffer(raw, dtype=vdt, count=nv, offset=end)
    pts = np.stack([vert["x"], vert["y"], vert["z"]], 1)
    col = np.stack([vert["red"], vert["green"], vert["blue"]], 1) if "red" in vdt.names else None
    tri = None
    off = end + nv * vdt.itemsize
    if faces:
        assert "property list uchar int vertex_indices" in lines
        nf = int(faces[0].split()[2])
        tri = np.zeros((nf, 3), np.int32)
        for i in range(nf):
            n, a, b, c = struct.unpack_from("<Biii", raw, off + 13 * i)
            assert n == 3
            tri[i] = a, b, c
        off += 13 * nf
    assert off == len(raw)
    return pts, tri, col


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_write_ply_round_trip(tmp_path, dtype):
    rng = np.random.default_rng(5)
    pts = rng.standard_normal((7, 3)).astype(dtype)
    tri = rng.integers(0, 7, size=(5, 3)).astype(np.int32)
    col = rng.integers(0, 256, size=(7, 3)).astype(np.uint8)
    G.write_ply(str(tmp_path / "a.ply"), G.Mesh(torch.from_numpy(pts), torch.from_numpy(tri), 7, 5, torch.from_numpy(col)))
    p, t, c = _read_ply(tmp_path / "a.ply")
    assert p.dtype == dtype and np.array_equal(p, pts) and np.array_equal(t, tri) and np.array_equal(c, col)
    G.write_ply(str(tmp_path / "b.ply"), pts)
    p, t, c = _read_ply(tmp_path / "b.ply")
    assert np.array_equal(p, pts) and t is None and c is None
    G.write_ply(str(tmp_path / "c.ply"), pts[:0], np.zeros((0, 3), np.int32))
    p, t, c = _read_ply(tmp_path / "c.ply")
    assert p.shape == (0, 3) and t.shape == (0, 3)
    with pytest.raises(ValueError, match="not there"):
        G.write_ply(str(tmp_path / "d.ply"), pts, np.array([[0, 1, 7]], np.int32))
    with pytest.raises(ValueError):
        G.write_ply(str(tmp_path / "d.ply"), pts.astype(np.float16))


def test_argument_errors_need_no_device():
    d = np.ones((4, 5), np.float32)
    for bad in (np.ones(5, np.float32), np.ones((1, 2, 3, 4), np.float32), np.ones((0, 5), np.float32)):
        with pytest.raises(ValueError, match="depth must be"):
            G.depth_to_points(bad)
    with pytest.raises(TypeError, match="float32"):
        G.depth_to_points(d.astype(np.float64))
    with pytest.raises(TypeError):
        G.depth_to_points([[1.0]])
    with pytest.raises(ValueError, match="dtype"):
        G.depth_to_points(d, dtype=torch.float16)
    with pytest.raises(ValueError, match="3 x 3"):
        G.depth_to_points(d, R=np.eye(4))
    with pytest.raises(ValueError, match="inverse"):
        G.depth_to_points(d, inverse=1.0)
    with pytest.raises(ValueError, match="capacity"):
        G.create_triangles(4, 5, capacity=-1)
    with pytest.raises(ValueError, match="2\\^30"):
        G.create_triangles(2 ** 15, 2 ** 15)
    with pytest.raises(ValueError, match="positive"):
        G.create_triangles(0, 5)
    with pytest.raises(ValueError, match="mask of shape"):
        G.create_triangles(4, 5, mask=np.ones((5, 4), np.uint8))
    with pytest.raises(TypeError, match="uint8 or bool"):
        G.create_triangles(4, 5, mask=np.ones((4, 5), np.float32))
    with pytest.raises(ValueError, match="differ in shape"):
        G.create_triangles(4, 5, mask=np.ones((2, 4, 5), np.uint8), depth=np.ones((3, 4, 5), np.float32))
    with pytest.raises(ValueError, match="max_ratio needs"):
        G.create_triangles(4, 5, max_ratio=2.0)
    with pytest.raises(ValueError, match="one map"):
        G.depth_to_mesh(np.ones((2, 4, 5), np.float32))
    # CPU tensors and a CPU target: no fallback
    with pytest.raises(hip_ext.HipExtError, match="no CPU fallback"):
        G.depth_to_points(torch.ones(4, 5))
    with pytest.raises(hip_ext.HipExtError, match="no CPU fallback"):
        G.create_triangles(4, 5, mask=torch.ones(4, 5, dtype=torch.uint8))
    with pytest.raises(hip_ext.HipExtError, match="no CPU fallback"):
        G.depth_to_mesh(d, device="cpu")
    with pytest.raises(hip_ext.HipExtError, match="no CPU fallback"):
        hip_ext.depth_points(torch.ones(1, 4, 5), [0.0] * 21, out_f64=torch.empty(1, 4, 5, 3, dtype=torch.float64))
    from hip_ext.pipeline import AmodalResult
    cpu = AmodalResult(torch.zeros(4, 5), None, torch.zeros(1, 4, 5), torch.zeros(1, 4, 5), None)
    with pytest.raises(hip_ext.HipExtError, match="no CPU fallback"):
        G.amodal_layers(cpu)


def test_library_rejects_bad_arguments_without_a_device():
    """The C entry points check their arguments before any launch: ADA_EINVAL needs no GPU."""
    lib = hip_ext.load()
    cam = (ctypes.c_double * 21)(*([0.0] * 21))
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    assert lib.ada_depth_points_fwd(p, 1, 2 ** 15, 2 ** 15, cam, 0, 0.0, 0.0, p, None, None, None) != 0
    assert b"2^30" in lib.ada_last_error()
    assert lib.ada_depth_points_fwd(p, 65536, 2, 2, cam, 0, 0.0, 0.0, p, None, None, None) != 0
    assert lib.ada_depth_points_fwd(p, 1, 2, 2, cam, 0, 0.0, 0.0, None, None, None, None) != 0
    assert lib.ada_mesh_triangles_fwd(None, 0, 0, None, 0, 0.0, 0.0, 0.0, 1, 2 ** 15, 2 ** 15, p, 4, p, p, 1 << 20, None) != 0
    assert lib.ada_mesh_triangles_fwd(None, 0, 0, None, 0, 0.0, 0.0, 0.0, 1, 4, 5, p, -1, p, p, 1 << 20, None) != 0
    assert lib.ada_mesh_triangles_fwd(None, 0, 0, None, 0, 0.0, 0.0, 2.0, 1, 4, 5, p, 4, p, p, 1 << 20, None) != 0
    assert b"max_ratio" in lib.ada_last_error()
    assert lib.ada_mesh_triangles_fwd(p, 4, 0, None, 0, 0.0, 0.0, 0.0, 1, 4, 5, p, 4, p, p, 1 << 20, None) != 0      # pitch below w
    assert lib.ada_mesh_triangles_fwd(None, 0, 0, None, 0, 0.0, 0.0, 0.0, 1, 40, 50, p, 4, p, p, 4, None) != 0       # workspace too small
    assert b"workspace" in lib.ada_last_error()
    assert lib.ada_mesh_compact_fwd(p, p, 4, 1, 4, 5, p, 2, None, p, None, 4, p, p, 1 << 20, None) != 0               # point_bytes
    assert lib.ada_mesh_compact_fwd(p, p, 4, 1, 4, 5, p, 8, None, p, None, 4, p, p, 16, None) != 0
    assert b"workspace" in lib.ada_last_error()


def test_depth_to_mesh_command_line(tmp_path, monkeypatch):
    """The script end to end, with hip_ext.geometry.depth_to_mesh replaced by the restatement (the PLY writer is the real one)."""
    from PIL import Image

    from src.scripts import depth_to_mesh as S
    rng = np.random.default_rng(11)
    v = rng.integers(0, 65536, size=(9, 12)).astype(np.uint16)
    v[2, 3] = 0
    mask = np.zeros((9, 12), np.uint8)
    mask[1:8, 2:11] = 255
    Image.fromarray(v).save(tmp_path / "d.png")
    Image.fromarray(mask).save(tmp_path / "m.png")
    calls = []

    def fake(depth, mask=None, colors=None, compact=True, inverse=None, max_ratio=None, fov_deg=55.0, device=None, **kw):
        calls.append(dict(inverse=inverse, max_ratio=max_ratio, fov_deg=fov_deg, device=device))
        return G.Mesh(*R.depth_to_mesh(depth, mask, colors, compact, inverse, max_ratio, fov_deg))

    monkeypatch.setattr(G, "depth_to_mesh", fake)
    out = tmp_path / "sub" / "o.ply"
    assert S.main([str(tmp_path / "d.png"), str(out), "--mask", str(tmp_path / "m.png"), "--inverse", "1", "10", "--max_ratio", "1.5", "--fov", "60"]) == 0
    assert calls == [dict(inverse=(1.0 / 1.0 - 1.0 / 10.0, 1.0 / 10.0), max_ratio=1.5, fov_deg=60.0, device="cuda")]
    depth = (v.astype(np.float64) / 65535.0).astype(np.float32)
    want = R.depth_to_mesh(depth, mask > 0, inverse=calls[0]["inverse"], max_ratio=1.5, fov_deg=60.0)
    p, t, c = _read_ply(out)
    assert want.triangle_count > 0 and want.vertex_count < 9 * 12
    assert np.array_equal(p, want.points) and np.array_equal(t, want.triangles) and c is None
    # a .npy map is taken as stored, and without --inverse as depth
    np.save(tmp_path / "z.npy", depth + 1)
    assert S.main([str(tmp_path / "z.npy"), str(tmp_path / "z.ply")]) == 0
    assert calls[1] == dict(inverse=None, max_ratio=None, fov_deg=55.0, device="cuda")
    p, t, c = _read_ply(tmp_path / "z.ply")
    want = R.depth_to_mesh(depth + 1)
    assert np.array_equal(p, want.points) and np.array_equal(t, want.triangles)
    with pytest.raises(ValueError, match="NEAR < FAR"):
        S.main([str(tmp_path / "z.npy"), str(tmp_path / "z.ply"), "--inverse", "5", "2"])
