"""Writes tests/golden/geometry/cases.npz with the reference's own functions.

    python tools/make_geometry_golden.py [--reference /path/to/the/reference/checkout]

The reference's src/models/amodalsynthdrive/zoedepth/utils/geometry.py (numpy only) is imported from its file and run on seeded inputs.  Only arrays are
stored: the inputs, the arguments and what the reference returned.  Runs where a reference checkout exists; the tests read the file.

  <name>_depth / _mask / _points / _tri / _tri_all   for 1x1, 1x7, 7x1, 2x2, 5x3 and 37x61: an fp32 depth map, a uint8 mask, depth_to_points(depth[None])
      (float64 [h, w, 3], default pose), create_triangles(h, w, mask) and create_triangles(h, w) (int64).  For h == 1 or w == 1 the reference raises
      IndexError with a mask; _tri is then its unmasked, empty list and <name>_mask_raises is 1.
  pose<i>_R / _t / _points   for 5x3 and 37x61 (the depth maps above): a random orthonormal R, a t, and depth_to_points(depth[None], R, t)
  inv_depth / inv_ab / inv_points   an fp32 map v in [0, 1], (a, b), and the reference applied to the float64 map 1 / (a v + b): what "inverse mode" means
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (37, 61)]


def load_geometry(reference):
    path = os.path.join(reference, "src", "models", "amodalsynthdrive", "zoedepth", "utils", "geometry.py")
    spec = importlib.util.spec_from_file_location("reference_geometry", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from oracle._refshim import REFERENCE_ROOT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REFERENCE_ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "geometry", "cases.npz"))
    a = ap.parse_args()
    G = load_geometry(a.reference)
    rng = np.random.default_rng(20261020)
    out = {"shapes": np.array(SHAPES, dtype=np.int64)}
    depths = {}
    for h, w in SHAPES:
        name = f"{h}x{w}"
        depth = rng.uniform(0.5, 20.0, size=(h, w)).astype(np.float32)
        mask = (rng.random((h, w)) < 0.7).astype(np.uint8)
        if h * w <= 4:
            mask[:] = 1
        depths[name] = depth
        out[name + "_depth"], out[name + "_mask"] = depth, mask
        out[name + "_points"] = G.depth_to_points(depth[None])
        out[name + "_tri_all"] = G.create_triangles(h, w)
        try:
            out[name + "_tri"] = G.create_triangles(h, w, mask)
            out[name + "_mask_raises"] = np.int64(0)
        except IndexError:
            out[name + "_tri"] = G.create_triangles(h, w)
            out[name + "_mask_raises"] = np.int64(1)
        assert out[name + "_points"].dtype == np.float64 and out[name + "_points"].shape == (h, w, 3)
    for i, name in enumerate(("5x3", "37x61")):
        R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        t = rng.uniform(-3.0, 3.0, size=3)
        out[f"pose{i}_shape"] = np.array([int(v) for v in name.split("x")], dtype=np.int64)
        out[f"pose{i}_R"], out[f"pose{i}_t"] = R, t
        out[f"pose{i}_points"] = G.depth_to_points(depths[name][None], R, t)
    v = rng.random((37, 61)).astype(np.float32)
    v[3, 4], v[20, 50] = 0.0, 1.0
    ab = np.array([1.0 / 1.0 - 1.0 / 10.0, 1.0 / 10.0])
    out["inv_depth"], out["inv_ab"] = v, ab
    out["inv_points"] = G.depth_to_points((1.0 / (ab[0] * v.astype(np.float64) + ab[1]))[None])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
