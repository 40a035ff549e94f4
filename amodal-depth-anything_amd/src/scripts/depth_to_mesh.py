#!/usr/bin/env python
"""A depth map in, a triangle mesh out: the reference's ``zoedepth/utils/geometry.py`` (depth_to_points, create_triangles) as a command line.

    python -m src.scripts.depth_to_mesh DEPTH OUTPUT.ply [--mask MASK.png] [--inverse NEAR FAR] [--max_ratio R] [--fov 55] [--image PHOTO]
                                                        [--max_error E] [--median K]

DEPTH is a 16-bit (or 8-bit) one-channel PNG / TIFF read with Pillow, or a ``.npy`` float array.  Without ``--inverse`` its values are depths, as the
reference takes them.  With ``--inverse NEAR FAR`` they are normalised inverse depth -- what this project's networks and its 16-bit pseudo-labels hold:
an integer image is first divided by its type's largest value, and v in [0, 1] becomes z = 1 / (v (1 / NEAR - 1 / FAR) + 1 / FAR).  The unprojection,
the triangle selection (inside MASK, valid depth, and with ``--max_ratio`` no triangle whose farthest vertex is more than R times its nearest) and the
vertex compaction run on the device (hip_ext.geometry); the PLY is written on the host.  ``--max_error E`` writes an adaptive mesh in place of two
triangles per pixel cell: conforming right triangles refined until the relative disparity error at every split point is at most E
(hip_ext.geometry.adaptive_triangles) -- 0.01 keeps a few per cent of the triangles of a smooth map.  ``--median K`` first replaces the depth inside
the mask by its K x K median among the mask's own samples (hip_ext.filters.median_filter, on the device): the flying pixels of an occlusion border
otherwise stand as spikes.
"""
import argparse
import os
import sys

import numpy as np
from PIL import Image

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from hip_ext import geometry  # noqa: E402

__all__ = ["read_depth", "read_mask", "mesh_file", "main"]


def read_depth(path, normalise=False) -> np.ndarray:
    """One depth map as fp32 [H, W].  ``normalise``: an integer image is divided by the largest value of its type (in float64, rounded once)."""
    arr = np.load(path) if path.lower().endswith(".npy") else np.asarray(Image.open(path))
    arr = np.squeeze(arr)
    if arr.ndim != 2:
        raise ValueError(f"{path}: expected a one-channel depth map, got shape {arr.shape}")
    if normalise and arr.dtype.kind in "iu":
        arr = arr.astype(np.float64) / float(np.iinfo(arr.dtype).max)
    return np.ascontiguousarray(arr.astype(np.float32))


def read_mask(path, shape) -> np.ndarray:
    m = np.asarray(Image.open(path))
    if m.ndim == 3:
        m = m.max(axis=2)
    if m.shape != tuple(shape):
        raise ValueError(f"{path}: mask of shape {m.shape} for a depth map of shape {tuple(shape)}")
    return np.ascontiguousarray((m > 0).astype(np.uint8))


def mesh_file(src, dst, mask=None, inverse=None, max_ratio=None, fov=55.0, image=None, device="cuda", max_error=None, median=None):
    """Meshes one file; returns the hip_ext.geometry.Mesh that was written."""
    depth = read_depth(src, normalise=inverse is not None)
    ab = None
    if inverse is not None:
        near, far = inverse
        if not (near > 0 and far > near):
            raise ValueError(f"--inverse: 0 < NEAR < FAR expected, got {near} {far}")
        ab = (1.0 / near - 1.0 / far, 1.0 / far)
    colors = None
    if image is not None:
        colors = np.ascontiguousarray(np.asarray(Image.open(image).convert("RGB")))
        if colors.shape[:2] != depth.shape:
            raise ValueError(f"{image}: photo of shape {colors.shape[:2]} for a depth map of shape {depth.shape}")
    mesh = geometry.depth_to_mesh(depth, mask=None if mask is None else read_mask(mask, depth.shape), colors=colors, fov_deg=fov, inverse=ab,
                                  max_ratio=max_ratio, max_error=max_error, median=median, device=device)
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    geometry.write_ply(dst, mesh)
    return mesh


def main(argv=None):
    ap = argparse.ArgumentParser(description="Turn a depth map into a triangle mesh (on the HIP device) and write it as a binary PLY")
    ap.add_argument("input", help="a depth file (.png / .tif 8- or 16-bit, .npy float)")
    ap.add_argument("output", help="output .ply")
    ap.add_argument("--mask", default=None, help="a mask image of the depth map's size: only vertices where it is non-zero are meshed")
    ap.add_argument("--inverse", type=float, nargs=2, metavar=("NEAR", "FAR"), default=None, help="the input is normalised inverse depth: 1 lies at NEAR, 0 at FAR")
    ap.add_argument("--max_ratio", type=float, default=None, help="drop triangles whose farthest vertex is more than this many times their nearest")
    ap.add_argument("--fov", type=float, default=55.0, help="field of view of the pinhole camera in degrees")
    ap.add_argument("--image", default=None, help="a photo of the depth map's size for the vertex colours")
    ap.add_argument("--max_error", type=float, default=None, help="adaptive mesh: the largest relative disparity error of a triangle that is not split (default: two triangles per cell)")
    ap.add_argument("--median", type=int, default=None, metavar="K", help="median-filter the depth over K x K windows (K odd) among the samples inside the mask before meshing: removes the flying pixels of occlusion borders")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    mesh = mesh_file(args.input, args.output, args.mask, args.inverse, args.max_ratio, args.fov, args.image, args.device, args.max_error, args.median)
    print(f"{args.output}: {mesh.vertex_count} vertices, {mesh.triangle_count} triangles")
    return 0


if __name__ == "__main__":
    sys.exit(main())
