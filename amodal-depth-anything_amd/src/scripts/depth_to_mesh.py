#!/usr/bin/env python
"""A depth map in, a triangle mesh out: the reference's ``zoedepth/utils/geometry.py`` (depth_to_points, create_triangles) as a command line.

    python -m src.scripts.depth_to_mesh DEPTH OUTPUT.ply [--mask MASK.png] [--inverse NEAR FAR] [--max_ratio R] [--fov 55] [--image PHOTO]
                                                        [--max_error E] [--median K] [--guided R EPS]

DEPTH is a 16-bit (or 8-bit) one-channel PNG / TIFF read with Pillow, or a ``.npy`` float array.  Without ``--inverse`` its values are depths, as the
reference takes them.  With ``--inverse NEAR FAR`` they are normalised inverse depth -- what this project's networks and its 16-bit pseudo-labels hold:
an integer image is first divided by its type's largest value, and v in [0, 1] becomes z = 1 / (v (1 / NEAR - 1 / FAR) + 1 / FAR).  The unprojection,
the triangle selection (inside MASK, valid depth, and with ``--max_ratio`` no triangle whose farthest vertex is more than R times its nearest) and the
vertex compaction run on the device (hip_ext.geometry); the PLY is written on the host.  ``--max_error E`` writes an adaptive mesh in place of two
triangles per pixel cell: conforming right triangles refined until the relative disparity error at every split point is at most E
(hip_ext.geometry.adaptive_triangles) -- 0.01 keeps a few per cent of the triangles of a smooth map.  ``--median K`` first replaces the depth inside
the mask by its K x K median among the mask's own samples (hip_ext.filters.median_filter, on the device): the flying pixels of an occlusion border
otherwise stand as spikes.  ``--guided R EPS`` (with ``--image``) first runs the guided filter over the depth with the photo as guide, radius R and
eps EPS in [0, 1]^2 units (hip_ext.guided, on the device): the depth's edges move to where the photo's lie.  The photo may then be LARGER than the
depth map: the depth is up-sampled to the photo's size (hip_ext.guided.guided_upsample), the mask follows by the nearest rule, and the mesh has one
vertex per photo pixel.  Without ``--guided`` a photo of another size is refused.
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

__all__ = ["read_depth", "read_mask", "read_photo", "guided_depth", "mesh_file", "build_parser", "main"]


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


def read_photo(path, shape, guided=None) -> np.ndarray:
    """The photo as uint8 [H, W, 3] (R, G, B).  It has the depth map's ``shape``; with ``guided`` it may be larger on both axes."""
    colors = np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB")))
    if guided is None and colors.shape[:2] != tuple(shape):
        raise ValueError(f"{path}: photo of shape {colors.shape[:2]} for a depth map of shape {tuple(shape)}")
    if guided is not None and (colors.shape[0] < shape[0] or colors.shape[1] < shape[1]):
        raise ValueError(f"{path}: --guided needs a photo at least as large as the depth map {tuple(shape)}, got {colors.shape[:2]}")
    return colors


def resize_mask_nearest(mask, shape) -> np.ndarray:
    """A mask at another size by the nearest rule of cv2.resize(INTER_NEAREST): output (Y, X) reads input (floor(Y h / H), floor(X w / W))."""
    h, w = mask.shape
    ys = np.minimum((np.arange(shape[0]) * h) // shape[0], h - 1)
    xs = np.minimum((np.arange(shape[1]) * w) // shape[1], w - 1)
    return np.ascontiguousarray(mask[ys][:, xs])


def guided_depth(depth, mask, colors, guided, device="cuda"):
    """--guided R EPS: (depth, mask) at the photo's size, the depth through hip_ext.guided.guided_upsample with the photo as guide (the plain guided
    filter for a photo of the depth's size) and the mask through the nearest rule.  The depth comes back as a device tensor."""
    from hip_ext.guided import guided_upsample
    radius, eps = guided
    if float(radius) != int(radius):
        raise ValueError(f"--guided: the radius R must be an integer, got {radius}")
    out = guided_upsample(depth, colors, int(radius), float(eps), device=device)
    if mask is not None and mask.shape != colors.shape[:2]:
        mask = resize_mask_nearest(mask, colors.shape[:2])
    return out, mask


def mesh_file(src, dst, mask=None, inverse=None, max_ratio=None, fov=55.0, image=None, device="cuda", max_error=None, median=None, guided=None):
    """Meshes one file; returns the hip_ext.geometry.Mesh that was written."""
    if guided is not None and image is None:
        raise ValueError("--guided needs --image: the photo is the guide")
    depth = read_depth(src, normalise=inverse is not None)
    ab = None
    if inverse is not None:
        near, far = inverse
        if not (near > 0 and far > near):
            raise ValueError(f"--inverse: 0 < NEAR < FAR expected, got {near} {far}")
        ab = (1.0 / near - 1.0 / far, 1.0 / far)
    colors = None if image is None else read_photo(image, depth.shape, guided)
    mask = None if mask is None else read_mask(mask, depth.shape)
    if guided is not None:
        depth, mask = guided_depth(depth, mask, colors, guided, device)
    mesh = geometry.depth_to_mesh(depth, mask=mask, colors=colors, fov_deg=fov, inverse=ab,
                                  max_ratio=max_ratio, max_error=max_error, median=median, device=device)
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    geometry.write_ply(dst, mesh)
    return mesh


def build_parser():
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
    ap.add_argument("--guided", type=float, nargs=2, metavar=("R", "EPS"), default=None, help="guided filter of the depth with --image as guide, radius R (integer) and eps EPS in [0, 1]^2 units; a photo larger than the depth map up-samples the depth to its size")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    mesh = mesh_file(args.input, args.output, args.mask, args.inverse, args.max_ratio, args.fov, args.image, args.device, args.max_error, args.median,
                     args.guided)
    print(f"{args.output}: {mesh.vertex_count} vertices, {mesh.triangle_count} triangles")
    return 0


if __name__ == "__main__":
    sys.exit(main())
