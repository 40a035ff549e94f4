#!/usr/bin/env python
"""A depth map in, a picture of its mesh from a moved camera out: depth_to_mesh's geometry looked at through hip_ext.geometry.render_mesh.

    python -m src.scripts.depth_to_view DEPTH OUT.png [--mask MASK.png] [--inverse NEAR FAR] [--max_ratio R] [--fov 55] [--image PHOTO]
                                                     [--yaw D] [--pitch D] [--shift X Y Z] [--size H W] [--max_error E] [--median K]
                                                     [--fill_holes {nearest,smooth,harmonic}] [--guided R EPS]

DEPTH, ``--mask``, ``--inverse``, ``--max_ratio``, ``--max_error``, ``--median``, ``--guided`` and ``--image`` are read as ``src.scripts.depth_to_mesh`` reads them.  The camera orbits by
``--yaw`` / ``--pitch`` degrees about the point on the optical axis at the map's median depth and then moves by ``--shift``
(hip_ext.geometry.look_at_pose).  With ``--image`` the output is the photo-coloured view; without it, the view's depth through the colour map of
hip_ext.image.colorize over the inverse depth (holes and background in its background grey).  ``--size`` renders at another size than the map's, with the same field
of view.  ``--fill_holes`` gives the pixels no triangle covered a value from the covered ones before the picture is coloured
(hip_ext.geometry.fill_view: ``smooth`` is the push-pull fill, ``nearest`` copies the nearest covered pixel); without it they keep the background.  Mesh,
rasteriser, fill and colour map run on the device; only the uint8 picture crosses to the host.
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
from src.scripts.depth_to_mesh import guided_depth, read_depth, read_mask, read_photo  # noqa: E402

INVALID = -99.0      # colorize's marker of a pixel without a value: the view's background and holes

__all__ = ["build_parser", "inverse_pair", "pivot_depth", "view_file", "main"]


def inverse_pair(inverse):
    """--inverse NEAR FAR -> (a, b) of z = 1 / (a v + b), or None."""
    if inverse is None:
        return None
    near, far = inverse
    if not (near > 0 and far > near):
        raise ValueError(f"--inverse: 0 < NEAR < FAR expected, got {near} {far}")
    return (1.0 / near - 1.0 / far, 1.0 / far)


def pivot_depth(depth, ab=None) -> float:
    """The median metric depth of the map's valid pixels (host side, from the file that was just read): where the camera's orbit is centred."""
    z = depth.astype(np.float64)
    if ab is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            z = 1.0 / (ab[0] * z + ab[1])
    z = z[np.isfinite(z) & (z > 0)]
    return float(np.median(z)) if z.size else 1.0


def view_file(src, dst, mask=None, inverse=None, max_ratio=None, fov=55.0, image=None, yaw=0.0, pitch=0.0, shift=(0.0, 0.0, 0.0), size=None,
              device="cuda", max_error=None, median=None, fill_holes=None, guided=None):
    """Renders one file; returns the uint8 picture [H, W, 3] (R, G, B) that was written."""
    from hip_ext import image as hip_image
    if guided is not None and image is None:
        raise ValueError("--guided needs --image: the photo is the guide")
    ab = inverse_pair(inverse)
    depth = read_depth(src, normalise=ab is not None)
    colors = None if image is None else read_photo(image, depth.shape, guided)
    mask = None if mask is None else read_mask(mask, depth.shape)
    pivot = pivot_depth(depth, ab)      # from the file that was read: the guided depth stays on the device
    if guided is not None:
        depth, mask = guided_depth(depth, mask, colors, guided, device)
    h, w = tuple(depth.shape) if size is None else (int(size[0]), int(size[1]))
    mesh = geometry.depth_to_mesh(depth, mask=mask, colors=colors, fov_deg=fov, inverse=ab,
                                  max_ratio=max_ratio, max_error=max_error, median=median, device=device)
    R, t = geometry.look_at_pose(yaw, pitch, shift, pivot_z=pivot)
    view = geometry.render_mesh(mesh, h, w, fov_deg=fov, R=R, t=t, out="w", fill=INVALID, device=device)
    if fill_holes is not None:
        view = geometry.fill_view(view, fill_holes)
    if view.color is not None:
        picture = view.color.cpu().numpy()
    else:
        picture = hip_image.colorize(view.depth, invalid_val=INVALID)[0, :, :, :3].cpu().numpy()      # R, G, B, A on the device
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(picture)).save(dst)
    return picture


def build_parser():
    ap = argparse.ArgumentParser(description="Render a depth map's mesh from a moved camera (on the HIP device) and write the picture")
    ap.add_argument("input", help="a depth file (.png / .tif 8- or 16-bit, .npy float)")
    ap.add_argument("output", help="output picture (.png)")
    ap.add_argument("--mask", default=None, help="a mask image of the depth map's size: only vertices where it is non-zero are meshed")
    ap.add_argument("--inverse", type=float, nargs=2, metavar=("NEAR", "FAR"), default=None, help="the input is normalised inverse depth: 1 lies at NEAR, 0 at FAR")
    ap.add_argument("--max_ratio", type=float, default=None, help="drop triangles whose farthest vertex is more than this many times their nearest")
    ap.add_argument("--fov", type=float, default=55.0, help="field of view of the pinhole camera in degrees")
    ap.add_argument("--image", default=None, help="a photo of the depth map's size for the vertex colours")
    ap.add_argument("--yaw", type=float, default=0.0, help="degrees about the vertical axis through the pivot")
    ap.add_argument("--pitch", type=float, default=0.0, help="degrees about the horizontal axis through the pivot")
    ap.add_argument("--shift", type=float, nargs=3, metavar=("X", "Y", "Z"), default=(0.0, 0.0, 0.0), help="translation added after the orbit (x left, y up, z forward)")
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), default=None, help="target size (default: the depth map's)")
    ap.add_argument("--max_error", type=float, default=None, help="adaptive mesh: the largest relative disparity error of a triangle that is not split (default: two triangles per cell)")
    ap.add_argument("--median", type=int, default=None, metavar="K", help="median-filter the depth over K x K windows (K odd) among the samples inside the mask before meshing: removes the flying pixels of occlusion borders")
    ap.add_argument("--fill_holes", choices=("nearest", "smooth", "harmonic"), default=None, help="fill the pixels no triangle covered from the covered ones: the nearest covered pixel's value, the smooth push-pull fill, or the harmonic fill of the membrane solve (default: they keep the background)")
    ap.add_argument("--guided", type=float, nargs=2, metavar=("R", "EPS"), default=None, help="guided filter of the depth with --image as guide, radius R (integer) and eps EPS in [0, 1]^2 units; a photo larger than the depth map up-samples the depth to its size")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    picture = view_file(args.input, args.output, args.mask, args.inverse, args.max_ratio, args.fov, args.image, args.yaw, args.pitch, tuple(args.shift),
                        args.size, args.device, args.max_error, args.median, args.fill_holes, args.guided)
    print(f"{args.output}: {picture.shape[0]} x {picture.shape[1]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
