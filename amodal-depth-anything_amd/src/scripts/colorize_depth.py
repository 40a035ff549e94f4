#!/usr/bin/env python
"""Depth files in, coloured PNGs out: the reference's ``src/scripts/colorize_depth.py`` as a command line.

    python -m src.scripts.colorize_depth INPUT OUTPUT [--cmap turbo_r] [--vminp 2] [--vmaxp 95] [--invalid_val -99]

The reference's script is its ``colorize()`` plus a few lines with hard-coded paths that colour one file.  Here ``colorize`` is
``hip_ext.image.colorize`` -- the percentiles (ada_quantile_fwd), the colour map and the background colour on the device -- and the paths are arguments:
INPUT is a depth file or a folder of them (16-bit or 8-bit PNG / TIFF read with Pillow, ``.npy`` float arrays), OUTPUT a file or a folder.  As the
reference does (``cv2.imwrite(path, coloured[:, :, [2, 1, 0]])``), the alpha channel is dropped and the file holds what an OpenCV reader returns as B, G, R.
Integer depths up to 2^24 are exact in fp32, which is what the device takes.
"""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from hip_ext.image import colorize  # noqa: E402  (the function the reference's scripts define, on the device)

__all__ = ["colorize", "read_depth", "colorize_file", "main"]

EXTENSIONS = (".png", ".tif", ".tiff", ".npy")


def read_depth(path) -> np.ndarray:
    """One depth map as fp32 [H, W]: ``.npy`` as stored (singleton axes squeezed), images through Pillow (8- / 16- / 32-bit integer or float, one channel)."""
    if path.lower().endswith(".npy"):
        arr = np.load(path)
    else:
        arr = np.asarray(Image.open(path))
    arr = np.squeeze(arr)
    if arr.ndim != 2:
        raise ValueError(f"{path}: expected a one-channel depth map, got shape {arr.shape}")
    return np.ascontiguousarray(arr.astype(np.float32))


def colorize_file(src, dst, device="cuda", cmap="turbo_r", vminp=2, vmaxp=95, invalid_val=-99):
    """Colours one file; returns the uint8 [H, W, 3] R, G, B picture that was written (B, G, R to an OpenCV reader, as the reference writes it)."""
    depth = torch.from_numpy(read_depth(src)).to(device)
    rgba = colorize(depth, cmap=cmap, invalid_val=invalid_val, vminp=vminp, vmaxp=vmaxp)[0].cpu().numpy()
    rgb = np.ascontiguousarray(rgba[:, :, :3])
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    Image.fromarray(rgb).save(dst)      # Pillow stores R, G, B: cv2.imwrite of the flipped array stores the same bytes
    return rgb


def main(argv=None):
    ap = argparse.ArgumentParser(description="Colour depth maps between two percentiles of their valid pixels (on the HIP device)")
    ap.add_argument("input", help="a depth file (.png / .tif 8- or 16-bit, .npy float) or a folder of them")
    ap.add_argument("output", help="output .png, or a folder (created) when the input is a folder")
    ap.add_argument("--cmap", default="turbo_r", help="a 256-entry matplotlib colour map")
    ap.add_argument("--vminp", type=float, default=2, help="percentile mapped to the start of the colour map")
    ap.add_argument("--vmaxp", type=float, default=95, help="percentile mapped to its end")
    ap.add_argument("--invalid_val", type=float, default=-99, help="pixels equal to it are painted grey and left out of the percentiles")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if os.path.isdir(args.input):
        names = sorted(f for f in os.listdir(args.input) if f.lower().endswith(EXTENSIONS))
        if not names:
            ap.error(f"{args.input}: no depth files ({', '.join(EXTENSIONS)})")
        jobs = [(os.path.join(args.input, f), os.path.join(args.output, os.path.splitext(f)[0] + ".png")) for f in names]
    else:
        out = os.path.join(args.output, os.path.splitext(os.path.basename(args.input))[0] + ".png") if os.path.isdir(args.output) else args.output
        jobs = [(args.input, out)]
    for src, dst in jobs:
        colorize_file(src, dst, args.device, args.cmap, args.vminp, args.vmaxp, args.invalid_val)
        print(dst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
