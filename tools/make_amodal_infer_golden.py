"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/amodal_infer/*.npz by calling the REAL reference's linear_regression_predict and
median_filter_blend (app.py:249-281) on seeded inputs.  Run where the reference tree exists (it does not travel to the GPU machine):

    python tools/make_amodal_infer_golden.py

app.py cannot be imported (it imports gradio, segment_anything, pix2gestalt ... at module level), so the file is parsed and just those two
function definitions are compiled from its syntax tree into a namespace that holds what they use: torch, F, np and a cv2 whose only member is
blur, bound to the project's box_blur (src/util/image_util.py; cv2 is not installed).  Nothing of the reference is copied into the fixtures:
they hold the seeded inputs and what its two functions returned.

Each fixture: amodal, base (fp32 [H, W] in [0, 1]), mask, visible (uint8 [H, W]), ref_aligned (fp32: linear_regression_predict(amodal, base,
visible)), ref_blend (fp32: median_filter_blend(ref_aligned, base, mask)), ref64 (the same fit called on float64 copies of the inputs).
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle._refshim import REFERENCE_ROOT  # noqa: E402
from src.util.image_util import box_blur  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "amodal_infer")
WANTED = ("linear_regression_predict", "median_filter_blend")
H, W = 48, 64      # small enough that each fixture stays near 60 KB, large enough for a ~100 pixel mask and a blurred border inside the map


def load_reference_functions(ref_root):
    path = os.path.join(ref_root, "app.py")
    tree = ast.parse(open(path).read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(d.name for d in defs) == sorted(WANTED), [d.name for d in defs]
    ns = dict(torch=torch, F=F, np=np, cv2=types.SimpleNamespace(blur=lambda img, ksize: box_blur(img, ksize[0])))
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns["linear_regression_predict"], ns["median_filter_blend"]


def ellipse(cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0)


def maps(seed):
    """A smooth base depth in [0, 1] and an amodal prediction that is an affine image of it plus structure of its own, both on a 2^-16 grid
    (the fixtures compress)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 0.5 + 0.25 * np.sin(yy * rng.uniform(0.03, 0.12) + xx * rng.uniform(0.03, 0.12)) + 0.2 * (xx / W - 0.5) + rng.normal(0, 0.01, (H, W))
    base = (base - base.min()) / (base.max() - base.min())
    amodal = rng.uniform(0.5, 0.8) * base + rng.uniform(0.05, 0.2) + 0.05 * np.cos(yy * 0.21 - xx * 0.17) + rng.normal(0, 0.01, (H, W))
    q = lambda a: (np.round(np.clip(a, 0, 1) * 65536) / 65536).astype(np.float32)
    return q(amodal), q(base)


# name -> (seed, amodal mask, visible mask)
def cases():
    whole = np.ones((H, W), bool)
    corner = np.zeros((H, W), bool)
    corner[:22, :28] = True                               # touches the top and the left border
    return {
        "visible_20pct": (1, ellipse(22, 32, 16, 24), ellipse(22, 27, 11, 17.8)),          # ~615 of 3072 pixels
        "visible_100px": (2, ellipse(25, 33, 15, 21), ellipse(22, 28, 5, 6.4)),             # ~100 pixels
        "visible_whole": (3, ellipse(21, 35, 13, 19), whole),
        "visible_two_borders": (4, ellipse(8, 10, 20, 24), corner),                         # the amodal mask runs off the same corner
    }


def generate(name, fit, blend):
    seed, mask, visible = cases()[name]
    amodal, base = maps(seed)
    a, b = torch.from_numpy(amodal), torch.from_numpy(base)
    vis = visible.astype(np.uint8)
    ref_aligned = fit(a, b, vis)
    ref64 = fit(a.double(), b.double(), vis)
    ref_blend = blend(ref_aligned, b.clone(), mask.astype(np.float64))
    assert ref_aligned.dtype == torch.float32 and ref64.dtype == torch.float64 and ref_blend.dtype == torch.float32
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, amodal=amodal, base=base, mask=mask.astype(np.uint8), visible=vis, ref_aligned=ref_aligned.numpy(),
                        ref_blend=ref_blend.numpy(), ref64=ref64.numpy())
    print(f"{name}: visible {int(vis.sum())} px, mask {int(mask.sum())} px, max|ref32 - ref64| = {float((ref_aligned.double() - ref64).abs().max()):.3e}, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    fit, blend = load_reference_functions(REFERENCE_ROOT)
    os.makedirs(OUT_DIR, exist_ok=True)
    for n in cases():
        generate(n, fit, blend)
