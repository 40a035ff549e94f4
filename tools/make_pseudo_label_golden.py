"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/pseudo_label/*.npz from the REAL reference's pseudo-label script
(src/scripts/sam_pl_gen_dav2.py) and its align_depth_least_square (src/util/alignment.py) on seeded inputs.  Run where the reference tree exists
(it does not travel to the GPU machine; its root comes from oracle/_refshim):

    python tools/make_pseudo_label_golden.py

The script cannot be imported or run: it parses arguments, lists cluster directories and loads ViT-G at module level.  What is done instead:

  * align_depth_least_square is the reference's own function, loaded from its file.
  * Lines 74-75, 88-89 (min-max normalisation), 101-106 (the call of the fit) and 115-117 (paste, * 65535, astype(np.uint16)) are EXECUTED FROM THE
    SCRIPT'S SYNTAX TREE: the statements of its sample loop that start on those lines are compiled as they stand and run in a namespace that holds
    the variables they read (depth, occ_depth, visible_mask, whole_mask) plus torch, np and the real fit.
  * Lines 93-94, 97-98 (masks: Image.open(path).resize((518, 518)), > 0) and 121 (Image.fromarray(u16).resize((512, 512))) are RESTATED here, because
    they hard-wire cluster paths and sizes and rely on Pillow's DEFAULT filter, which changed: the reference pins Pillow 10.0.1
    (environment.yaml:227), where mode L defaults to BICUBIC and modes with ';' ("I;16") to NEAREST; Pillow 12 resizes "I;16" with BICUBIC.  The
    restated lines pass Image.BICUBIC / Image.NEAREST explicitly -- the pinned version's defaults, never the installed one's.

Nothing of the reference is copied into the fixtures.  Each holds seeded inputs -- whole_depth, occ_depth (fp32 [70, 70], smooth, on a 2^-13 grid),
visible, whole (uint8 [45, 61] masks) -- and recorded results: ref_visible, ref_whole (uint8 [70, 70], the masks after the resize and > 0),
ref_whole_norm, ref_occ_norm (fp32, after lines 74 / 88), ref_scale_shift (fp32 [2], what the fit returned), ref_combined (fp32 [70, 70], line 116),
ref_label (uint16 [64, 64], lines 117 + 121 at label size 64).  cast_probes.npz holds the probe values of numpy's float32 -> uint16 cast and what
``astype(np.uint16)`` returned for them on this x86-64 host.
"""
import ast
import importlib.util
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle._refshim import REFERENCE_ROOT, reference_available  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "pseudo_label")
S, LABEL = 70, 64          # network size and label size of the fixtures (the script: 518 and 512)
MH, MW = 45, 61            # the masks' own size
FROM_TREE = (74, 75, 88, 89, 101, 115, 116, 117)     # first lines of the statements executed from the script's syntax tree


def load_reference():
    """(align_depth_least_square, code object of the script's statements FROM_TREE)."""
    assert reference_available(), f"reference tree not present at {REFERENCE_ROOT}"
    spec = importlib.util.spec_from_file_location("_adaref_alignment", os.path.join(REFERENCE_ROOT, "src", "util", "alignment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = os.path.join(REFERENCE_ROOT, "src", "scripts", "sam_pl_gen_dav2.py")
    tree = ast.parse(open(path).read(), filename=path)
    loops = [n for n in tree.body if isinstance(n, ast.For)]
    assert len(loops) == 1, "the script has one sample loop"
    stmts = [s for s in loops[0].body if s.lineno in FROM_TREE]
    assert [s.lineno for s in stmts] == list(FROM_TREE), [s.lineno for s in stmts]
    return mod.align_depth_least_square, compile(ast.Module(body=stmts, type_ignores=[]), path, "exec")


def ellipse(cy, cx, ry, rx):
    yy, xx = np.mgrid[0:MH, 0:MW]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0)


def q16(a):
    return (np.round(np.clip(a, 0, 1) * 65536) / 65536).astype(np.float32)


def maps(seed, a=None, b=None):
    """whole_depth, occ_depth: raw 'network outputs' whose min-max normalisations are exact.  W spans exactly [0, 1] on a 2^-16 grid and
    whole_depth = 8 W + 2; the occluded map is a W + b plus structure of its own, pinned to 0 and 1 at two pixels of the bottom-right corner (outside
    every mask), and occ_depth = 4 occ + 1."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    W = 0.5 + 0.25 * np.sin(yy * rng.uniform(0.03, 0.12) + xx * rng.uniform(0.03, 0.12)) + 0.2 * (xx / S - 0.5) + rng.normal(0, 0.01, (S, S))
    W = q16((W - W.min()) / (W.max() - W.min()))
    assert W.min() == 0 and W.max() == 1
    a = rng.uniform(0.5, 0.8) if a is None else a
    b = rng.uniform(0.05, 0.2) if b is None else b
    occ = a * W + b + 0.03 * np.cos(yy * 0.21 - xx * 0.17) + rng.normal(0, 0.005, (S, S))
    occ = q16(np.clip(occ, 1.0 / 64, 1 - 1.0 / 64))
    occ[S - 1, S - 1], occ[S - 1, S - 2] = 1.0, 0.0
    return (W * 8 + 2).astype(np.float32), (occ * 4 + 1).astype(np.float32)


# name -> (seed, whole mask, visible mask, overflow case, (a, b) of the occluded map or None)
def cases():
    corner = np.zeros((MH, MW), bool)
    corner[:16, :22] = True                                  # touches the top and the left border
    ell = ellipse(20, 30, 13, 20)
    return {
        "ellipse_partial": (1, ell, ell & (np.mgrid[0:MH, 0:MW][1] < 33), False, None),
        "visible_whole": (2, ellipse(22, 28, 12, 17), ellipse(22, 28, 12, 17), False, None),
        "two_borders": (3, ellipse(5, 7, 15, 19), corner & ellipse(5, 7, 15, 19), False, None),
        "empty_visible": (4, ellipse(21, 33, 11, 16), np.zeros((MH, MW), bool), False, None),
        "overflow": (5, ellipse(20, 30, 14, 22), ellipse(20, 30, 5, 7), True, (2.6, -0.8)),   # the occluded map clips at both ends: the fit leaves [0, 1]
    }


def generate(name, fit, code):
    seed, whole, visible, overflow, ab = cases()[name]
    whole_depth, occ_depth = maps(seed, *(ab or (None, None)))
    whole_u8, visible_u8 = whole.astype(np.uint8) * 255, visible.astype(np.uint8) * 255
    # lines 93-94, 97-98 restated: Image.open(path).resize((518, 518)) of a mode-L file, BICUBIC under the pinned Pillow; np.asarray(...) > 0
    visible_mask = np.asarray(Image.fromarray(visible_u8).resize((S, S), Image.BICUBIC)) > 0
    whole_mask = np.asarray(Image.fromarray(whole_u8).resize((S, S), Image.BICUBIC)) > 0
    # lines 72-73, 86-87: the network's [1, H, W] output, unsqueezed to [1, 1, H, W] (F.interpolate to its own size is the identity)
    ns = dict(torch=torch, np=np, align_depth_least_square=fit, visible_mask=visible_mask, whole_mask=whole_mask,
              depth=torch.from_numpy(whole_depth)[None, None].clone(), occ_depth=torch.from_numpy(occ_depth)[None, None].clone())
    with np.errstate(invalid="ignore"):
        exec(code, ns)
    combine, save = ns["combine_depth"], ns["combine_depth_save"]
    assert save.dtype == np.uint16 and combine.dtype == torch.float32 and tuple(combine.shape) == (S, S)
    # line 121 restated: Image.fromarray(u16).resize((512, 512)) of an "I;16" image, NEAREST under the pinned Pillow
    im = Image.fromarray(save)
    assert im.mode == "I;16", im.mode
    label = np.asarray(im.resize((LABEL, LABEL), Image.NEAREST))
    ss = np.array([np.asarray(ns["scale"]).reshape(-1)[0], np.asarray(ns["shift"]).reshape(-1)[0]])
    assert ss.dtype == np.float32, ss.dtype
    inside = combine.numpy()[whole_mask]
    if not overflow:   # the +-1 code bound of the chain test means something only when nothing wraps
        assert inside.min() >= 0 and inside.max() < 1, (name, inside.min(), inside.max())
    else:
        assert inside.min() < 0 and inside.max() * 65535 >= 65536, (name, inside.min(), inside.max())
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, whole_depth=whole_depth, occ_depth=occ_depth, visible=visible_u8, whole=whole_u8,
                        ref_visible=visible_mask.astype(np.uint8), ref_whole=whole_mask.astype(np.uint8), ref_whole_norm=ns["depth"].numpy(),
                        ref_occ_norm=ns["occ_depth"].numpy(), ref_scale_shift=ss, ref_combined=combine.numpy(), ref_label=label)
    print(f"{name}: visible {int(visible_mask.sum())} px, whole {int(whole_mask.sum())} px, scale, shift = {ss.tolist()}, inside the mask "
          f"[{inside.min():.4f}, {inside.max():.4f}], {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 100 * 1024


def cast_probes():
    """numpy's float32 -> uint16 astype on this host, recorded: the probes of include/ada_hip.h and a few more around the edges."""
    t = np.array([-3.7, 65536.0, 65537.9, 70000.5, np.nan, 1e10, -1e10, -0.5, 65535.99, -65536.2, 0.0, 1.5, 65535.0, 2147483520.0, -2147483648.0,
                  np.inf, -np.inf], np.float32)
    with np.errstate(invalid="ignore"):
        u = t.astype(np.uint16)
    np.savez_compressed(os.path.join(OUT_DIR, "cast_probes.npz"), values=t, as_uint16=u)
    print("cast probes:", dict(zip(t.tolist(), u.tolist())))


if __name__ == "__main__":
    fit, code = load_reference()
    os.makedirs(OUT_DIR, exist_ok=True)
    for n in cases():
        generate(n, fit, code)
    cast_probes()
