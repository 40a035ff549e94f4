"""Writes tests/golden/colorize/*.npz and tests/golden/depth_transform/*.npz with the reference's own functions.

    python tools/make_golden_quantile.py --reference /path/to/the/reference/checkout

* colorize() is lifted out of src/scripts/colorize_depth.py with ``ast`` at run time -- the script opens hard-coded paths when imported -- and executed
  with numpy / torch / matplotlib in its globals (matplotlib.cm.get_cmap, which the function calls and matplotlib 3.9 removed, is mapped onto
  matplotlib.colormaps).  The maps go in as float64 copies of fp32 values: that is the arithmetic the device reproduces.
* The normalizer is the reference's src/util/depth_transform.py, imported from its file and run on CPU tensors.

Only arrays are stored: the inputs, the arguments and what the reference returned.  Runs where a reference checkout exists; the tests read the files.
"""
import argparse
import ast
import importlib.util
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lift_colorize(reference):
    import matplotlib
    path = os.path.join(reference, "src", "scripts", "colorize_depth.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "colorize"]
    assert len(fn) == 1, f"{path}: expected one colorize()"
    shim = types.SimpleNamespace(cm=types.SimpleNamespace(get_cmap=lambda name: matplotlib.colormaps[name]))
    scope = {"np": np, "torch": torch, "matplotlib": shim}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), scope)
    return scope["colorize"]


def load_depth_transform(reference):
    path = os.path.join(reference, "src", "util", "depth_transform.py")
    spec = importlib.util.spec_from_file_location("reference_depth_transform", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def depth_map(rng, h, w):
    """A smooth ramp with noise and a flat far region: fp32, a few hundred distinct values, ties included."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    d = 2.0 + 0.05 * x + 0.03 * y + rng.standard_normal((h, w)).astype(np.float32) * 0.25
    d[y + x > 0.8 * (h + w)] = 9.5
    return d.astype(np.float32)


def colorize_cases(rng):
    d = depth_map(rng, 37, 53)
    a = d.copy()
    a[rng.random(a.shape) < 0.1] = -99
    yield "invalid_val", a, {}
    m = rng.random((64, 64)) < 0.3
    yield "invalid_mask", depth_map(rng, 64, 64), {"invalid_mask": m, "cmap": "Spectral_r"}
    yield "explicit_range", depth_map(rng, 48, 40), {"vmin": 2.5, "vmax": 6.25, "cmap": "magma_r"}
    yield "one_bound", depth_map(rng, 33, 29), {"vmax": 7.0, "vminp": 5}
    yield "constant", np.full((16, 24), 3.25, np.float32), {}
    n = depth_map(rng, 20, 31)
    n[3, 4] = np.nan
    yield "nan_pixel_explicit", n, {"vmin": 2.0, "vmax": 8.0}
    yield "nan_pixel_percentile", n, {}
    # with both bounds left to the percentiles np.percentile raises on the empty selection: the reference has no answer to pin (the device paints the background)
    yield "all_invalid_explicit", np.full((9, 11), -99, np.float32), {"vmin": 0.0, "vmax": 1.0}
    yield "other_percentiles", depth_map(rng, 41, 23), {"vminp": 0, "vmaxp": 100, "background_color": (1, 2, 3, 4), "invalid_val": 9.5}


def normalizer_cases(rng):
    d = depth_map(rng, 48, 40)
    d[rng.random(d.shape) < 0.05] = 0.0
    d[rng.random(d.shape) < 0.05] = -1.0
    valid = rng.random(d.shape) < 0.9
    yield "default", d, valid, dict(norm_min=-1.0, norm_max=1.0, min_max_quantile=0.02, clip=True)
    yield "unit_no_clip", d, None, dict(norm_min=0.0, norm_max=1.0, min_max_quantile=0.02, clip=False)
    yield "wide_quantile", depth_map(rng, 31, 17), None, dict(norm_min=-1.0, norm_max=1.0, min_max_quantile=0.1, clip=True)
    b = np.stack([depth_map(rng, 32, 32) * s for s in (1.0, 0.5, 3.0)])
    yield "batch_one_population", b, rng.random(b.shape) < 0.8, dict(norm_min=-1.0, norm_max=1.0, min_max_quantile=0.02, clip=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    args = ap.parse_args()
    colorize = lift_colorize(args.reference)
    out_dir = os.path.join(ROOT, "tests", "golden", "colorize")
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(20260)
    for name, value, kw in colorize_cases(rng):
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                img = colorize(value.astype(np.float64), **kw)
        assert img.dtype == np.uint8 and img.shape == value.shape + (4,)
        keys = {f"arg_{k}": np.asarray(v) for k, v in kw.items()}
        np.savez_compressed(os.path.join(out_dir, f"{name}.npz"), value=value, image=img, **keys)
        print("colorize", name, value.shape, sorted(kw))
    ref = load_depth_transform(args.reference)
    out_dir = os.path.join(ROOT, "tests", "golden", "depth_transform")
    os.makedirs(out_dir, exist_ok=True)
    for name, depth, valid, cfg in normalizer_cases(rng):
        norm = ref.get_depth_normalizer(types.SimpleNamespace(type="scale_shift_depth", **cfg))
        out = norm(torch.from_numpy(depth), None if valid is None else torch.from_numpy(valid)).numpy()
        assert out.dtype == np.float32 and out.shape == depth.shape
        keys = {f"cfg_{k}": np.asarray(v) for k, v in cfg.items()}
        if valid is not None:
            keys["valid"] = valid
        np.savez_compressed(os.path.join(out_dir, f"{name}.npz"), depth=depth, out=out, **keys)
        print("depth_transform", name, depth.shape, cfg)


if __name__ == "__main__":
    main()
