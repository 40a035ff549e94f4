"""Time of the mask-component kernels (csrc/ada_masks.hip) and of hip_ext.masks' three functions, on the device this runs on.

    python tools/profile_mask_components.py [--out profiles/mask_components.txt] [--window 0.2]

Masks of 518 x 518, 1080 x 1920 and 2160 x 3840; contents: an ellipse (one smooth component), noise at density 0.59 (near the percolation threshold:
one winding giant component and a crowd of small ones), a serpentine (even rows full, joined at alternating ends: the longest chain a union-find can
meet) and a checkerboard (one component under 8-connectivity, h w / 2 under 4).  The serpentine and the checkerboard are there for ONE condition: they
must finish within the order of magnitude of the ellipse at equal size -- a data-dependent blow-up would mean the union loop is wrong, not slow.

Raw exports: HIP events around back-to-back calls on masks already in HBM, workspaces allocated once.  Python functions: host clock around calls that
end in a device synchronise (they include their allocations and, where documented, their one host read).  Every figure is the median of three windows
of at least ``--window`` seconds after a warm-up, with the windows' min-max.  Beside them, for context, the host path on the same masks: the device ->
host copy of the mask plus scipy.ndimage.label where scipy exists, otherwise the numpy restatement of the tests (518 x 518 only: it is plain Python).
There is no CPU path: without a device the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = ((518, 518), (1080, 1920), (2160, 3840))


def make_mask(kind, h, w):
    yy, xx = np.mgrid[:h, :w]
    if kind == "ellipse":
        return ((((yy - 0.54 * h) / (0.23 * h)) ** 2 + ((xx - 0.44 * w) / (0.29 * w)) ** 2) <= 1.0).astype(np.uint8)
    if kind == "noise_0.59":
        return (np.random.default_rng(h + w).random((h, w)) < 0.59).astype(np.uint8)
    if kind == "serpentine":
        m = np.zeros((h, w), np.uint8)
        m[0::2] = 1
        for k, y in enumerate(range(1, h - 1, 2)):
            m[y, w - 1 if k % 2 == 0 else 0] = 1
        return m
    if kind == "checkerboard":
        return ((yy + xx) % 2 == 0).astype(np.uint8)
    raise ValueError(kind)


def windows(fn, seconds, device_events):
    """Median and min-max, in microseconds per call, of three windows of at least ``seconds``."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(3, int(seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
    out = []
    for _ in range(3):
        if device_events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) * 1e3 / reps)
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e6 / reps)
    return {"us": round(statistics.median(out), 1), "us_min_max": [round(min(out), 1), round(max(out), 1)], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_components.txt"))
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--sizes", type=int, default=len(SIZES), help="how many of the sizes to run, smallest first")
    a = ap.parse_args()
    import hip_ext as H
    from hip_ext import masks as M
    H.load()
    assert torch.cuda.is_available(), "profile_mask_components needs a HIP device"
    try:
        from scipy import ndimage
        host_name = "scipy.ndimage.label"
    except ImportError:
        ndimage = None
        host_name = "tests/_components_ref.label"
    import _components_ref as R
    lines = [f"# mask components on {torch.cuda.get_device_name(0)} (csrc/ada_masks.hip, hip_ext/masks.py)",
             "# python tools/profile_mask_components.py",
             "# us per call: median of three windows (and their min-max) after a warm-up.  label / stats / keep_area / grid_points: the raw exports, HIP events, mask and",
             "# workspaces resident; connected_components / remove_small_noise / points_from_components: the Python functions on a device tensor, host clock to a",
             "# synchronise (allocations and their documented host read included).  8-connectivity except remove_small_noise (4, the reference's).",
             f"# host_*: device -> host copy of the mask + {host_name} on one core, for context.  components = what the device counted.",
             "# No bar was fixed in advance.  The one condition: serpentine and checkerboard within the order of magnitude of the ellipse at equal size."]
    for h, w in SIZES[:a.sizes]:
        label_us = {}
        for kind in ("ellipse", "noise_0.59", "serpentine", "checkerboard"):
            m = make_mask(kind, h, w)
            dev = torch.from_numpy(m).cuda()[None]
            labels = torch.empty(1, h, w, dtype=torch.int32, device="cuda")
            count = torch.empty(1, dtype=torch.int32, device="cuda")
            ws = torch.empty(H.mask_label_workspace_bytes(1, h, w) // 4, dtype=torch.int32, device="cuda")
            ws_keep = torch.empty(H.mask_keep_area_workspace_bytes(1, h, w) // 4, dtype=torch.int32, device="cuda")
            H.mask_label(dev, 1, h, w, w, h * w, 8, labels, count, ws)
            n = int(count.item())
            if ndimage is not None:
                want, n_want = ndimage.label(m, structure=np.ones((3, 3)))
                exact = bool(n == n_want and np.array_equal(labels[0].cpu().numpy(), want))
            elif h * w <= 518 * 518:
                want, n_want = R.label(m, 8)
                exact = bool(n == n_want and np.array_equal(labels[0].cpu().numpy(), want))
            else:
                exact = None
            stats = torch.empty(1, n + 1, 5, dtype=torch.int32, device="cuda")
            sums = torch.empty(1, n + 1, 2, dtype=torch.int64, device="cuda")
            keep = torch.empty(1, h, w, dtype=torch.uint8, device="cuda")
            hit = torch.empty_like(labels)
            row = {"size": [h, w], "mask": kind, "components": n, "labels_equal_host": exact}
            row["label"] = windows(lambda: H.mask_label(dev, 1, h, w, w, h * w, 8, labels, count, ws), a.window, True)
            row["stats"] = windows(lambda: H.mask_stats(labels, n, stats, sums), a.window, True)
            row["keep_area"] = windows(lambda: H.mask_keep_area(labels, 500, out_u8=keep, workspace=ws_keep), a.window, True)
            row["grid_points"] = windows(lambda: H.mask_grid_points(labels, stats, 100, 10, hit), a.window, True)
            row["connected_components"] = windows(lambda: M.connected_components(dev), a.window, False)
            row["remove_small_noise"] = windows(lambda: M.remove_small_noise(dev), a.window, False)
            row["points_from_components"] = windows(lambda: M.points_from_components(dev), a.window, False)
            row["points"] = int(M.points_from_components(dev)[0].shape[0])
            if ndimage is not None:
                row["host_copy_and_label"] = windows(lambda: ndimage.label(dev[0].cpu().numpy(), structure=np.ones((3, 3))), a.window, False)
            elif h * w <= 518 * 518:
                row["host_copy_and_label"] = windows(lambda: R.label(dev[0].cpu().numpy(), 8), 0.0, False)
            else:
                row["host_copy_and_label"] = "not measured (no scipy here; the restatement is plain Python)"
            label_us[kind] = row["label"]["us"]
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        cond = {k: round(label_us[k] / label_us["ellipse"], 2) for k in ("noise_0.59", "serpentine", "checkerboard")}
        lines.append(json.dumps({"size": [h, w], "label_time_over_ellipse": cond, "within_one_order_of_magnitude": all(v < 10 for v in cond.values())}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
