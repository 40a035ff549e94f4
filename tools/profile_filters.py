"""Time of the rank filters on the device (csrc/ada_filters.hip, hip_ext/filters.py), on the device this runs on.

    python tools/profile_filters.py [--out profiles/filters_timing.txt] [--window 0.5] [--runs 2] [--no-scipy]

The median filter at 3, 5, 7 and 9 (the general kernel) and the maximum at 3 and 63 (the separable kernels) on fp32 maps of [8, 518, 518] and
[1, 1022, 1022] (a smooth ramp plus noise), border 'mirror', every sample voting.  HIP events around back-to-back launches of the raw exports on maps
already in HBM, outputs and workspace allocated once; every figure is the median of three windows of at least ``--window`` seconds after a warm-up,
with the windows' min-max.  Beside each: a plain device copy of the same map (``Tensor.copy_``, the memory floor: one read and one write of the map)
timed the same way, and -- context only -- scipy.ndimage's median_filter / maximum_filter for the same call on one host core.  ``--runs N`` repeats
the whole table in one process, one column per run, so the spread between runs is on the page.  Cache state: the maps (8.6 MB and 4.2 MB) fit the
Infinity Cache and are re-read every call: inputs warm.  There is no CPU path: without a device the tool fails."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ((8, 518, 518), (1, 1022, 1022))
CASES = (("median", 3), ("median", 5), ("median", 7), ("median", 9), ("max", 3), ("max", 63))


def windows(fn, seconds):
    """Median and min-max, in microseconds per call, of three HIP-event windows of at least ``seconds``."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(3, int(seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
    out = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return round(statistics.median(out), 1), round(min(out), 1), round(max(out), 1)


def scene(shape):
    B, h, w = shape
    rng = np.random.default_rng(h)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(1.0 + 0.002 * xx + 0.001 * yy + rng.normal(0, 0.05, (h, w))).astype(np.float32) for _ in range(B)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filters_timing.txt"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    import hip_ext
    hip_ext.load()
    assert torch.cuda.is_available(), "profile_filters needs a HIP device"
    prop = torch.cuda.get_device_properties(0)
    lines = [f"device: {prop.name} ({getattr(prop, 'gcnArchName', '?')}), {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB; "
             f"us per call, median of three windows of >= {args.window} s [min-max]; border mirror, fp32, every sample voting"]
    for shape in SHAPES:
        x_host = scene(shape)
        x = torch.from_numpy(x_host).cuda()
        out = torch.empty_like(x)
        ws = torch.empty(hip_ext.extreme_filter_workspace_bytes(*shape), dtype=torch.uint8, device="cuda")
        lines.append(f"shape {list(shape)}")
        for run in range(args.runs):
            med, lo, hi = windows(lambda: out.copy_(x), args.window)
            lines.append(f"  run {run}  device copy            {med:9.1f} [{lo}-{hi}]")
            for rank, k in CASES:
                if rank == "median":
                    fn = lambda: hip_ext.rank_filter_fwd(x, k, k, hip_ext.RANK_MEDIAN, hip_ext.BORDER_MIRROR, out)      # noqa: E731
                else:
                    fn = lambda: hip_ext.extreme_filter_fwd(x, k, k, hip_ext.RANK_MAX, hip_ext.BORDER_MIRROR, out, workspace=ws)      # noqa: E731
                med, lo, hi = windows(fn, args.window)
                lines.append(f"  run {run}  {rank:6s} {k:2d} x {k:2d}         {med:9.1f} [{lo}-{hi}]")
        if not args.no_scipy:
            import scipy.ndimage as ndi
            for rank, k in CASES:
                t0 = time.perf_counter()
                for m in x_host:
                    (ndi.median_filter if rank == "median" else ndi.maximum_filter)(m, size=k, mode="mirror")
                lines.append(f"  host   scipy {rank:6s} {k:2d} x {k:2d}   {(time.perf_counter() - t0) * 1e6:11.0f}   (one core, one pass, context only)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
