"""Time of the guided filter's two passes on the device (csrc/ada_guided.hip, hip_ext/guided.py), on the device this runs on.

    python tools/profile_guided.py [--out profiles/guided_timing.txt] [--window 0.3] [--runs 2]

A 518 x 518 fp32 map (a ramp, a step and noise) against a uint8 guide of its own size and of 2160 x 3840, with C = 1 and 3 and r = 4, 8 and 31.  HIP
events around back-to-back launches of the raw exports on buffers already in HBM, outputs and workspace allocated once; every figure is the median of
three windows of at least ``--window`` seconds after a warm-up, with the windows' min-max.  Beside the coefficient pass: the rank filters' 9 x 9 median
of the same map, timed the same way (the other windowed operation of this size).  Beside the apply pass: its traffic floor, C bytes in and 4 bytes out
per guide pixel at 6.3 TB/s -- the coefficient table (8 (C + 1) bytes per map pixel) is re-read from cache and not counted -- and a plain device copy
of the output map.  ``--runs N`` repeats the whole table in one process, one column set per run, so the spread between runs is on the page.  Cache
state: every input fits the Infinity Cache and is re-read every call: inputs warm.  There is no CPU path: without a device the tool fails."""
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

MAP = (518, 518)
GUIDES = ((518, 518), (2160, 3840))
RADII = (4, 8, 31)
HBM_BYTES_PER_S = 6.3e12      # what a streaming kernel reaches on this part


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


def scene(h, w, H, W, C):
    rng = np.random.default_rng(h + W)
    yy, xx = np.mgrid[0:h, 0:w]
    p = (1.0 + 0.002 * xx + 0.001 * yy + 0.5 * (xx > 0.4 * w) + rng.normal(0, 0.05, (h, w))).astype(np.float32)
    XX = np.mgrid[0:H, 0:W][1]
    g = rng.integers(0, 80, (H, W, C)) + 120 * (XX > 0.42 * W)[..., None]
    return p[None], g.astype(np.uint8)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_timing.txt"))
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    import hip_ext
    hip_ext.load()
    assert torch.cuda.is_available(), "profile_guided needs a HIP device"
    prop = torch.cuda.get_device_properties(0)
    h, w = MAP
    lines = [f"device: {prop.name} ({getattr(prop, 'gcnArchName', '?')}), {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB; "
             f"us per call, median of three windows of >= {args.window} s [min-max]; map fp32 {h} x {w}, guide uint8, eps 1e-3 * 255^2, every sample voting"]
    for run in range(args.runs):
        x = torch.from_numpy(scene(h, w, h, w, 1)[0]).cuda()
        med_out = torch.empty_like(x)
        med, lo, hi = windows(lambda: hip_ext.rank_filter_fwd(x, 9, 9, hip_ext.RANK_MEDIAN, hip_ext.BORDER_MIRROR, med_out), args.window)
        lines.append(f"run {run}  median 9 x 9 of the map (rank_filter_fwd)        {med:9.1f} [{lo}-{hi}]")
        for H, W in GUIDES:
            for C in (1, 3):
                p_host, g_host = scene(h, w, H, W, C)
                p, g = torch.from_numpy(p_host).cuda(), torch.from_numpy(g_host).cuda()
                coeff = torch.empty(1, h, w, C + 1, dtype=torch.float64, device="cuda")
                covered = torch.empty(1, h, w, dtype=torch.uint8, device="cuda")
                out = torch.empty(1, H, W, dtype=torch.float32, device="cuda")
                other = torch.empty_like(out)
                ws = torch.empty(hip_ext.guided_workspace_bytes(1, h, w, C), dtype=torch.uint8, device="cuda")
                floor = H * W * (C + 4) / HBM_BYTES_PER_S * 1e6
                cp, cl, ch = windows(lambda: other.copy_(out), args.window)
                lines.append(f"run {run}  guide {H} x {W} C={C}: apply floor {floor:.1f} us ({C + 4} B per pixel at 6.3 TB/s), device copy of the output {cp} [{cl}-{ch}]")
                for r in RADII:
                    fit = lambda: hip_ext.guided_coeff_fwd(p, g, r, 1e-3 * 65025.0, coeff, covered, workspace=ws)      # noqa: E731
                    med, lo, hi = windows(fit, args.window)
                    lines.append(f"run {run}    r={r:2d}  coefficients {med:9.1f} [{lo}-{hi}]")
                med, lo, hi = windows(lambda: hip_ext.guided_apply_fwd(coeff, covered, g, out), args.window)
                lines.append(f"run {run}          apply        {med:9.1f} [{lo}-{hi}]   {med / floor:.1f} x its floor")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
