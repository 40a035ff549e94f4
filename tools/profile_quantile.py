"""Time of the exact device quantiles (csrc/ada_quantile.hip) behind hip_ext.quantile.percentile_range, on the device this runs on.

    python tools/profile_quantile.py [--out profiles/quantile.txt] [--window 1.0] [--bench LABEL=FILE ...]

Maps of 518 x 518, 1080 x 1920 and 2160 x 3840 with B = 1, and 32 x 518 x 518; contents: Gaussian noise (every digit of the radix select spread out), a
constant map and a map 87 % equal to 0 (a clipped ReLU) -- the two where, without the wave-level aggregation of equal bins, a whole wave adds to one LDS
word.  The recorded ratios constant / noise and clipped / noise at 4K say whether the aggregation does its job (near 1; above 2 needs an explanation in
DESIGN.md).

``select``: the raw export on a resident map with its workspace allocated once.  ``percentile_range``: the Python function, its allocations included.
Beside them: ``torch.quantile`` on the same device tensor (it sorts, and refuses more than 16 M elements) and the host path, a device -> host copy plus
``np.percentile`` on one core.  The three device figures share ONE clock -- HIP events around back-to-back calls -- and the host path takes the host clock
to a synchronise.  Every figure is the median of three windows after a warm-up, each sized from one host-timed call to about ``--window`` seconds (default 1; back-to-back
calls run faster than that one call, so a window lasts 0.7 s or more), with the windows' min-max.
Cache state: the calls of a window re-read ONE map of at most 33 MB (32 x 518 x 518: 34 MB), far below the 256 MB Infinity Cache, so after the first call
the passes are served from that cache, not from HBM: the figures are the warm-cache cost of the select.  ``select_rotating`` is the same call walking
round copies of the map that add up to 768 MB, three times the cache: its first pass comes from HBM, the other three from whatever the first left behind.  The device result is compared with np.percentile on float64 for every row.
``--bench``: JSON result lines of bench.py (the headline before and after) copied into the file.  There is no CPU path: without a device the tool fails."""
import argparse
import json
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

SHAPES = ((1, 518, 518), (1, 1080, 1920), (1, 2160, 3840), (32, 518, 518))
CONTENTS = ("noise", "constant", "clipped_87")


def make_map(kind, shape):
    rng = np.random.default_rng(shape[0] + shape[1] + shape[2])
    if kind == "noise":
        return rng.standard_normal(shape).astype(np.float32)
    if kind == "constant":
        return np.full(shape, 0.731, np.float32)
    x = rng.standard_normal(shape).astype(np.float32) - np.float32(1.1264)      # the 87 % point of the normal distribution
    return np.maximum(x, np.float32(0))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile.txt"))
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="how many of the shapes to run, in the order above")
    ap.add_argument("--bench", nargs="*", default=[], help="label=file pairs: the last JSON line of each file (a bench.py run) is recorded")
    a = ap.parse_args()
    import hip_ext as H
    from hip_ext.quantile import percentile_range
    H.load()
    assert torch.cuda.is_available(), "profile_quantile needs a HIP device"
    qs = [0.02, 0.95]
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# exact quantiles on {prop.name}: arch {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB "
             "(csrc/ada_quantile.hip, hip_ext/quantile.py)",
             "# python tools/profile_quantile.py",
             "# us per call: median of three windows (and their min-max) after a warm-up; the 2nd and 95th percentile of every image, map on the device.",
             f"# windows of about {a.window} s (sized from one host-timed call; 0.7 s or more).  select (ada_quantile_fwd alone, workspace allocated once), percentile_range (the Python function) and torch_quantile:",
             "# HIP events around back-to-back calls, one clock for the three.  Cache state: every call of a window re-reads the same map (<= 34 MB), which stays in the",
             "# 256 MB Infinity Cache: warm-cache figures, not HBM streaming.  select_rotating: select walking round copies of the map adding up to 768 MB (3 x the cache).",
             "# torch_quantile: torch.quantile(x.view(B, -1), [0.02, 0.95], dim=1) on the same device tensor (sorts; refuses > 16 M elements per call).",
             "# host: host clock to a synchronise; device -> host copy + np.percentile(float64) per image on one core.  exact: device result == np.percentile on float64, bit for bit.",
             "# No bar was fixed in advance.  The one condition: constant / noise and clipped / noise at 4K near 1 (the wave-level aggregation); above 2 is explained in DESIGN.md."]
    select_us = {}
    for shape in SHAPES[:a.shapes]:
        B = shape[0]
        for kind in CONTENTS:
            x = make_map(kind, shape)
            dev = torch.from_numpy(x).cuda()
            out = torch.empty(B, 2, dtype=torch.float64, device="cuda")
            out32 = torch.empty(B, 2, dtype=torch.float32, device="cuda")
            cnt = torch.empty(B, dtype=torch.int64, device="cuda")
            ws = torch.empty(H.quantile_workspace_bytes(B) // 4, dtype=torch.int32, device="cuda")

            def select():
                H.quantile_select(dev, qs, out, out_f32=out32, count=cnt, workspace=ws)
            select()
            want = np.stack([np.percentile(x[b].astype(np.float64).ravel(), [2, 95]) for b in range(min(B, 2))])
            exact = bool(np.array_equal(out[:min(B, 2)].cpu().numpy(), want))
            row = {"shape": list(shape), "map": kind, "exact": exact}
            row["select"] = windows(select, a.window, True)
            copies = dev[None].repeat(max(2, -(-768 * 2 ** 20 // (dev.numel() * 4))), *([1] * dev.dim()))
            turn = [0]

            def select_rotating():
                turn[0] = (turn[0] + 1) % copies.shape[0]
                H.quantile_select(copies[turn[0]], qs, out, out_f32=out32, count=cnt, workspace=ws)
            row["select_rotating"] = windows(select_rotating, a.window, True)
            row["select_rotating"]["copies"] = int(copies.shape[0])
            del copies
            row["percentile_range"] = windows(lambda: percentile_range(dev), a.window, True)
            tq = torch.tensor(qs, dtype=torch.float32, device="cuda")
            flat = dev.view(B, -1)
            try:
                row["torch_quantile"] = windows(lambda: torch.quantile(flat, tq, dim=1), a.window, True)
            except RuntimeError as e:
                row["torch_quantile"] = f"refused: {str(e).splitlines()[0][:80]}"
            row["host_copy_and_percentile"] = windows(lambda: [np.percentile(v.astype(np.float64).ravel(), [2, 95]) for v in dev.cpu().numpy()], 0.0, False)
            select_us[(shape, kind)] = row["select"]["us"]
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        ratio = {k: round(select_us[(shape, k)] / select_us[(shape, "noise")], 2) for k in CONTENTS[1:]}
        lines.append(json.dumps({"shape": list(shape), "select_time_over_noise": ratio, "within_2x": all(v <= 2 for v in ratio.values())}))
        print(lines[-1], flush=True)
    for item in a.bench:
        label, path = item.split("=", 1)
        last = [ln for ln in open(path).read().splitlines() if ln.startswith("{")][-1]
        lines.append(json.dumps({"bench": label, "result": json.loads(last)}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
