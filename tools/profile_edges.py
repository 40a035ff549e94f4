"""Time of the edge metrics on the device (csrc/ada_edges.hip, hip_ext/edges.py, src/util/metric.py), on the device this runs on.

    python tools/profile_edges.py [--out profiles/edges_timing.txt] [--window 1.0] [--no-kernel-trace]

``edge_metrics`` at 518 x 518 with B = 1 and B = 32, on synthetic depth scenes (a ramp, a sine, discs of constant depth and noise: a few thousand edge
pixels per map), and the per-kernel split behind it: the detector's front end, hysteresis (the labeller included), the distance transform, the sums,
and soft_edge_error at radius 1.

Raw exports: HIP events around back-to-back calls on maps already in HBM, outputs and workspaces allocated once.  Python functions: host clock around
calls that end in a device synchronise (they include their allocations).  Every figure is the median of three windows of at least ``--window`` seconds
after a warm-up, with the windows' min-max.  These are CALL times: an export such as the hysteresis covers ten kernels (the labeller's six and four of its
own).  KERNEL times come from a run of their own: the tool starts a fresh child process under ``rocprofv3 --kernel-trace`` that calls ``edge_metrics``
a fixed number of times, and reports per kernel the launches per call and the median duration from the trace, with the share of the call's span that
no kernel covers (launch gaps).  Cache state: the maps of a window (at most 32 x 518 x 518 x 8 bytes = 69 MB for the fp64 distance maps) fit
the 256 MB Infinity Cache and are re-read every call: inputs warm.  No time was promised for this path; the file records what was measured.  Where scipy
exists, the host path on the same maps is recorded beside it: the device -> host copy of two maps and, on one core, tests/_edges_ref's stages with
scipy.ndimage.label and distance_transform_edt in place of the plain-Python ones.  There is no CPU path: without a device the tool fails."""
import argparse
import collections
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZE = (518, 518)
BATCHES = (1, 32)


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


CHILD_WARMUP, CHILD_CALLS = 5, 40


def scenes(B, h, w):
    import _edges_ref as R
    pred = torch.from_numpy(np.stack([R.scene(2 * b, h, w) for b in range(B)])).cuda()
    gt = torch.from_numpy(np.stack([R.scene(2 * b + 1, h, w) for b in range(B)])).cuda()
    valid = torch.from_numpy(np.random.default_rng(B).random((B, h, w)) < 0.8).cuda()
    return pred, gt, valid


def child(B):
    """What the profiler runs: edge_metrics on B maps, CHILD_WARMUP + CHILD_CALLS times, a synchronise after each call."""
    from src.util import metric
    pred, gt, valid = scenes(B, *SIZE)
    for _ in range(CHILD_WARMUP + CHILD_CALLS):
        metric.edge_metrics(pred, gt, valid)
        torch.cuda.synchronize()


def short_name(name):
    if "at::native" in name or "rocclr" in name or "at::cuda" in name:
        return "torch ops and copies"
    m = re.search(r"(\w+)(?:<[^()]*>)?\(", name)
    return m.group(1) if m else name[:40]


def kernel_split(B):
    """Per kernel of one edge_metrics call on B maps, from a rocprofv3 --kernel-trace run of a fresh child process: launches per call, median kernel
    duration, their product; then the kernels' sum and the median span from a call's first kernel start to its last kernel end."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="edges_trace_")
    try:
        subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", str(B)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=240)
        path = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)[0]
        rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short_name(r["Kernel_Name"])) for r in csv.DictReader(open(path))))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # the calls are separated by synchronises: the canny front end runs exactly twice per call and opens it
    starts = [i for i, r in enumerate(rows) if r[2] == "canny_kernel"][0::2]
    assert len(starts) == CHILD_WARMUP + CHILD_CALLS, (len(starts), "calls found in the trace")
    bounds = starts[CHILD_WARMUP:] + [len(rows)]
    per, spans = collections.OrderedDict(), []
    for a, b in zip(bounds[:-1], bounds[1:]):
        call = rows[a:b]
        spans.append((max(r[1] for r in call) - call[0][0]) / 1e3)
        for st, en, name in call:
            per.setdefault(name, []).append((en - st) / 1e3)
    out = {"batch": B, "kernel_trace_of": f"{CHILD_CALLS} calls of edge_metrics after {CHILD_WARMUP}", "kernels": {}}
    total = 0.0
    for name, d in per.items():
        launches = len(d) / CHILD_CALLS
        med = statistics.median(d)
        total += launches * med
        out["kernels"][name] = {"launches_per_call": round(launches, 2), "median_us": round(med, 2), "us_per_call": round(launches * med, 1)}
    out["kernels_us_per_call"] = round(total, 1)
    out["span_us_per_call"] = round(statistics.median(spans), 1)
    out["uncovered_share_of_span"] = round(1.0 - total / statistics.median(spans), 3)
    return out


def host_path(pred, gt, valid, ndimage, R):
    """The reference's EdgeAcc + EdgeComp for one sample on the host, the detector run once per map (the reference runs it twice)."""
    def edges(d):
        st_in = R.to_log(d)
        s = R.smooth(st_in, 1.0)
        i, j = R.sobel(s, 0), R.sobel(s, 1)
        lm = R.nms(i, j, R.magnitude(i, j), 0.1)
        labels, count = ndimage.label(lm > 0, np.ones((3, 3), bool))
        good = np.zeros(count + 1, bool)
        good[np.unique(labels[lm >= np.float32(0.2)])] = True
        good[0] = False
        return good[labels]
    pe, ge = edges(pred), edges(gt)
    dt, dp = ndimage.distance_transform_edt(~ge), ndimage.distance_transform_edt(~pe)
    bde = pe & valid & (dt < 10)
    return (dt[bde].mean() if bde.any() else 10.0), (dp[ge & valid].mean() if bde.any() and (ge & valid).any() else 10.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edges_timing.txt"))
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--no-kernel-trace", action="store_true", help="skip the rocprofv3 --kernel-trace child runs")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    import hip_ext as H
    from hip_ext import edges as E
    from src.util import metric
    import _edges_ref as R
    H.load()
    assert torch.cuda.is_available(), "profile_edges needs a HIP device"
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    h, w = SIZE
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# edge metrics on {prop.name}: {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB "
             "(csrc/ada_edges.hip, hip_ext/edges.py, src/util/metric.py)",
             "# python tools/profile_edges.py",
             f"# {h} x {w} maps, sigma 1 (a 44 x 44 LDS tile per 32 x 32 outputs).  us per call: median of three windows (and their min-max) after a warm-up.",
             "# canny_front / hysteresis / edt / edge_sums / soft_edge: the raw exports, HIP events, maps, outputs and workspaces resident (inputs warm in the",
             "# Infinity Cache); per call they cover ONE set of B maps, edge_metrics runs the first three twice (prediction and ground truth).",
             "# edge_metrics / soft_edge_error: the Python functions on device tensors, host clock to a synchronise, allocations included.",
             "# host_*: device -> host copy of two maps + tests/_edges_ref's numpy stages with scipy's label and distance transform, ONE detector run per map, one",
             "# core, one sample.  It is NOT skimage and not the reference's two detector runs per map per metric: context only, no speed-up is claimed from it.",
             "# kernel_trace rows: rocprofv3 --kernel-trace over a fresh child process, per kernel launches per edge_metrics call and the median duration; the tracer",
             "# slows the host, so the span is not a call time -- the call times are the rows above, taken with the profiler off.",
             "# No bar was fixed in advance: this file records what was measured."]
    for B in BATCHES:
        pred, gt, valid = scenes(B, h, w)
        valid8 = valid.view(torch.uint8)
        weights = torch.from_numpy(E.gaussian_weights(1.0)).cuda()
        low_masked = torch.empty_like(pred)
        edges = torch.empty(B, h, w, dtype=torch.uint8, device="cuda")
        gt_edges = E.canny(gt, pre="log")
        dist, dist_gt = torch.empty(B, h, w, dtype=torch.float64, device="cuda"), E.distance_transform_edt(gt_edges)
        sums4 = torch.empty(B, 4, dtype=torch.float64, device="cuda")
        sums2 = torch.empty(B, 2, dtype=torch.float64, device="cuda")
        ws_h = torch.empty(H.canny_hysteresis_workspace_bytes(B, h, w) // 4 + 1, dtype=torch.int32, device="cuda")
        ws_e = torch.empty(H.edt_workspace_bytes(B, h, w) // 4, dtype=torch.int32, device="cuda")
        ws_s = torch.empty(H.edge_sums_workspace_bytes(B, 4) // 4, dtype=torch.int32, device="cuda")
        row = {"size": [h, w], "batch": B}
        row["canny_front"] = windows(lambda: H.canny_front(pred, weights, 0.1, low_masked, H.CANNY_PRE_LOG), a.window, True)
        row["hysteresis"] = windows(lambda: H.canny_hysteresis(low_masked, 0.2, edges, ws_h), a.window, True)
        row["edge_pixels_per_map"] = round(float(edges.sum()) / B, 1)
        row["edt"] = windows(lambda: H.edt(edges, dist, ws_e), a.window, True)
        row["edge_sums"] = windows(lambda: H.edge_metric_sums(edges, gt_edges, valid8, dist_gt, dist, 10.0, sums4, ws_s), a.window, True)
        row["soft_edge_r1"] = windows(lambda: H.soft_edge(pred, gt, valid8, 1, sums2, ws_s), a.window, True)
        row["edge_metrics"] = windows(lambda: metric.edge_metrics(pred, gt, valid), a.window, False)
        row["soft_edge_error"] = windows(lambda: metric.soft_edge_error(pred[0], gt[0], valid[0]), a.window, False)
        row["per_image_us"] = round(row["edge_metrics"]["us"] / B, 1)
        if ndimage is not None and B == 1:
            row["host_copy_and_edge_metrics"] = windows(lambda: host_path(pred[0].cpu().numpy(), gt[0].cpu().numpy(), valid[0].cpu().numpy(), ndimage, R),
                                                        a.window, False)
        elif B == 1:
            row["host_copy_and_edge_metrics"] = "not measured (no scipy here)"
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if not a.no_kernel_trace:
        for B in BATCHES:
            lines.append(json.dumps(kernel_split(B)))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
