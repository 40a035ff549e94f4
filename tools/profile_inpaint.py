"""Time of the hole-filling kernels on the device (csrc/ada_inpaint.hip, hip_ext/inpaint.py), on the device this runs on.

    python tools/profile_inpaint.py [--out FILE] [--window 0.5] [--runs 2]

ada_nearest_valid_fwd, ada_fill_gather_fwd and ada_push_pull_fwd on 518 x 518 and 1022 x 1022, B = 1, C in {1, 3}: a smooth ramp plus noise with a
centred disc of a third of the shorter side and 10 % random pixels marked invalid.  HIP events around back-to-back launches of the raw exports on
maps already in HBM, outputs and workspace allocated once; every figure is the median of three windows of at least ``--window`` seconds after a
warm-up, with the windows' min-max.  Beside each: the bytes the pass must move once (counted from the shapes by ``must_move`` below: every map read
once, every map written once, the workspace written and read back) and a plain device-to-device copy that moves the same number of bytes
(``Tensor.copy_`` of half of them: one read, one write), timed the same way in the same run -- the memory floor.  ``--runs N`` repeats the whole
table in one process.  Cache state: every map fits the Infinity Cache and is re-read every call: inputs warm.  There is no CPU path: without a
device the tool fails."""
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

SIZES = ((518, 518), (1022, 1022))


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


def levels(h, w):
    out = [(h, w)]
    while out[-1] != (1, 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def must_move(h, w, C):
    """Bytes each entry point moves when every map is read once and written once (B = 1)."""
    n = h * w
    px = [a * b for a, b in levels(h, w)]
    pull = sum((4 * C + 1) * (lo + up) for lo, up in zip(px[:-1], px[1:]))                      # a level's values and mask in, the next level's out
    push = sum(lo + 4 * C * up + 4 * C * lo for lo, up in zip(px[:-1], px[1:])) + 4 * C * n      # mask and upper level in, the level out; level 0 reads x too
    return {"nearest_valid": (1 + 4 + 4 + 4) * n + (4 + 4 + 4) * n,      # columns: valid in, rows out, in, out; rows: rows in, index and dist2 out
            "fill_gather": (1 + 4 + 4 * C + 4 * C) * n,
            "push_pull": pull + push}


def scene(h, w, C):
    rng = np.random.default_rng(h)
    yy, xx = np.mgrid[0:h, 0:w]
    x = np.stack([(1.0 + 0.002 * xx + 0.001 * yy + rng.normal(0, 0.05, (h, w))).astype(np.float32) for _ in range(C)])[None]
    r = min(h, w) / 3.0
    valid = (((yy - h / 2.0) ** 2 + (xx - w / 2.0) ** 2) > r * r) & (rng.random((h, w)) >= 0.1)
    return x, valid.astype(np.uint8)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    import hip_ext
    hip_ext.load()
    assert torch.cuda.is_available(), "profile_inpaint needs a HIP device"
    prop = torch.cuda.get_device_properties(0)
    lines = [f"device: {prop.name} ({getattr(prop, 'gcnArchName', '?')}), {prop.multi_processor_count} CUs; us per call, median of three windows of >= {args.window} s "
             f"[min-max]; B = 1, fp32; bytes = what the pass must move once; copy = a device-to-device copy moving as many bytes, same run"]
    for h, w in SIZES:
        for C in (1, 3):
            x_host, v_host = scene(h, w, C)
            x, v = torch.from_numpy(x_host).cuda(), torch.from_numpy(v_host).cuda()
            out = torch.empty_like(x)
            index = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
            dist2 = torch.empty_like(index)
            ws_n = torch.empty(hip_ext.nearest_valid_workspace_bytes(1, h, w), dtype=torch.uint8, device="cuda")
            ws_p = torch.empty(hip_ext.push_pull_workspace_bytes(1, C, h, w), dtype=torch.uint8, device="cuda")
            calls = {"nearest_valid": lambda: hip_ext.nearest_valid_fwd(v, index, dist2, workspace=ws_n),
                     "fill_gather": lambda: hip_ext.fill_gather(x, v, index, out),
                     "push_pull": lambda: hip_ext.push_pull(x, v, out, workspace=ws_p)}
            need = must_move(h, w, C)
            lines.append(f"shape [1, {C}, {h}, {w}], {100.0 * (1.0 - v_host.mean()):.1f} % invalid, {len(levels(h, w)) - 1} pyramid levels above level 0")
            for run in range(args.runs):
                for name, fn in calls.items():
                    if name == "nearest_valid" and C != 1:
                        continue      # the transform does not see the channels
                    half = torch.empty(need[name] // 2, dtype=torch.uint8, device="cuda")
                    dst = torch.empty_like(half)
                    cmed, clo, chi = windows(lambda: dst.copy_(half), args.window)
                    med, lo, hi = windows(fn, args.window)
                    lines.append(f"  run {run}  {name:14s} {med:9.1f} [{lo}-{hi}]   bytes {need[name]:10d}   copy {cmed:7.1f} [{clo}-{chi}]")
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
