"""Cost of rendering the amodal infer_image's maps on the device: 518 x 518 maps to 480p, 1080p and 4K pictures, K = 1 and 8 masks.

    python tools/profile_render.py > profiles/render_kernels.txt

With HIP events, ada_depth_render_fwd alone (hip_ext.depth_render: Spectral_r, B, G, R bytes): the raw rendering (one map, no mask) and the K amodal
renderings (mask, outline of thickness 2, no overlay -- what infer.py draws).  The kernel has two store shapes: four pixels per thread with dword
stores when the width is a multiple of 4 and the output is aligned ("ppt4"), one pixel per thread with byte stores otherwise ("ppt1").  Both are
timed on the same inputs, alternating, three rounds each (median, and the min-max spread over the rounds): the one-pixel form is reached through
the launcher's own rule, by handing it an output pointer one byte off alignment.  854 is not a multiple of 4, so 480p has only the one-pixel figure.
Bytes are the algorithm's: the K maps and masks read once (fp32), the K pictures written once (3 bytes per pixel); GB/s is bytes over kernel time.
With the host clock, what the CLI does instead per mask without --device_render: the device -> host copy of the map, colorize_depth_maps,
highlight_target, resize_nearest and the channel flip (src/util/image_util.py, infer.py), K + 1 times (the raw map once).  No network runs here.
Prints one JSON line per (picture, K).
"""
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

import hip_ext  # noqa: E402
import infer  # noqa: E402
from hip_ext.image import colormap_lut  # noqa: E402
from src.util.image_util import chw2hwc, colorize_depth_maps, resize_nearest  # noqa: E402

S = 518
WINDOW_S = 0.25      # each timed window holds at least this much kernel time


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fns, rounds=3):
    """fns: name -> callable.  Warm-up, a short estimate to size the window, then `rounds` alternating windows per name: name -> (median, min, max) in ms."""
    reps = {}
    for name, fn in fns.items():
        for _ in range(5):
            fn()
        reps[name] = int(min(max(WINDOW_S * 1e3 / max(event_ms(fn, 20), 1e-3), 50), 5000))
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(event_ms(fn, reps[name]))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def blobs(k):
    yy, xx = np.mgrid[0:S, 0:S]
    return np.stack([(((yy - S * (0.3 + 0.05 * i)) / (S * 0.2)) ** 2 + ((xx - S * (0.3 + 0.05 * i)) / (S * 0.2)) ** 2 <= 1) for i in range(k)]).astype(np.float32)


def host_render(maps, masks, h, w):
    """The parent's host rendering of infer.py for one raw map and K blended ones, device -> host copies included."""
    raw = maps[0].cpu().numpy()
    raw_colored = (colorize_depth_maps(raw, 0, 1, cmap="Spectral_r").squeeze() * 255).astype(np.uint8)
    out = [resize_nearest(chw2hwc(raw_colored), w, h)[:, :, [2, 1, 0]]]
    for k in range(masks.shape[0]):
        agg = maps[k + 1].cpu().numpy()
        mask518 = (masks[k].cpu().numpy() > 0).astype(np.uint8) * 255
        colored = (colorize_depth_maps(agg, 0, 1, cmap="Spectral_r").squeeze() * 255).astype(np.uint8)
        out.append(np.ascontiguousarray(resize_nearest(infer.highlight_target(chw2hwc(colored), mask518), w, h)[:, :, [2, 1, 0]]))
    return out


def main():
    hip_ext.load()
    dev = "cuda"
    lut = colormap_lut("Spectral_r", dev)
    for h, w in ((480, 854), (1080, 1920), (2160, 3840)):
        for k in (1, 8):
            maps = torch.rand(k + 1, S, S, device=dev)
            masks = torch.from_numpy(blobs(k)).to(dev)
            raw_buf = torch.empty(h * w * 3 + 4, dtype=torch.uint8, device=dev)
            am_buf = torch.empty(k * h * w * 3 + 4, dtype=torch.uint8, device=dev)
            fns = {}
            for name, off in (("ppt4", 0), ("ppt1", 1)):
                if name == "ppt4" and w % 4:
                    continue
                fns["raw_" + name] = lambda off=off: hip_ext.depth_render(maps[:1], lut, h, w, raw_buf[off:], bgr=True)
                fns["amodal_" + name] = lambda off=off: hip_ext.depth_render(maps[1:], lut, h, w, am_buf[off:], mask=masks, thickness=2, bgr=True)
            if "amodal_ppt4" in fns:     # the two store shapes write the same bytes
                fns["amodal_ppt4"]()
                a = am_buf[:k * h * w * 3].clone()
                fns["amodal_ppt1"]()
                assert torch.equal(a, am_buf[1:1 + k * h * w * 3]), "ppt4 and ppt1 disagree"
            t = timed(fns)
            reps = 3
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                host_render(maps, masks, h, w)
            host_ms = (time.perf_counter() - t0) * 1e3 / reps
            raw_bytes = S * S * 4 + h * w * 3
            am_bytes = k * (2 * S * S * 4 + h * w * 3)
            rec = dict(picture=[h, w], K=k, size=S, raw_bytes=raw_bytes, amodal_bytes=am_bytes)
            for name, (med, lo, hi) in t.items():
                rec[name + "_us"] = round(med * 1e3, 1)
                rec[name + "_us_min_max"] = [round(lo * 1e3, 1), round(hi * 1e3, 1)]
                rec[name + "_GBps"] = round((raw_bytes if name.startswith("raw") else am_bytes) / (med * 1e6), 1)
            best = lambda kind: min(v[0] for n, v in t.items() if n.startswith(kind))      # noqa: E731
            rec["device_render_total_ms"] = round(best("raw") + best("amodal"), 3)
            rec["host_render_ms"] = round(host_ms, 2)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
