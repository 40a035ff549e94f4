"""Cost of the amodal infer_image's preparation on photo-sized inputs: 480p, 1080p and 4K uint8 BGR photos, K = 1 and 8 masks.

    python tools/profile_amodal_prep.py > profiles/amodal_prep_kernels.txt

With HIP events, each of the four kernels alone: ada_photo_prep_fwd (both 518 x 518 planes in one pass), ada_mask_prep_fwd (K masks at the photo's
size, both outputs), ada_blend_ex (K maps at 518 x 518, with a scale / shift) and ada_nearest_resize_fwd (base + K blended maps back to the
photo's size); the host-to-device copies of the photo and the masks beside them.  With the host clock, the preparation the CLI's
_on_device_pipeline (infer.py) does per mask on the host: the float bilinear resize + rounding, two F.interpolate calls and three
host-to-device copies of fp32 planes -- K times, since that path prepares (and runs the base network for) every mask anew.
No network runs here.  Prints one JSON line per (photo, K).
"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hip_ext  # noqa: E402
from src.util.image_util import resize_bilinear_u8  # noqa: E402

S = 518


def photo(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 0.5 + 0.4 * np.sin(yy[..., None] * rng.uniform(0.001, 0.02, 3) + xx[..., None] * rng.uniform(0.001, 0.02, 3))
    return np.ascontiguousarray(np.clip(base * 255 + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8))


def masks(k, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(((yy - h * (0.3 + 0.05 * i)) / (h * 0.2)) ** 2 + ((xx - w * (0.3 + 0.05 * i)) / (w * 0.2)) ** 2 <= 1) for i in range(k)]).astype(np.uint8) * 255


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_prep(image_bgr, amodal_mask, device):
    """The host preparation of infer.py's _on_device_pipeline for one mask, copies included."""
    img518 = resize_bilinear_u8(image_bgr, S, S)
    rgb_raw = (torch.tensor(img518).permute(2, 0, 1).unsqueeze(0) / 255).to(device)
    rgb = F.interpolate(torch.tensor(image_bgr).unsqueeze(0).permute(0, 3, 1, 2) / 255, size=(S, S), mode="nearest").float().to(device)
    mask_ts = (F.interpolate(torch.tensor(amodal_mask).float()[None, None], size=(S, S), mode="nearest") > 0).float().to(device)
    return rgb_raw, rgb, mask_ts


def main():
    hip_ext.load()
    dev = "cuda"
    for h, w in ((480, 854), (1080, 1920), (2160, 3840)):
        img = photo(h, w)
        img_dev = torch.from_numpy(img).to(dev)
        raw, near = torch.empty(3, S, S, device=dev), torch.empty(3, S, S, device=dev)
        photo_ms = event_ms(lambda: hip_ext.photo_prep(img_dev, h, w, 3, w * 3, S, S, raw_out=raw, near_out=near), 50)
        h2d_photo_ms = event_ms(lambda: torch.from_numpy(img).to(dev), 10)
        for k in (1, 8):
            m = masks(k, h, w)
            m_dev = torch.from_numpy(m).to(dev)
            m01, pm1 = torch.empty(k, 1, S, S, device=dev), torch.empty(k, 1, S, S, device=dev)
            mask_ms = event_ms(lambda: hip_ext.mask_prep(m_dev, k, h, w, w, h * w, S, S, m01, pm1), 50)
            h2d_masks_ms = event_ms(lambda: torch.from_numpy(m).to(dev), 10)
            am, base = torch.rand(k, S, S, device=dev), torch.rand(k, S, S, device=dev)
            ss = torch.tensor([[0.9, 0.05]] * k, device=dev)
            out = torch.empty_like(am)
            blend_ms = event_ms(lambda: hip_ext.blend_ex(am, base, m01.reshape(k, S, S), out, ss), 50)
            maps = torch.rand(k + 1, S, S, device=dev)
            big = torch.empty(k + 1, h, w, device=dev)
            nearest_ms = event_ms(lambda: hip_ext.nearest_resize(maps, big), 50)
            reps = 3
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                for i in range(k):
                    host_prep(img, m[i] > 0, dev)
            torch.cuda.synchronize()
            host_ms = (time.perf_counter() - t0) * 1e3 / reps
            rec = dict(photo=[h, w], K=k, size=S, photo_prep_us=round(photo_ms * 1e3, 1), mask_prep_us=round(mask_ms * 1e3, 1),
                       blend_ex_us=round(blend_ms * 1e3, 1), nearest_resize_us=round(nearest_ms * 1e3, 1),
                       h2d_photo_ms=round(h2d_photo_ms, 3), h2d_masks_ms=round(h2d_masks_ms, 3),
                       device_prep_total_ms=round(photo_ms + mask_ms + h2d_photo_ms + h2d_masks_ms, 3),
                       host_prep_ms=round(host_ms, 2), host_prep_ms_per_mask=round(host_ms / k, 2),
                       nearest_resize_bytes=(k + 1) * (h * w + S * S) * 4)
            rec["nearest_resize_GBps"] = round(rec["nearest_resize_bytes"] / (nearest_ms * 1e6), 1)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
