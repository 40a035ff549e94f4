"""Cost of the raw model's infer_image on photo-sized inputs: raw ViT-L (synthetic weights), a 1080p and a 4K uint8 BGR photo.

    python tools/profile_infer_image.py                                                   # device-event timings
    rocprofv3 --kernel-trace --stats -d OUT -o infer_image -- python tools/profile_infer_image.py   # + the per-kernel table

For each photo: the whole call (host clock; it ends in the copy of the depth map to the host, the call's one synchronisation), and with HIP
events the prep kernel (ada_image_prep_fwd) and the depth resize (ada_depth_resize_fwd) alone, the host-to-device copy of the photo and the
device-to-host copy of the map.  Prints one JSON line per photo.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hip_ext  # noqa: E402
from hip_ext.image import PIXEL_MEAN, PIXEL_STD, network_size, resize_depth  # noqa: E402
from src.models.amodalsynthdrive.depth_anything_v2_raw.dpt import DepthAnythingV2  # noqa: E402
from src.util.synth_weights import fill_state_dict_  # noqa: E402


def photo(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 0.5 + 0.4 * np.sin(yy[..., None] * rng.uniform(0.001, 0.02, 3) + xx[..., None] * rng.uniform(0.001, 0.02, 3))
    return np.ascontiguousarray(np.clip(base * 255 + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8))


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    hip_ext.load()
    m = DepthAnythingV2(encoder="vitl", features=256, out_channels=(256, 512, 1024, 1024)).eval()
    sd = m.state_dict()
    fill_state_dict_(sd, 0)
    # the final bias of the ViT-L infer_image fixture (same fill): a centred map, as a real checkpoint gives, not one the ladder re-runs
    meta = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "infer_image", "vitl_100x150.npz"))["meta"]))
    sd[meta["final_bias_key"]].fill_(meta["final_bias"])
    m.load_state_dict(sd)
    m = m.cuda()
    for h, w in ((1080, 1920), (2160, 3840)):
        img = photo(h, w)
        H, W = network_size(h, w)
        for _ in range(3):
            m.infer_image(img)
        reps = 10
        t0 = time.perf_counter()
        for _ in range(reps):
            m.infer_image(img)
        call_ms = (time.perf_counter() - t0) * 1e3 / reps
        dev = torch.from_numpy(img).cuda()
        x = torch.empty(1, 3, H, W, device="cuda")
        prep_ms = event_ms(lambda: hip_ext.image_prep(dev, 1, h, w, 3, w * 3, h * w * 3, H, W, PIXEL_MEAN, PIXEL_STD, x), 50)
        depth = m.forward(x, normalise_input=False)
        out = torch.empty(1, h, w, device="cuda")
        resize_ms = event_ms(lambda: hip_ext.depth_resize(depth, out), 50)
        h2d_ms = event_ms(lambda: torch.from_numpy(img).to("cuda"), 10)
        d2h_ms = event_ms(lambda: resize_depth(depth, h, w)[0].cpu(), 10) - resize_ms
        fwd_ms = event_ms(lambda: m.forward(x, normalise_input=False), 10)
        rec = dict(photo=[h, w], network=[H, W], call_ms=round(call_ms, 3), forward_ms=round(fwd_ms, 3), prep_us=round(prep_ms * 1e3, 1),
                   depth_resize_us=round(resize_ms * 1e3, 1), h2d_photo_ms=round(h2d_ms, 3), d2h_map_ms=round(d2h_ms, 3),
                   kernels_share_of_call=round((prep_ms + resize_ms) / call_ms, 4),
                   prep_bytes=h * w * 3 + 3 * H * W * 4, depth_resize_bytes=H * W * 4 + h * w * 4)
        rec["prep_GBps"] = round(rec["prep_bytes"] / (prep_ms * 1e6), 1)
        rec["depth_resize_GBps"] = round(rec["depth_resize_bytes"] / (resize_ms * 1e6), 1)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
