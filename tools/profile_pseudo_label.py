"""Cost of generating ADIW pseudo-labels on the device (hip_ext/labels.py, src/scripts/sam_pl_gen_dav2.py).

    python tools/profile_pseudo_label.py > profiles/pseudo_label.txt

Two measurements, one JSON line each kind:

  * "prep": the preparation of ONE 1500 x 2250 photo (the usual SA-1B size) to the network's 518 x 518 fp32 planes, and of one mask of that size to
    the 0 / 1 mask.  Device: pil_resize on pixels already in HBM (HIP events; warm-up, then three windows of >= 0.25 s: median and min-max), and
    from a host numpy array, the host -> device copy and the allocations included (host clock around a synchronise).  Host: what load_im and lines
    93-94 of the reference do after decoding, ``Image.resize((518, 518), BICUBIC)`` then ``np.array(im) / 255`` cast to float32 (``> 0`` for the mask),
    host clock, same windows.  Pillow's resize runs on one core; the figure is one process.  The bytes are compared before anything is timed.
  * "run": pairs per second of the runner's ``run()`` -- decode on the host, preparation, ONE raw ViT-G batch of 2 P at 518, fit, paste, quantise,
    device -> host copy of the labels, PNG encode -- over N synthetic samples (1500 x 2250 JPEG photos and PNG composites / masks written to a
    temporary directory), synthetic weights, for two batch sizes with 8 decode threads and for the larger one with 1, alternating, three passes each
    after a warm-up pass: median and min-max.  "decode_s" is the host clock over the four loaders of the same N samples alone, on one thread: the host
    work of a pass that the decode threads hide behind the device or spread over cores.

No network weights ship with the repository.  With the synthetic fill the precision ladder re-runs every image of these batches on
its third rung, the whole forward in split precision, so the network's share of a pass is an upper bound for a checkpoint that stays on the first rung.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hip_ext  # noqa: E402
from hip_ext.labels import pil_resize  # noqa: E402
from src.scripts import sam_pl_gen_dav2 as G  # noqa: E402

WINDOW_S = 0.25


def photo(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.4 * np.sin(yy[..., None] * rng.uniform(0.002, 0.02, 3) + xx[..., None] * rng.uniform(0.002, 0.02, 3))
    return np.clip(base * 255 + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def masks(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = h * rng.uniform(0.4, 0.6), w * rng.uniform(0.4, 0.6)
    whole = ((((yy - cy) / (h * 0.25)) ** 2 + ((xx - cx) / (w * 0.2)) ** 2) <= 1).astype(np.uint8) * 255
    return whole * (xx < cx + w * 0.05).astype(np.uint8), whole


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def windows(fn, clock, rounds=3):
    for _ in range(3):
        fn()
    reps = int(min(max(WINDOW_S * 1e3 / max(clock(fn, 3), 1e-3), 3), 5000))
    v = [clock(fn, reps) for _ in range(rounds)]
    return dict(ms=round(statistics.median(v), 4), ms_min_max=[round(min(v), 4), round(max(v), 4)], reps=reps)


def profile_prep(h, w, size):
    img = photo(h, w, 0)
    mask = masks(h, w, 1)[1]
    dev_img, dev_mask = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    want = np.asarray(Image.fromarray(img).resize((size, size), Image.BICUBIC))
    want_m = np.asarray(Image.fromarray(mask).resize((size, size), Image.BICUBIC))
    diff = int((pil_resize(dev_img, (size, size)).cpu().numpy() != want).sum()) + int((pil_resize(dev_mask, (size, size)).cpu().numpy() != want_m).sum())
    assert diff == 0, f"{diff} bytes differ from Pillow {Image.__version__}"
    rec = dict(kind="prep", photo=[h, w], size=size, pillow=Image.__version__, bytes_differing_from_pillow=diff)
    rec["photo_device_resident"] = windows(lambda: pil_resize(dev_img, (size, size), out="float"), event_ms)
    rec["photo_device_from_host_array"] = windows(lambda: pil_resize(img, (size, size), out="float", device="cuda"), host_ms)
    rec["photo_pillow_host"] = windows(lambda: (np.array(Image.fromarray(img).resize((size, size), Image.BICUBIC)) / 255).astype(np.float32), host_ms)
    rec["mask_device_resident"] = windows(lambda: pil_resize(dev_mask, (size, size), out="mask"), event_ms)
    rec["mask_device_from_host_array"] = windows(lambda: pil_resize(mask, (size, size), out="mask", device="cuda"), host_ms)
    rec["mask_pillow_host"] = windows(lambda: np.asarray(Image.fromarray(mask).resize((size, size), Image.BICUBIC)) > 0, host_ms)
    print(json.dumps(rec), flush=True)


def write_samples(root, n, h, w):
    dirs = {k: os.path.join(root, k) for k in ("image", "occ", "visible", "whole")}
    for d in dirs.values():
        os.makedirs(d)
    ids = [str(1000 + i) for i in range(n)]
    for i, sid in enumerate(ids):
        img = photo(h, w, 10 + i)
        vis, whole = masks(h, w, 100 + i)
        occ = img.copy()
        occ[(whole > 0) & (vis == 0)] = (40, 180, 90)
        p = G.sample_paths(sid, dirs["image"], dirs["occ"], dirs["visible"], dirs["whole"], os.path.join(root, "out"))
        Image.fromarray(img).save(p["image"], quality=90)
        Image.fromarray(occ).save(p["occ"], compress_level=1)
        Image.fromarray(vis).save(p["visible"])
        Image.fromarray(whole).save(p["whole"])
    return ids, dirs


def profile_run(encoder, size, n, h, w, variants, rounds=3):
    with tempfile.TemporaryDirectory() as root:
        ids, d = write_samples(root, n, h, w)
        out = os.path.join(root, "out")
        model = G.load_model(encoder, None, "cuda")

        def one_pass(variant):
            bs, workers = variant
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = G.run(model, ids, d["image"], d["occ"], d["visible"], d["whole"], out, batch_size=bs, size=size, decode_workers=workers)
            torch.cuda.synchronize()
            assert res["samples"] == n
            return time.perf_counter() - t0

        t0 = time.perf_counter()
        for sid in ids:
            p = G.sample_paths(sid, d["image"], d["occ"], d["visible"], d["whole"], out)
            G.load_photo(p["image"]), G.load_photo(p["occ"]), G.load_mask(p["visible"]), G.load_mask(p["whole"])
        decode_s = time.perf_counter() - t0
        for v in variants:
            one_pass(v)                       # warm-up: every shape of the timed passes
        secs = {v: [] for v in variants}
        for _ in range(rounds):
            for v in variants:
                secs[v].append(one_pass(v))
        label = np.asarray(Image.open(os.path.join(out, f"{ids[0]}_depth.png")))
        assert label.dtype == np.uint16 and label.shape == (512, 512)
        for (bs, workers), v in secs.items():
            print(json.dumps(dict(kind="run", encoder=encoder, size=size, photo=[h, w], samples=n, batch_pairs=bs, network_batch=2 * bs, decode_workers=workers,
                                  pairs_per_s=round(n / statistics.median(v), 2), pairs_per_s_min_max=[round(n / max(v), 2), round(n / min(v), 2)],
                                  pass_s=round(statistics.median(v), 3), decode_s=round(decode_s, 3), rounds=rounds)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder", default="vitg")
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--photo", type=int, nargs=2, default=(1500, 2250))
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--variants", type=int, nargs="+", default=(2, 8, 8, 8, 8, 1), help="pairs of (pairs per batch, decode threads)")
    a = ap.parse_args()
    hip_ext.load()
    assert torch.cuda.is_available(), "a measurement needs the device"
    profile_prep(a.photo[0], a.photo[1], a.size)
    profile_run(a.encoder, a.size, a.samples, a.photo[0], a.photo[1], list(zip(a.variants[0::2], a.variants[1::2])))


if __name__ == "__main__":
    main()
