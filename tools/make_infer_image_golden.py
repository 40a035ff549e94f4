"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/infer_image/ by running the REAL reference DepthAnythingV2.infer_image (RAW/dpt.py:186-221)
on the CPU, imported read-only through oracle/_refshim.py.  Run where the reference tree exists (it does not travel to the GPU machine):

    python tools/make_infer_image_golden.py              # fixtures + sizes.json + surface.json
    python tools/make_infer_image_golden.py vits_90x120  # one fixture

cv2 is not installed: after loading, the shim's cv2 stand-in gets resize / cvtColor / COLOR_BGR2RGB from tests/_cv2_cubic.py (the numpy
restatement of OpenCV's float INTER_CUBIC path), and the torchvision Compose stand-in of the raw dpt module is replaced by a real compose.
Everything else is the reference's own code: Resize.get_size, NormalizeImage, PrepareForNet, the forward and the final F.interpolate.
Weights: the synthetic fill of oracle/make_golden.py (build_reference) with its raw centring rule (final bias moved so that the logits
of this very input average 1.5).  Each fixture stores the uint8 input, input_size, the reference's output (every `stride`-th pixel) and
the meta in the schema tests/_cases.py rebuilds the product model from.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _cv2_cubic as C  # noqa: E402
from oracle import _refshim  # noqa: E402
from oracle import dav2_oracle as O  # noqa: E402
from oracle.make_golden import FINAL_BIAS_KEY, build_reference  # noqa: E402
from src.util.synth_weights import make_inputs  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "infer_image")
RAW_DPT = "_adaref_src.models.amodalsynthdrive.depth_anything_v2_raw.dpt"
RAW_TRANSFORM = "_adaref_src.models.amodalsynthdrive.depth_anything_v2_raw.util.transform"
VITS = dict(encoder="vits", features=64, out_channels=[48, 96, 192, 384])
VITL = dict(encoder="vitl", features=256, out_channels=[256, 512, 1024, 1024])
VITG = dict(encoder="vitg", features=384, out_channels=[1536, 1536, 1536, 1536])
# name -> (model, photo h, w, channels, input_size, image seed, output stride)
CASES = {
    "vits_90x120": (VITS, 90, 120, 3, 518, 1, 1),          # up-scaling, landscape: 518 x 686
    "vits_200x61_bgra": (VITS, 200, 61, 4, 266, 2, 1),     # tall, width-bound, BGRA input: 868 x 266
    "vits_160x208": (VITS, 160, 208, 3, 70, 3, 2),         # down-scaling; 91 / 14 = 6.5 rounds to even: 70 x 84
    "vitl_100x150": (VITL, 100, 150, 3, 518, 4, 1),        # the ladder's model; 777 / 14 = 55.5 rounds to even: 518 x 784
    "vitg_120x160": (VITG, 120, 160, 3, 224, 5, 1),        # infer.py's base-depth encoder: 224 x 294
}


class _Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, sample):
        for t in self.transforms:
            sample = t(sample)
        return sample


def install():
    """The reference's raw DepthAnythingV2 class with a working cv2 stand-in and Compose."""
    _, Raw = _refshim.load_reference()
    cv2 = sys.modules["cv2"]
    cv2.resize, cv2.cvtColor, cv2.COLOR_BGR2RGB = C.resize, C.cvt_color, C.COLOR_BGR2RGB
    sys.modules[RAW_DPT].Compose = _Compose
    return Raw


def photo(h, w, channels, seed):
    """A uint8 BGR(A) photo: image-like smooth colour (src.util.synth_weights structured inputs) with one hard-edged bright ellipse (the cubic
    kernel's overshoot at its border) that keeps 30 % of the texture under it, and, for BGRA, a random alpha channel that must not matter.
    (A FLAT ellipse, without texture, put raw ViT-G at 1.01e-3 against the reference: the forward's margin on large constant
    regions; not the preparation, which matches the restatement to 1e-5.)"""
    x, _, mask, _ = make_inputs(1, h, w, seed, style="structured")
    rgb = x[0].permute(1, 2, 0).numpy()
    inside = mask[0, 0].numpy() > 0
    rgb[inside] = 0.7 * np.array([0.95, 0.9, 0.1]) + 0.3 * rgb[inside]
    bgr = np.round(rgb[..., ::-1] * 255.0).clip(0, 255).astype(np.uint8)
    if channels == 4:
        alpha = np.random.default_rng(seed).integers(0, 256, size=(h, w, 1), dtype=np.uint8)
        bgr = np.concatenate([bgr, alpha], axis=2)
    return np.ascontiguousarray(bgr)


@torch.no_grad()
def generate(name):
    Raw = install()
    model_cfg, h, w, channels, input_size, seed, stride = CASES[name]
    case = dict(kind="raw", **model_cfg)
    m, sd = build_reference(case)
    assert isinstance(m, Raw)
    img = photo(h, w, channels, seed)
    x, _ = m.image2tensor(img, input_size)
    tr = {}
    O.raw_forward(sd, case["encoder"], x, trace=tr)
    key = FINAL_BIAS_KEY["raw"]
    sd[key] = sd[key] - (float(tr["logits"].mean()) - 1.5)
    m.load_state_dict(sd, strict=True)
    ref = m.infer_image(img, input_size)
    assert ref.dtype == np.float32 and ref.shape == (h, w), (ref.dtype, ref.shape)
    meta = dict(case=case, final_bias=float(sd[key].item()), final_bias_key=key, input_size=input_size, network_size=list(x.shape[-2:]),
                stride=stride, out_shape=list(ref.shape), out_mean=float(ref.mean()), out_abs_mean=float(np.abs(ref).mean()),
                out_zero_fraction=float((ref == 0).mean()), torch=torch.__version__)
    os.makedirs(OUT_DIR, exist_ok=True)
    np.savez_compressed(os.path.join(OUT_DIR, name + ".npz"), image=img, input_size=np.int32(input_size),
                        out=np.ascontiguousarray(ref[::stride, ::stride]), meta=json.dumps(meta))
    print(f"{name}: {h}x{w}x{channels} -> network {tuple(x.shape[-2:])}, out mean {meta['out_mean']:.4f}, "
          f"zero fraction {meta['out_zero_fraction']:.3f}, {os.path.getsize(os.path.join(OUT_DIR, name + '.npz'))} bytes")


def write_sizes():
    """[h, w, input_size, H, W] from the reference's own Resize.get_size for the configuration image2tensor uses, over a grid, random sizes
    up to 8K and every half-way tie (x / 14 = k + 0.5 exactly in float64, where np.round goes to the even k) found in a scan."""
    install()
    Resize = sys.modules[RAW_TRANSFORM].Resize
    rows = set()
    rng = np.random.default_rng(0)
    sizes = (518, 266, 224, 70, 14, 1022)
    for s in sizes:
        resize = Resize(width=s, height=s, resize_target=False, keep_aspect_ratio=True, ensure_multiple_of=14, resize_method="lower_bound",
                        image_interpolation_method=2)
        pairs = {(1, 1), (1, 4000), (4000, 1), (1080, 1920), (2160, 3840), (1920, 1080), (160, 208), (100, 150), (90, 120), (200, 61), (120, 160)}
        pairs |= {(int(a), int(b)) for a, b in np.exp(rng.uniform(0, np.log(8000), size=(300, 2)))}
        ties = 0
        for a in range(1, 400):
            for b in range(1, 400):
                sc = max(s / a, s / b)
                if ((sc * a) / 14) % 1 == 0.5 or ((sc * b) / 14) % 1 == 0.5:
                    pairs.add((a, b))
                    ties += 1
                    if ties >= 150:
                        break
            if ties >= 150:
                break
        for a, b in pairs:
            W, H = resize.get_size(b, a)
            rows.add((a, b, s, int(H), int(W)))
    rows = sorted(rows, key=lambda r: (r[2], r[0], r[1]))
    with open(os.path.join(OUT_DIR, "sizes.json"), "w") as f:
        json.dump(rows, f, separators=(",", ":"))
    print(f"sizes.json: {len(rows)} rows")


def write_surface():
    """Public methods of the reference's raw DepthAnythingV2 with their signatures."""
    import inspect
    Raw = install()
    surf = {n: [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in inspect.signature(v).parameters.values()]
            for n, v in sorted(vars(Raw).items()) if callable(v) and not n.startswith("_")}
    with open(os.path.join(OUT_DIR, "surface.json"), "w") as f:
        json.dump(surf, f, indent=1)
    print("surface.json:", sorted(surf))


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    names = sys.argv[1:] or (list(CASES) + ["sizes", "surface"])
    for n in names:
        if n == "sizes":
            write_sizes()
        elif n == "surface":
            write_surface()
        else:
            generate(n)
