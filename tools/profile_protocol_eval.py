"""Device time of the paper-protocol evaluation (ada_protocol_fit_fwd + ada_protocol_eval_fwd) next to the legacy evaluation of the same batch
(scale_shift_least_square + depth_eval: two passes of ada_depth_eval_fwd), on the device this runs on.

    python tools/profile_protocol_eval.py [--out profiles/protocol_eval_kernels.txt] [--iters 200]

Timing: HIP events around ``iters`` back-to-back calls after a warm-up of the same shape, the two variants alternating in rounds inside one
process; median and minimum over the rounds.  Outputs stay on the device (no host read inside the timed window).  Calls rotate over four
batches of inputs: the 32-image batch reads 86 MB per pass, which the 256 MiB Infinity Cache would otherwise serve on every call but the first
(the one-image batch stays cache-resident whatever is done: its figure is launch latency).  The traffic bound next to each
figure is the bytes the pass must read -- two fp32 maps and two byte masks, 10 B per pixel -- over the HBM peak.  There is no CPU path: without a
device the tool fails."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12      # bytes / s, MI355X


def scene(B, h, w, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    gt = torch.rand(B, h, w, device="cuda", generator=g) * 0.8 + 0.1
    obs = gt + 0.01 * torch.randn(B, h, w, device="cuda", generator=g)
    pred = ((gt - 0.05) / 1.5 + 0.01 * torch.randn(B, h, w, device="cuda", generator=g)).clamp_min(0.01)
    whole = torch.zeros(B, h, w, dtype=torch.bool, device="cuda")
    whole[:, h // 6:h - h // 6, w // 8:w - w // 8] = True
    rows = torch.arange(h, device="cuda").view(1, h, 1)
    visible = whole & (rows < h * 0.55)
    return pred, gt, obs, whole.view(torch.uint8), visible.view(torch.uint8), (whole & ~visible).view(torch.uint8), (gt > 0).view(torch.uint8)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "protocol_eval_kernels.txt"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import hip_ext as H
    from src.util import alignment
    H.load()
    assert torch.cuda.is_available(), "profile_protocol_eval needs a HIP device"
    lines = [f"paper-protocol evaluation kernels on {torch.cuda.get_device_name(0)}; {a.iters} calls per round, {a.rounds} rounds, variants alternating; us per call",
             "traffic bound: 10 B per pixel and pass (two fp32 maps, two byte masks) over 8.0 TB/s", ""]
    for B in (32, 1):
        h = w = 518
        scenes = [scene(B, h, w, 10 * B + k) for k in range(4)]
        ws = torch.empty(H.protocol_workspace_bytes(B, h, w) // 8, dtype=torch.float64, device="cuda")
        legacy_masks = [(s[3] != 0) & (s[1] > 0) for s in scenes]
        state = {"fit": H.protocol_fit(scenes[0][0], scenes[0][2], scenes[0][4], scenes[0][3], workspace=ws)}

        def fit(i):
            pred, gt, obs, whole, visible, region, valid = scenes[i % 4]
            state["fit"] = H.protocol_fit(pred, obs, visible, whole, workspace=ws)

        def ev(i):
            pred, gt, obs, whole, visible, region, valid = scenes[i % 4]
            H.protocol_eval(pred, gt, region, valid, state["fit"], workspace=ws)

        def both(i):
            fit(i)
            ev(i)

        def legacy(i):
            pred, gt = scenes[i % 4][:2]
            ss = alignment.scale_shift_least_square(gt, pred, legacy_masks[i % 4])
            H.depth_eval(pred, gt, legacy_masks[i % 4], scale_shift=ss.float().contiguous(), clip=(1e-3, 1.0))

        variants = (("protocol_fit", fit), ("protocol_eval", ev), ("protocol fit + eval", both), ("legacy fit + eval", legacy))
        for _, fn in variants:
            timed(fn, 20)
        res = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            for name, fn in variants:
                res[name].append(timed(fn, a.iters))
        bound = 10.0 * B * h * w / HBM_PEAK * 1e6
        lines.append(f"{B} x {h} x {w}   ({10.0 * B * h * w / 1e6:.1f} MB per pass, {bound:.2f} us at the HBM peak)")
        for name, _ in variants:
            med, lo = statistics.median(res[name]), min(res[name])
            passes = 2 if "+" in name else 1
            lines.append(f"  {name:22s} median {med:9.2f}   min {lo:9.2f}   traffic bound {passes * bound:7.2f}   ({passes * bound / med * 100:5.1f} % of it at the median)")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
