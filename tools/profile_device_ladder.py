#!/usr/bin/env python
"""What the precision ladder's device mode (module.ladder_on_device) costs, recorded into profiles/device_ladder.txt:

  (a) ViT-L, 32 x 518 x 518 on the benchmarked weights and inputs: ms / step and the allocator's peak memory in the eager default mode, device mode True and "head";
  (b) one ViT-B and one ViT-L image: eager default, device mode as plain launches, device mode captured into the caller's graph and replayed;
  (c) ViT-B, 8 x 518 x 518 (config 2): default against device "head", which removes the per-call host read.

    python tools/profile_device_ladder.py [a] [b] [c] [--out profiles/device_ladder.txt]

Nothing in the test-suite depends on these numbers.  Each measurement: warm-up, then blocks of steps between device synchronisations, best and median block."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from hip_ext import engine as E  # noqa: E402
from src.models import get_model  # noqa: E402
from src.util.synth_weights import centred_final_bias, fill_state_dict_, make_inputs  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def build(enc):
    m = get_model("AmodalDAv2", guide_type="mask+observation", loss_stategy="entire_target_object", encoder=enc, pretrained=False).eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    fill_state_dict_(sd, 0)
    cb = centred_final_bias(enc, ROOT)      # the benchmark's logit-centring bias: the maps span (0, 1), the default path stays on the first rung
    if cb:
        sd[cb[0]] = torch.full_like(sd[cb[0]], cb[1])
    m.load_state_dict(sd)
    return m.cuda()


def timed(fn, warmup, blocks, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    return min(ms), statistics.median(ms)


def modes(m, x, mask, obs, which, warmup, blocks, steps, label):
    enc = m.encoder

    def fn():
        with torch.no_grad():
            return m(x, guide_rgb=None, guide_mask=mask, observation=obs)
    base = None
    for mode in which:
        enc.ladder_on_device = mode
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        best, med = timed(fn, warmup, blocks, steps)
        peak = torch.cuda.max_memory_allocated()
        eng = enc._engine()
        rep = eng.device_ladder_report() if mode is not False else None
        books = (f"device rungs of the last call {sorted(set(rep['rungs'].tolist()))}, unserved so far {rep['unserved']}" if rep else
                 f"escalated so far {eng.escalated}")
        base = best if base is None else base
        say(f"{label} ladder_on_device = {mode!r:7}: {best:8.2f} ms / step best, {med:8.2f} median ({x.shape[0] / best * 1e3:7.1f} images/s; x {best / base:4.2f} of the first row); "
            f"allocator peak {peak / 2**30:6.2f} GiB (held before the block {before / 2**30:5.2f}); {books}")
    enc.ladder_on_device = False


def captured(m, x, mask, obs, warmup, blocks, steps, label):
    enc = m.encoder
    enc.ladder_on_device = True
    with torch.no_grad():
        for _ in range(3):
            m(x, guide_rgb=None, guide_mask=mask, observation=obs)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m(x, guide_rgb=None, guide_mask=mask, observation=obs)
    best, med = timed(g.replay, warmup, blocks, steps)
    enc.ladder_on_device = False
    with torch.no_grad():
        same = torch.equal(out, m(x, guide_rgb=None, guide_mask=mask, observation=obs))
    say(f"{label} device mode, captured by the caller and replayed: {best:8.2f} ms / step best, {med:8.2f} median; replayed == eager default mode: {same}")
    del g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["a", "b", "c"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_ladder.txt"))
    a = ap.parse_args()
    say(f"# tools/profile_device_ladder.py {' '.join(a.parts)} -- {torch.cuda.get_device_name(0)}, torch {torch.__version__}; ADA_GRAPH={E.GRAPH_MODE}")
    if "a" in a.parts:
        say("\n## (a) ViT-L, 32 x 518 x 518, benchmarked weights and inputs (make_inputs seed 100): every image stays on the first rung")
        m = build("vitl")
        x, _, mask, obs = make_inputs(32, 518, 518, seed=100, device="cuda")
        modes(m, x, mask, obs, (False, "head", True), 3, 3, 5, "ViT-L bs=32")
        del m, x, mask, obs
        torch.cuda.empty_cache()
    if "b" in a.parts:
        say("\n## (b) one 518 x 518 image")
        for enc in ("vitb", "vitl"):
            m = build(enc)
            x, _, mask, obs = make_inputs(1, 518, 518, seed=100, device="cuda")
            modes(m, x, mask, obs, (False, "head", True), 5, 3, 20, f"{enc} bs=1")
            captured(m, x, mask, obs, 5, 3, 20, f"{enc} bs=1")
            del m
            torch.cuda.empty_cache()
    if "c" in a.parts:
        say("\n## (c) ViT-B, 8 x 518 x 518 (config 2): the default mode reads the statistics back every call, device \"head\" does not")
        m = build("vitb")
        x, _, mask, obs = make_inputs(8, 518, 518, seed=100, device="cuda")
        modes(m, x, mask, obs, (False, "head", True), 5, 3, 20, "ViT-B bs=8")
        old = m.encoder.precision_ladder if hasattr(m.encoder, "precision_ladder") else None
        m.encoder.precision_ladder = False
        modes(m, x, mask, obs, (False,), 5, 3, 20, "ViT-B bs=8, precision_ladder = False,")
        m.encoder.precision_ladder = old
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if os.path.exists(a.out) else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
