"""Step counts and times of the membrane solve on the device (csrc/ada_membrane.hip, hip_ext.inpaint.fill_harmonic), on the device this runs on.

    python tools/profile_membrane.py [--out FILE] [--tol 1e-9]

Three problems at 518 x 518 and 1022 x 1022, B = 1, C = 1, on a smooth ramp plus noise:
    disc     a centred disc of a third of the shorter side is unknown, everything else known (a hole of fill_smooth's profile);
    object   the domain is an elliptical object mask whose upper half is known (visible) and whose lower half is unknown: the amodal blend's problem;
    sparse   0.1 % of the pixels are known, the whole image is the domain.
Each with the zero start and with fill_smooth's values as the start.  Per row: the unknowns, the steps the device took to the freeze at ``--tol``, the
true residual it reports, microseconds per step (HIP events around one ada_membrane_iterate_fwd of min(steps, 200) steps issued right after begin, while
no plane is frozen: two launches per step) and per solve (begin, exactly the steps it needs, end; the start's push-pull fill is not included), each the
median of three repetitions with their min-max, and the bytes a step must move once (``step_bytes`` below).  There is no CPU path: without a device
the tool fails."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = ((518, 518), (1022, 1022))


def step_bytes(n_domain, n_unknown):
    """Bytes one step moves when every vector is read or written once per use: the direction launch reads the code, r and p and writes p' and q over the
    unknowns (the halo re-reads are cache hits at best and not counted); the update launch reads the code, p', q, u, r and writes u and r."""
    return n_domain * 2 + n_unknown * 8 * (2 + 2) + n_unknown * 8 * (4 + 2)


def scene(kind, h, w):
    rng = np.random.default_rng(h)
    yy, xx = np.mgrid[0:h, 0:w]
    x = (1.0 + 0.002 * xx + 0.001 * yy + rng.normal(0, 0.05, (h, w))).astype(np.float32)
    if kind == "disc":
        r = min(h, w) / 3.0
        return x, ((yy - h / 2.0) ** 2 + (xx - w / 2.0) ** 2) > r * r, np.ones((h, w), bool)
    if kind == "object":
        domain = ((yy - h / 2.0) / (0.3 * h)) ** 2 + ((xx - w / 2.0) / (0.2 * w)) ** 2 <= 1.0
        return x, domain & (yy < h / 2.0), domain
    known = rng.random((h, w)) < 0.001
    known[0, 0] = True
    return x, known, np.ones((h, w), bool)


def timed(fn, reps=3):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tol", type=float, default=1e-9)
    args = ap.parse_args()
    import hip_ext
    from hip_ext import inpaint
    hip_ext.load()
    assert torch.cuda.is_available(), "profile_membrane needs a HIP device"
    prop = torch.cuda.get_device_properties(0)
    lines = [f"device: {prop.name} ({getattr(prop, 'gcnArchName', '?')}), {prop.multi_processor_count} CUs; tol {args.tol:g}; B = 1, C = 1; us = median of three [min-max]; "
             f"a step is two launches; cap = default_max_iter(h, w)"]
    for h, w in SIZES:
        for kind in ("disc", "object", "sparse"):
            x_host, known, domain = scene(kind, h, w)
            x = torch.from_numpy(x_host).cuda()[None, None].contiguous()
            k8, d8 = torch.from_numpy(known.astype(np.uint8)).cuda()[None], torch.from_numpy(domain.astype(np.uint8)).cuda()[None]
            unknown = int((domain & ~known).sum())
            ws = torch.empty(hip_ext.membrane_workspace_bytes(1, 1, h, w), dtype=torch.uint8, device="cuda")
            out = torch.empty_like(x)
            res = torch.empty(1, dtype=torch.float64, device="cuda")
            it = torch.empty(1, dtype=torch.int32, device="cuda")
            cv = torch.empty(1, dtype=torch.uint8, device="cuda")
            smooth = torch.empty_like(x)
            hip_ext.push_pull(x, k8 & d8, smooth, 0.0)
            for guess_name, guess in (("zero", None), ("smooth", smooth)):
                def solve(n):
                    hip_ext.membrane_begin(x, k8, ws, domain=d8, guess=guess, tol=args.tol)
                    hip_ext.membrane_iterate(x, ws, n)
                    hip_ext.membrane_end(x, ws, res, it, cv, out=out)
                solve(inpaint.default_max_iter(h, w))
                steps, ok, r = int(it.item()), int(cv.item()), float(res.item())
                few = max(min(steps, 200), 1)
                hip_ext.membrane_begin(x, k8, ws, domain=d8, guess=guess, tol=args.tol)
                torch.cuda.synchronize()

                def some_steps():
                    hip_ext.membrane_begin(x, k8, ws, domain=d8, guess=guess, tol=args.tol)
                    hip_ext.membrane_iterate(x, ws, few)
                begin_only = timed(lambda: hip_ext.membrane_begin(x, k8, ws, domain=d8, guess=guess, tol=args.tol))[0]
                sm, slo, shi = ((t - begin_only) / few for t in timed(some_steps))
                tm, tlo, thi = timed(lambda: solve(steps))
                lines.append(f"{h} x {w}  {kind:7s} guess {guess_name:6s} unknowns {unknown:8d}  steps {steps:6d} (cap {inpaint.default_max_iter(h, w)}) converged {ok} "
                             f"residual {r:.2e}   us/step {sm:7.1f} [{slo:.1f}-{shi:.1f}]   us/solve {tm:10.1f} [{tlo:.1f}-{thi:.1f}]   "
                             f"bytes/step {step_bytes(int(domain.sum()), unknown)}")
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
