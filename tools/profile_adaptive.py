"""Size and time of the adaptive meshes (csrc/ada_adaptive.hip) behind hip_ext.geometry.adaptive_triangles, on the device this runs on.

    python tools/profile_adaptive.py [--out profiles/adaptive_mesh.txt] [--window 0.3] [--shapes N] [--bench LABEL=FILE ...]

Maps of 518 x 518 and 2072 x 2072 of seeded synthetic depth whose relief does not depend on the resolution: a tilted ground plane (linear in
disparity), a smooth wave, four depth steps and an elliptic object in front, masked out of the scene (its own mesh would be a second layer).  Meshed with
max_ratio=1.5 and the mask, swept over the tolerance; per tolerance:
  triangles        rows kept, against the full grid's create_triangles count
  adaptive         ada_mesh_adaptive_fwd, error phase and emission, into a buffer of the full grid's capacity (no host read), workspace allocated once
  emit_only        the same with the error map of an earlier call (error_ready): what one more tolerance of a sweep costs
  create           ada_mesh_triangles_fwd on the same map (the row ``full`` holds it once)
  render           the identity view through ada_mesh_project_fwd + ada_mesh_raster_fwd of the mesh with all h w points, no colours
Every time is the median of three windows of HIP events around back-to-back calls on resident buffers, in microseconds per call, with the windows'
min-max.  The 518 x 518 mesh at the first tolerance is also compared, row for row, with tests/_adaptive_ref.py when that file is there.
Not measured: the compacted forms (mesh_compact), PLY sizes, real network output (the relief is synthetic), any other camera than the identity view,
and counters (bytes moved, occupancy).  ``--bench``: JSON result lines of bench.py copied into the file.  There is no CPU path."""
import argparse
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

SHAPES = ((518, 518), (2072, 2072))
TAUS = (0.0, 0.001, 0.003, 0.01, 0.03, 0.1)
RATIO = 1.5


def windows(fn, seconds):
    """Median and min-max, in microseconds per call, of three windows of about ``seconds`` of HIP events around back-to-back calls."""
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
    return {"us": round(statistics.median(out), 1), "us_min_max": [round(min(out), 1), round(max(out), 1)], "reps": reps}


def scene(h, w):
    """(depth fp32 [h, w], mask uint8 [h, w]) of the seeded relief."""
    rng = np.random.default_rng(518)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = xx / float(w), yy / float(h)
    omega = 0.15 + 0.35 * v + 0.05 * u                                  # the ground: linear in disparity
    omega = omega + 0.02 * np.sin(25.0 * u) * np.cos(19.0 * v)            # a smooth wave
    omega = omega + 0.08 * ((np.floor(u * 4.0) % 2) * (v < 0.6))         # four steps in the upper part
    omega = omega + rng.uniform(0.0, 2e-5, size=(h, w))                  # the network's fine grain
    obj = ((u - 0.55) / 0.18) ** 2 + ((v - 0.62) / 0.25) ** 2 <= 1.0
    mask = (~obj).astype(np.uint8)
    return (1.0 / omega).astype(np.float32), mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_mesh.txt"))
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="how many of the shapes to run, in the order above")
    ap.add_argument("--bench", nargs="*", default=[], help="label=file pairs: the last JSON line of each file (a bench.py run) is recorded")
    a = ap.parse_args()
    import hip_ext as H
    from hip_ext import geometry as G
    H.load()
    assert torch.cuda.is_available(), "profile_adaptive needs a HIP device"
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# adaptive depth-map meshes on {prop.name}: arch {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB "
             "(csrc/ada_adaptive.hip, hip_ext/geometry.py)",
             "# python tools/profile_adaptive.py",
             f"# us per call: median of three windows of about {a.window} s (and their min-max) of HIP events around back-to-back calls, resident buffers, workspace allocated once.",
             f"# Synthetic seeded relief (tilted ground linear in disparity, smooth wave, four steps, a masked elliptic object), mask and max_ratio={RATIO} in every row.",
             "# adaptive = ada_mesh_adaptive_fwd (error phase + emission, capacity of the full grid, no host read); emit_only = the same with error_ready;",
             "# create = ada_mesh_triangles_fwd; render = ada_mesh_project_fwd + ada_mesh_raster_fwd, identity view at the map's size, all h w points, no colours.",
             f"# Virtual grid: the enclosing power-of-two square (518 -> N = 1024, 2072 -> N = 4096); levels with <= {H.ADAPT_FOLD} midpoints share one workgroup; subtrees of {H.ADAPT_CELL}-wide cells.",
             "# NOT measured: mesh_compact and PLY sizes, real network output, other views than the identity, counters (bytes, occupancy).  No bar was fixed in advance."]
    for h, w in SHAPES[:a.shapes]:
        depth_np, mask_np = scene(h, w)
        depth, mask = torch.from_numpy(depth_np[None]).cuda(), torch.from_numpy(mask_np[None]).cuda()
        cap = 2 * (h - 1) * (w - 1)
        tri = torch.empty(1, cap, 3, dtype=torch.int32, device="cuda")
        count = torch.empty(1, dtype=torch.int32, device="cuda")
        err = torch.empty(1, h, w, dtype=torch.float64, device="cuda")
        ws_a = torch.empty((H.mesh_adaptive_workspace_bytes(h, w) + 15) // 16 * 2, dtype=torch.int64, device="cuda")
        ws_t = torch.empty(H.mesh_triangles_workspace_bytes(1, h, w) // 4 + 1, dtype=torch.int32, device="cuda")
        points = G.depth_to_points(depth[0], dtype=torch.float32).reshape(-1, 3)
        K = G.get_intrinsics(h, w)
        cam = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]] + list(np.eye(3).reshape(-1)) + [0.0, 0.0, 0.0]
        V = h * w
        x = torch.empty(V, dtype=torch.int32, device="cuda")
        y = torch.empty(V, dtype=torch.int32, device="cuda")
        wv = torch.empty(V, dtype=torch.float64, device="cuda")
        out_d = torch.empty(h, w, dtype=torch.float32, device="cuda")
        out_i = torch.empty(h, w, dtype=torch.int32, device="cuda")
        ws_r = torch.empty((H.mesh_raster_workspace_bytes(h, w, cap) + 15) // 16 * 2, dtype=torch.int64, device="cuda")

        def render(t):
            H.mesh_project(points, cam, x, y, wv, pose=False)
            H.mesh_raster(x, y, wv, t, h, w, out_d, out_i, workspace=ws_r)

        create = lambda: H.mesh_triangles(1, h, w, tri, count, mask=mask, row_pitch=w, image_stride=h * w, depth=depth, max_ratio=RATIO, workspace=ws_t)
        create()
        n_full = int(count.item())
        full = tri[0, :n_full].clone()
        row = {"map": [h, w], "mesh": "full", "triangles": n_full, "create": windows(create, a.window), "render": windows(lambda: render(full), a.window)}
        render(full)
        covered_full = int((out_i >= 0).sum().item())
        row["covered"] = covered_full
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        kw = dict(mask=mask, row_pitch=w, image_stride=h * w, max_ratio=RATIO, workspace=ws_a)
        for tau in TAUS:
            adaptive = lambda: H.mesh_adaptive(1, h, w, depth, tri, count, max_error=tau, error=err, **kw)
            emit_only = lambda: H.mesh_adaptive(1, h, w, depth, tri, count, max_error=tau, error=err, error_ready=True, **kw)
            adaptive()
            n = int(count.item())
            mesh = tri[0, :n].clone()
            row = {"map": [h, w], "max_error": tau, "triangles": n, "of_full": round(n / max(n_full, 1), 5)}
            if (h, w) == SHAPES[0] and tau == TAUS[0] and os.path.exists(os.path.join(ROOT, "tests", "_adaptive_ref.py")):
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import _adaptive_ref as A
                want = A.adaptive_triangles(depth_np, mask=mask_np, max_ratio=RATIO, max_error=tau)
                row["equals_restatement"] = bool(np.array_equal(mesh.cpu().numpy(), want))
            row["adaptive"] = windows(adaptive, a.window)
            row["emit_only"] = windows(emit_only, a.window)
            row["render"] = windows(lambda: render(mesh), a.window)
            render(mesh)
            row["covered"] = int((out_i >= 0).sum().item())
            row["render_over_full"] = round(row["render"]["us"] / json.loads(lines[-1 - TAUS.index(tau)])["render"]["us"], 3)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        del tri, err, ws_a, ws_r, points, x, y, wv, full
    for item in a.bench:
        label, path = item.split("=", 1)
        last = [ln for ln in open(path).read().splitlines() if ln.startswith("{")][-1]
        lines.append(json.dumps({"bench": label, "result": json.loads(last)}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
