"""Time of the rasteriser (csrc/ada_raster.hip) behind hip_ext.geometry.render_mesh, on the device this runs on.

    python tools/profile_raster.py [--out profiles/raster.txt] [--window 0.3] [--shapes N] [--bench LABEL=FILE ...]

Targets of 518 x 518, 1080 x 1920 and 2160 x 3840.  Scenes, each rendered at the size of its depth map:
  identity        the full grid mesh of a depth map (all-ones mask, 2 (h - 1)(w - 1) triangles about one pixel wide), no pose
  yaw12           a depth map with eight vertical depth steps (z = 2 | 4, plus a smooth wave of 0.05) under look_at_pose(yaw_deg=12, pivot at z = 3): the triangles across a step stretch
  yaw12_ratio     the same map meshed with max_ratio=1.5 (the stretched triangles are gone, holes open)
  two_large       two triangles that together fill the screen
  stack64         64 screen-filling triangles at distinct depths, the nearest last in the list
Every figure is the median of three windows of HIP events around back-to-back calls on resident buffers with the workspace allocated once, in
microseconds per call, with the windows' min-max.  ``project`` is ada_mesh_project_fwd, ``raster`` ada_mesh_raster_fwd (clear, bin, walk, resolve) with
and without vertex colours, ``render_mesh`` the public call (its allocations and the owner map included).  Beside ``raster``: the bytes the call has to
move at least and the TB/s that implies -- per vertex 16 B of records gathered at least once, per triangle 12 B of indices, per pixel 8 B of key
cleared, 8 B read by the resolve, 8 B of depth and index written, one 8-B key atomic per covered sample at least (the count actually issued is not
measured here: it needs a counter pass), with colours 3 B per vertex and per pixel more.

Cache state: the calls of a window re-read the same vertex records and triangle list (up to 133 MB and 199 MB at 4K: the list alone nearly fills the
256 MB Infinity Cache, so it streams), the key buffer (66 MB at 4K) is cleared, hit by the atomics and read back within one call.

The one condition fixed beforehand: at 4K, two_large takes no longer than identity.  ``--bench``: JSON result lines of bench.py copied into the file.
There is no CPU path."""
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

SHAPES = ((518, 518), (1080, 1920), (2160, 3840))


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


def scenes(G, h, w):
    """name -> (points fp32 [V, 3], triangles int32 [T, 3], colors uint8 [V, 3], R, t), all on the device."""
    rng = np.random.default_rng(h)
    smooth = rng.uniform(1.0, 1.5, size=(h, w)).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w] / float(w)      # relief that does not depend on the resolution: eight depth steps and a smooth wave
    steps = (2.0 + 2.0 * ((np.arange(w) * 8 // w) % 2)[None, :] + 0.05 * np.sin(40.0 * xx) * np.cos(31.0 * yy)).astype(np.float32)
    photo = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
    pose = G.look_at_pose(yaw_deg=12.0, pivot_z=3.0)
    m = G.depth_to_mesh(smooth, colors=photo, compact=False)
    yield "identity", (m.points, m.triangles, m.colors, None, None)
    m = G.depth_to_mesh(steps, colors=photo, compact=False)
    yield "yaw12", (m.points, m.triangles, m.colors) + pose
    m = G.depth_to_mesh(steps, colors=photo, compact=False, max_ratio=1.5)
    yield "yaw12_ratio", (m.points, m.triangles, m.colors) + pose
    K = G.get_intrinsics(h, w)

    def at(u, v, z):      # the point the camera sees at pixel (u, v), depth z
        return [-(u - K[0, 2]) / K[0, 0] * z, -(v - K[1, 2]) / K[1, 1] * z, z]
    quad = lambda z: [at(-0.5, -0.5, z), at(w - 0.5, -0.5, z), at(-0.5, h - 0.5, z), at(w - 0.5, h - 0.5, z)]
    pts = torch.tensor(quad(2.0), dtype=torch.float32, device="cuda")
    tri = torch.tensor([[0, 2, 1], [3, 1, 2]], dtype=torch.int32, device="cuda")
    yield "two_large", (pts, tri, photo.reshape(-1, 3)[:4].contiguous(), None, None)
    cover = lambda z: [at(-1.0, -1.0, z), at(2.0 * w + 1, -1.0, z), at(-1.0, 2.0 * h + 1, z)]
    pts = torch.tensor(sum((cover(70.0 - k) for k in range(64)), []), dtype=torch.float32, device="cuda")
    tri = torch.arange(192, dtype=torch.int32, device="cuda").reshape(64, 3)
    yield "stack64", (pts, tri, photo.reshape(-1, 3)[:192].contiguous(), None, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster.txt"))
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="how many of the shapes to run, in the order above")
    ap.add_argument("--bench", nargs="*", default=[], help="label=file pairs: the last JSON line of each file (a bench.py run) is recorded")
    a = ap.parse_args()
    import hip_ext as H
    from hip_ext import geometry as G
    H.load()
    assert torch.cuda.is_available(), "profile_raster needs a HIP device"
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# mesh rasteriser on {prop.name}: arch {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB "
             "(csrc/ada_raster.hip, hip_ext/geometry.py)",
             "# python tools/profile_raster.py",
             f"# us per call: median of three windows of about {a.window} s (and their min-max) of HIP events around back-to-back calls, resident buffers, workspace allocated once.",
             "# project = ada_mesh_project_fwd; raster = ada_mesh_raster_fwd (clear, bin, walk, resolve), raster_color the same with vertex colours; render_mesh(_color) = the public call, allocations and owner map included.",
             "# bytes: what raster has to move at least: 16 B per vertex record, 12 B per triangle, per pixel 8 B key cleared + 8 B key read + 8 B depth and index written + one 8-B atomic per covered sample.",
             "# The key atomics actually issued per covered sample are not measured here (no counter pass); covered = samples with a triangle, middle / large = entries of the two device lists.",
             "# Cache state: vertex records and triangle list re-read every call (at 4K identity 133 MB + 199 MB: streamed, above the 256 MB Infinity Cache); keys (66 MB at 4K) cleared, hit and read back within a call.",
             f"# Classes: box <= {H.RASTER_SMALL_MAX} samples by the triangle's thread, <= {H.RASTER_WAVE_MAX} by one wave, larger by a team of >= {H.RASTER_WALK_SHARE} of the walk's {H.RASTER_WALK_BLOCKS} workgroups.",
             "# No bar was fixed in advance but one: at 4K, two_large takes no longer than identity."]
    for h, w in SHAPES[:a.shapes]:
        us = {}
        K = G.get_intrinsics(h, w)
        for name, (pts, tri, col, Rm, t) in scenes(G, h, w):
            V, T = pts.shape[0], tri.shape[0]
            cam = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]] + list((np.eye(3) if Rm is None else Rm).reshape(-1)) + list(np.zeros(3) if t is None else t)
            x = torch.empty(V, dtype=torch.int32, device="cuda")
            y = torch.empty(V, dtype=torch.int32, device="cuda")
            wv = torch.empty(V, dtype=torch.float64, device="cuda")
            depth = torch.empty(h, w, dtype=torch.float32, device="cuda")
            index = torch.empty(h, w, dtype=torch.int32, device="cuda")
            color = torch.empty(h, w, 3, dtype=torch.uint8, device="cuda")
            ws = torch.empty((H.mesh_raster_workspace_bytes(h, w, T) + 15) // 16 * 2, dtype=torch.int64, device="cuda")
            project = lambda: H.mesh_project(pts, cam, x, y, wv, pose=Rm is not None)
            raster = lambda c=None, o=None: H.mesh_raster(x, y, wv, tri, h, w, depth, index, colors=c, color=o, workspace=ws)
            row = {"target": [h, w], "scene": name, "vertices": V, "triangles": T}
            row["project"] = windows(project, a.window)
            raster()
            torch.cuda.synchronize()
            hw2 = h * w + (h * w) % 2
            counters = ws.view(torch.int32)[2 * hw2: 2 * hw2 + 2].tolist()
            covered = int((index >= 0).sum().item())
            row.update({"covered": covered, "middle": counters[0], "large": counters[1]})
            row["raster"] = windows(raster, a.window)
            nbytes = 16 * V + 12 * T + 24 * h * w + 8 * covered
            row["raster"].update({"bytes": int(nbytes), "TB_per_s": round(nbytes / (row["raster"]["us"] * 1e-6) / 1e12, 3)})
            row["raster_color"] = windows(lambda: raster(col, color), a.window)
            row["render_mesh"] = windows(lambda: G.render_mesh(pts, h, w, triangles=tri, R=Rm, t=t), a.window)
            row["render_mesh_color"] = windows(lambda: G.render_mesh(pts, h, w, triangles=tri, colors=col, R=Rm, t=t), a.window)
            us[name] = row["raster"]["us"]
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
            del x, y, wv, depth, index, color, ws, pts, tri, col
        lines.append(json.dumps({"target": [h, w], "two_large_over_identity": round(us["two_large"] / us["identity"], 3),
                                 "two_large_no_longer_than_identity": bool(us["two_large"] <= us["identity"])}))
        print(lines[-1], flush=True)
    for item in a.bench:
        label, path = item.split("=", 1)
        last = [ln for ln in open(path).read().splitlines() if ln.startswith("{")][-1]
        lines.append(json.dumps({"bench": label, "result": json.loads(last)}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
