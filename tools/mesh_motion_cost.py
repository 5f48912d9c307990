#!/usr/bin/env python3
"""What moving meshes cost on BASELINE config 2: scenes/example_scene.yaml with the 69,451-triangle stand-in, 1024 x 768, one
GPU, one handle (the host builder's tree adopted first, as bench.py does). Modelled on tools/animation_cost.py.

  frame     bench.py's frame, 50 spp, in alternating rounds of timed render_device steps in one process, every step a camera the
            handle has not seen (the tile pass is inside the time):
              plain              no motion: the trace kernel's plain build
              spheres moving     its two small spheres moving --travel units an exposure (the general build)
              mesh, zero travel  an all-zero mesh motion (the mesh-motion builds of the trace kernel, the tile pass and the stage)
              mesh moving        the stand-in moving --mesh-travel units across the view
              mesh moving, out   the same at a phase that has carried the mesh out of the view
  bench     bench.py --gpus 1 --steps K --warmup W, --bench-runs times in child processes: its ms_per_step
  stages    the features at --feature-samples, with and without d_motion, between two events, per call
The tool runs on any build of the library: rows whose entry point a build lacks are left out, so the same file measures the
parent commit (--record FILE writes every row's runs as JSON). With --parent FILE (the parent's record, made in the same
session on the same machine) the table ends with the verdicts: a row's median here must not exceed the parent's slowest run of
that row, for the plain frame, the frame with the spheres moving, bench.py and the features with and without d_motion. The
mesh rows have nothing to be compared with and carry no verdict.

    python tools/mesh_motion_cost.py [--rounds 5] [--steps 20] [--bench-runs 3] [--record FILE] [--parent FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--spp", type=int, default=50)
    ap.add_argument("--travel", type=float, default=0.5, help="how far the small spheres move an exposure, in scene units")
    ap.add_argument("--mesh-travel", type=float, default=0.05, help="how far the stand-in moves an exposure, in scene units")
    ap.add_argument("--out-phase", type=float, default=2000.0, help="the phase of the row whose mesh has left the view")
    ap.add_argument("--feature-samples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--record", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    lib = abi.load_hip()
    has_mesh = hasattr(lib, "rbrt_hip_scene_set_mesh_motion")
    w, h = args.width, args.height
    work = Path(tempfile.mkdtemp(prefix="rbrt_mesh_motion_cost_"))
    obj = standin.ensure_obj(work / "bunny.obj", standin.BUNNY_TRIANGLES)
    (work / "scene.yaml").write_text((ROOT / "scenes" / "example_scene.yaml").read_text().replace("obj_filepath: bunny.obj", f"obj_filepath: {obj}"))
    devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(1)
    os.dup2(devnull, 1)  # (the host prints the reference's loading lines)
    try:
        host = abi.HostScene(work / "scene.yaml", h, w)
    finally:
        os.dup2(saved, 1)
        os.close(devnull)
    n_sph = host.struct.n_spheres
    small = [i for i in range(n_sph) if host.struct.spheres[i].radius <= 1.5]
    moving = np.zeros((n_sph, 3), np.float32)
    for k, i in enumerate(small):
        moving[i] = (args.travel, 0.0, 0.0) if k % 2 == 0 else (0.0, 0.0, args.travel)
    across = np.array([(args.mesh_travel, 0.0, 0.0)], np.float32)
    # (spheres' travels, meshes' travels, phase)
    cases = {"plain": (None, None, 0.0), "spheres moving": (moving, None, 0.0)}
    if has_mesh:
        cases["mesh, zero travel"] = (None, np.zeros((1, 3), np.float32), 0.0)
        cases["mesh moving"] = (None, across, 0.0)
        cases["mesh moving, out"] = (None, across, args.out_phase)
    hd = rbrt_amd.HipScene(host)
    hd.refine_wait(300.0)
    opts = abi.default_opts(spp=args.spp, seed=1)
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    image = new(h, w, 3)
    stream = torch.cuda.current_stream().cuda_stream
    cam = type(host.camera).from_buffer_copy(host.camera)

    def step():  # a camera the handle has not seen: the tile pass runs
        cam.position[0] = float(np.nextafter(np.float32(cam.position[0]), np.float32(np.inf)))
        hd.render_device(cam, opts, image.data_ptr(), None, stream)

    def set_case(tv, mw, phase):
        hd.set_motion(tv)
        if has_mesh:
            hd.set_mesh_motion(mw)
        if hasattr(lib, "rbrt_hip_scene_set_motion_phase"):
            hd.set_motion_phase(phase)

    runs = {k: [] for k in cases}
    build, sky, meshless = {}, {}, {}
    for _ in range(args.rounds):
        for k, case in cases.items():
            set_case(*case)
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            runs[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
            hd.check()
            build[k] = hd.last_trace_build()
            table = hd.primary_cull(host.camera)
            sky[k], meshless[k] = int(np.count_nonzero(table >> 31)), int(np.count_nonzero((table >> 24) & 1))
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    lines = [f"moving meshes on config 2: {w} x {h}, {standin.BUNNY_TRIANGLES}-triangle stand-in, one handle; spheres {small} of {n_sph} move {args.travel} units an "
             f"exposure, the mesh {args.mesh_travel}; the out-of-view phase is {args.out_phase}",
             f"frame rows: {args.spp} spp, {args.rounds} alternating rounds of {args.steps} steps in one process, a new camera every step; ms per step, median (every run)"]
    for k in cases:
        lines.append(f"{k:28s} {statistics.median(runs[k]):8.4f} ms  ({', '.join(f'{x:.4f}' for x in runs[k])})   {build[k]:7s} build   "
                     f"background-only tiles {sky[k]}, mesh-free tiles {meshless[k]} of {tiles}   over plain {statistics.median(runs[k]) / statistics.median(runs['plain']):.4f}")

    # ---- the features ----
    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.repeats + 1):
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms[1:]

    albedo, normal, motion = (new(h, w, 3) for _ in range(3))
    depth, coverage = (new(h, w) for _ in range(2))
    fopts = abi.default_opts(spp=args.spp, seed=1)

    def features(with_motion):
        kw = dict(d_motion=motion.data_ptr()) if with_motion else {}
        hd.render_features(host.camera, fopts, args.feature_samples, albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(), coverage.data_ptr(), stream=stream, **kw)

    stage = {}
    set_case(moving, None, 0.0)  # (the handle the parent can have too: the spheres' motion only)
    stage["features"] = events(lambda: features(False))
    if hasattr(lib, "rbrt_hip_render_features_motion"):
        stage["features motion"] = events(lambda: features(True))
    if has_mesh:
        set_case(None, across, 0.0)
        stage["features, mesh moving"] = events(lambda: features(False))
        stage["features motion, mesh moving"] = events(lambda: features(True))
    hd.check()
    hd.close()
    lines.append(f"stage rows: the features at {args.feature_samples} samples on the handle with the spheres moving (and with the mesh moving), one call between two "
                 f"events, median (least - most) of {args.repeats} warm measurements")
    for k, ms in stage.items():
        lines.append(f"{k:28s} {statistics.median(ms):8.4f} ms  ({min(ms):.4f} - {max(ms):.4f})")

    # ---- bench.py, in child processes ----
    bench = []
    for _ in range(args.bench_runs):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)],
                           capture_output=True, text=True, timeout=900)
        rows = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not rows:
            lines.append(f"bench.py failed (exit {r.returncode}): {r.stderr[-300:]}")
            break
        bench.append(float(json.loads(rows[-1])["ms_per_step"]))
    if bench:
        lines.append(f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}, {len(bench)} runs in child processes: ms_per_step "
                     f"{', '.join(f'{x:.4f}' for x in bench)}   median {statistics.median(bench):.4f}")
    record = {"frame": runs, "stage": stage, "bench": {"bench.py": bench} if bench else {}}
    if args.record:
        Path(args.record).parent.mkdir(parents=True, exist_ok=True)
        Path(args.record).write_text(json.dumps(record))
    if args.parent:
        par = json.loads(Path(args.parent).read_text())
        lines.append("against the parent commit, built and run in the same session on the same machine: this median <= the parent's slowest run?")
        pairs = [("frame", "plain"), ("frame", "spheres moving"), ("bench", "bench.py"), ("stage", "features"), ("stage", "features motion")]
        for kind, row in pairs:
            if row not in record.get(kind, {}) or row not in par.get(kind, {}):
                lines.append(f"{row:28s} not measured on both builds")
                continue
            mine, theirs = record[kind][row], par[kind][row]
            med, worst = statistics.median(mine), max(theirs)
            lines.append(f"{row:28s} {med:8.4f} ms here; the parent: median {statistics.median(theirs):.4f}, runs {min(theirs):.4f} - {worst:.4f}   "
                         f"{'yes' if med <= worst else 'NO'}")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(out)


if __name__ == "__main__":
    main()
