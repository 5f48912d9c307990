#!/usr/bin/env python3
"""What the animation costs on BASELINE config 2: scenes/example_scene.yaml with the 69,451-triangle stand-in, 1024 x 768, one
GPU, one handle (the host builder's tree adopted first, as bench.py does).

  frame     bench.py's frame, 50 spp, in alternating rounds of timed render_device steps in one process, every step a camera the
            handle has not seen (the tile pass is inside the time), as tools/motion_cost.py measures it:
              plain            no motion: the trace kernel's plain build
              moving           its two small spheres moving --travel units an exposure (the general build), no phase call
              moving, phase 7  the same seven exposures later (the tile pass bounds around the advanced centres)
  stages    at the same size, between two events around --inner calls in a row, per call:
              accumulate       rbrt_hip_temporal_accumulate with every output under a drifting camera
              accumulate moving  rbrt_hip_temporal_accumulate_moving on the same inputs with a motion buffer and a step of 1
              copy             a device copy that moves the plain call's 170 bytes a pixel
              features         rbrt_hip_render_features at --feature-samples on the moving handle
              features motion  rbrt_hip_render_features_motion on the same handle, d_motion written too
The tool runs on any build of the library: rows whose entry point a build lacks are left out, so the same file measures the
parent commit (--record FILE writes every row's runs as JSON). With --parent FILE (the parent's record, made in the same
session on the same machine) the table ends with the verdicts: a row's median here must not exceed the parent's slowest run of
that row, for the plain frame, the moving frame at phase 0 and 7 against the parent's moving frame, and the plain stage calls.

    python tools/animation_cost.py [--rounds 5] [--steps 20] [--record FILE] [--parent FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BYTES_PER_PIXEL = 170  # (tools/temporal_cost.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--spp", type=int, default=50)
    ap.add_argument("--travel", type=float, default=0.5, help="how far the small spheres move an exposure, in scene units")
    ap.add_argument("--feature-samples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--record", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    lib = abi.load_hip()
    has = {k: hasattr(lib, k) for k in ("rbrt_hip_scene_set_motion_phase", "rbrt_hip_render_features_motion", "rbrt_hip_temporal_accumulate_moving")}
    w, h = args.width, args.height
    npix = w * h
    work = Path(tempfile.mkdtemp(prefix="rbrt_animation_cost_"))
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
    small = [i for i in range(n_sph) if host.struct.spheres[i].radius <= 1.5]  # the two spheres of radius 1.5; the ground and the mirror stay
    moving = np.zeros((n_sph, 3), np.float32)
    for k, i in enumerate(small):
        moving[i] = (args.travel, 0.0, 0.0) if k % 2 == 0 else (0.0, 0.0, args.travel)  # one across the view, one towards the camera
    cases = {"plain": (None, None), "moving": (moving, None)}
    if has["rbrt_hip_scene_set_motion_phase"]:
        cases["moving, phase 7"] = (moving, 7.0)
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

    runs = {k: [] for k in cases}
    build, sky = {}, {}
    for _ in range(args.rounds):
        for k, (tv, phase) in cases.items():
            hd.set_motion(tv)
            if has["rbrt_hip_scene_set_motion_phase"]:
                hd.set_motion_phase(phase if phase is not None else 0.0)
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
            sky[k] = int(np.count_nonzero(hd.primary_cull(host.camera) >> 31))
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    lines = [f"animation on config 2: {w} x {h}, {standin.BUNNY_TRIANGLES}-triangle stand-in, one handle; spheres {small} of {n_sph} move {args.travel} units an exposure",
             f"frame rows: {args.spp} spp, {args.rounds} alternating rounds of {args.steps} steps in one process, a new camera every step; ms per step, median (every run)"]
    for k in cases:
        lines.append(f"{k:28s} {statistics.median(runs[k]):8.4f} ms  ({', '.join(f'{x:.4f}' for x in runs[k])})   {build[k]:7s} build   "
                     f"background-only tiles {sky[k]} of {tiles}   over plain {statistics.median(runs[k]) / statistics.median(runs['plain']):.4f}")

    # ---- the image stages ----
    def events(call, inner=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.repeats + 1):
            e0.record()
            for _ in range(inner):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / inner)
        return ms[1:]

    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    rad, ha, hb, oa, ob, albedo, normal, motion = (new(h, w, 3) for _ in range(8))
    depth, coverage, length = (new(h, w) for _ in range(3))
    hist = [torch.zeros((rbrt_amd.temporal_history_bytes(w, h),), dtype=torch.uint8, device="cuda") for _ in range(2)]
    src, dst = (torch.zeros((BYTES_PER_PIXEL * npix // 2,), dtype=torch.uint8, device="cuda") for _ in range(2))  # a copy reads and writes: half each way
    hd.set_motion(moving)
    if has["rbrt_hip_scene_set_motion_phase"]:
        hd.set_motion_phase(1.0)
    fopts = abi.default_opts(spp=args.spp, seed=1)
    hd.render_adaptive(host.camera, fopts, 0.0, args.spp, args.spp, rad.data_ptr(), rgb.data_ptr())
    hd.denoise(None, None, ha.data_ptr(), hb.data_ptr())
    prev = type(host.camera).from_buffer_copy(host.camera)
    prev.position[0] -= 0.002
    prev.img_center_point[0] -= 0.002

    def features(c, with_motion):
        kw = dict(d_motion=motion.data_ptr()) if with_motion else {}
        hd.render_features(c, fopts, args.feature_samples, albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(), coverage.data_ptr(), stream=stream, **kw)

    def accumulate(c, p, hin, hout, moving_call):
        kw = dict(d_motion=motion.data_ptr(), phase_step=1.0) if moving_call else {}
        rbrt_amd.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), normal.data_ptr(), depth.data_ptr(), coverage.data_ptr(), c, p,
                                     hin.data_ptr() if hin is not None else None, hout.data_ptr(), oa.data_ptr(), ob.data_ptr(), length.data_ptr(),
                                     stream=stream, **kw)

    features(prev, False)
    accumulate(prev, None, None, hist[0], False)
    features(host.camera, has["rbrt_hip_render_features_motion"])
    torch.cuda.synchronize()
    stage = {"accumulate": events(lambda: accumulate(host.camera, prev, hist[0], hist[1], False), args.inner)}
    valid = {"accumulate": float((length > 1).float().mean().item())}
    if has["rbrt_hip_temporal_accumulate_moving"]:
        stage["accumulate moving"] = events(lambda: accumulate(host.camera, prev, hist[0], hist[1], True), args.inner)
        valid["accumulate moving"] = float((length > 1).float().mean().item())
    stage["copy"] = events(lambda: dst.copy_(src), args.inner)
    stage["features"] = events(lambda: features(host.camera, False))
    if has["rbrt_hip_render_features_motion"]:
        stage["features motion"] = events(lambda: features(host.camera, True))
    hd.check()
    hd.close()
    lines.append(f"stage rows: events around {args.inner} calls in a row (the features: one), per call, median (least - most) of {args.repeats} warm measurements; "
                 f"features at {args.feature_samples} samples; the copy moves {BYTES_PER_PIXEL} bytes a pixel")
    for k, ms in stage.items():
        note = f"   valid history {100 * valid[k]:6.2f} %" if k in valid else ""
        lines.append(f"{k:28s} {statistics.median(ms):8.4f} ms  ({min(ms):.4f} - {max(ms):.4f}){note}")
    record = {"frame": runs, "stage": stage}
    if args.record:
        Path(args.record).parent.mkdir(parents=True, exist_ok=True)
        Path(args.record).write_text(json.dumps(record))
    if args.parent:
        par = json.loads(Path(args.parent).read_text())
        lines.append("against the parent commit, built and run in the same session on the same machine: this median <= the parent's slowest run?")
        pairs = [("frame", "plain", "plain"), ("frame", "moving", "moving"), ("frame", "moving, phase 7", "moving"),
                 ("stage", "accumulate", "accumulate"), ("stage", "features", "features")]
        for kind, here, there in pairs:
            if here not in record[kind] or there not in par[kind]:
                continue
            mine, theirs = record[kind][here], par[kind][there]
            med, worst = statistics.median(mine), max(theirs)
            lines.append(f"{here:28s} {med:8.4f} ms here; the parent's {there}: median {statistics.median(theirs):.4f}, runs {min(theirs):.4f} - {worst:.4f}   "
                         f"{'yes' if med <= worst else 'NO'}")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(out)


if __name__ == "__main__":
    main()
