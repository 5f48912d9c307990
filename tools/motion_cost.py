#!/usr/bin/env python3
"""What moving spheres cost on the benchmark frame.

  frame     BASELINE config 2 -- bench.py's frame: scenes/example_scene.yaml with the 69,451-triangle stand-in,
            1024 x 768 x 50 spp, one GPU -- on ONE handle without a motion (the trace kernel's plain build), with an all-zero
            motion (the general build, the draw, the travels in LDS and the word per path, nothing moves) and with its two small
            spheres moving (the tile pass's wider margins on top), in alternating rounds of timed render_device steps in one
            process (the host builder's tree adopted first, as bench.py does). Every step renders a camera the handle has not
            seen (the position moves by one unit in the last place a step, as in bench.py), so the tile pass is inside the time.
            ms per step of every round, the medians, their ratios to the first row, the build each row ran and the
            background-only tiles of the tile pass.
Nothing here is a threshold: the output is the record (profiles/motion_config2.txt).

    python tools/motion_cost.py [--steps 20] [--warmup 3] [--rounds 3] [--travel 0.5] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--spp", type=int, default=50)
    ap.add_argument("--travel", type=float, default=0.5, help="how far the small spheres move, in scene units")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    w, h = args.width, args.height
    work = Path(tempfile.mkdtemp(prefix="rbrt_motion_cost_"))
    obj = standin.ensure_obj(work / "bunny.obj", standin.BUNNY_TRIANGLES)
    text = (ROOT / "scenes" / "example_scene.yaml").read_text().replace("obj_filepath: bunny.obj", f"obj_filepath: {obj}")
    (work / "scene.yaml").write_text(text)
    devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(1)
    os.dup2(devnull, 1)  # (the host prints the reference's loading lines)
    try:
        host = abi.HostScene(work / "scene.yaml", h, w)
    finally:
        os.dup2(saved, 1)
        os.close(devnull)
    n_sph = host.struct.n_spheres
    radii = [host.struct.spheres[i].radius for i in range(n_sph)]
    small = [i for i in range(n_sph) if radii[i] <= 1.5]  # the two spheres of radius 1.5; the ground and the mirror stay
    moving = np.zeros((n_sph, 3), np.float32)
    for k, i in enumerate(small):
        moving[i] = (args.travel, 0.0, 0.0) if k % 2 == 0 else (0.0, 0.0, args.travel)  # one across the view, one towards the camera
    motions = {"no motion": None, "zero motion": np.zeros((n_sph, 3), np.float32), "moving": moving}
    hd = rbrt_amd.HipScene(host)
    hd.refine_wait(300.0)
    lds = hd.info()["lds_bytes_per_wave"]
    opts = abi.default_opts(spp=args.spp, seed=1)
    image = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    cam = type(host.camera).from_buffer_copy(host.camera)

    def step():  # a camera the handle has not seen: the tile pass runs
        cam.position[0] = float(np.nextafter(np.float32(cam.position[0]), np.float32(np.inf)))
        hd.render_device(cam, opts, image.data_ptr(), None, stream)

    ms = {k: [] for k in motions}
    build, sky = {}, {}
    for _ in range(args.rounds):
        for k, tv in motions.items():
            hd.set_motion(tv)
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
            hd.check()
            build[k] = hd.last_trace_build()
            sky[k] = int(np.count_nonzero(hd.primary_cull(host.camera) >> 31))
            assert hd.info()["lds_bytes_per_wave"] == lds
    hd.close()
    samples = w * h * args.spp
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [f"moving spheres on config 2: {w} x {h} x {args.spp} spp, {standin.BUNNY_TRIANGLES}-triangle stand-in, spheres {small} of {n_sph} move "
             f"{args.travel} units, one handle, {args.rounds} alternating rounds of {args.steps} steps in one process, a new camera every step"]
    for k in motions:
        lines.append(f"{k:12s} {med[k]:8.4f} ms per step  ({', '.join(f'{x:.4f}' for x in ms[k])})   {samples / (med[k] * 1e-3) / 1e6:8.1f} Mray-samples/s   "
                     f"{build[k]:7s} build   background-only tiles {sky[k]} of {tiles}   over no motion {med[k] / med['no motion']:.4f}")
    lines.append(f"(LDS of a launch without a motion {lds} bytes per wave; a motion launch stages {12 * n_sph} more and keeps 4 bytes per pool slot in global memory)")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(out)


if __name__ == "__main__":
    main()
