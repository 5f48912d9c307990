#!/usr/bin/env python3
"""What a camera shutter costs on the benchmark frame.

  frame     BASELINE config 2 -- bench.py's frame: scenes/example_scene.yaml with the 69,451-triangle stand-in,
            1024 x 768 x 50 spp, one GPU -- on ONE handle without a shutter and with rbrt_hip_scene_set_shutter(travel), in
            alternating rounds of timed render_device steps in one process (the host builder's tree adopted first, as bench.py
            does). Every step renders a camera the handle has not seen (the position moves by one unit in the last place a
            step, as in bench.py), so the tile pass with its wider margins is inside the time. ms per step of every round, the
            medians, their ratio, and the background-only tiles of the tile pass for either.
Nothing here is a threshold: the output is the record (profiles/shutter_config2.txt).

    python tools/shutter_cost.py [--steps 20] [--warmup 3] [--rounds 3] [--travel 0.002,0,0] [--out FILE]
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
    ap.add_argument("--travel", default="0.002,0,0")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    w, h = args.width, args.height
    travel = tuple(float(v) for v in args.travel.split(","))
    work = Path(tempfile.mkdtemp(prefix="rbrt_shutter_cost_"))
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
    hd = rbrt_amd.HipScene(host)
    hd.refine_wait(300.0)
    lds = hd.info()["lds_bytes_per_wave"]
    sky = {"plain": int(np.count_nonzero(hd.primary_cull(host.camera) >> 31)),
           "shutter": int(np.count_nonzero(hd.primary_cull_shutter(host.camera, None, travel) >> 31))}
    opts = abi.default_opts(spp=args.spp, seed=1)
    image = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    cam = type(host.camera).from_buffer_copy(host.camera)

    def step():  # a camera the handle has not seen: the tile pass runs
        cam.position[0] = float(np.nextafter(np.float32(cam.position[0]), np.float32(np.inf)))
        hd.render_device(cam, opts, image.data_ptr(), None, stream)

    ms = {"plain": [], "shutter": []}
    for _ in range(args.rounds):
        for k in ms:
            hd.set_shutter(travel if k == "shutter" else None)
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
            hd.check()
            assert hd.info()["lds_bytes_per_wave"] == lds
    hd.close()
    samples = w * h * args.spp
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [f"a camera shutter on config 2: {w} x {h} x {args.spp} spp, {standin.BUNNY_TRIANGLES}-triangle stand-in, travel {travel}, one handle, "
             f"{args.rounds} alternating rounds of {args.steps} steps in one process, a new camera every step"]
    for k in ("plain", "shutter"):
        lines.append(f"{k:8s} {med[k]:8.4f} ms per step  ({', '.join(f'{x:.4f}' for x in ms[k])})   "
                     f"{samples / (med[k] * 1e-3) / 1e6:8.1f} Mray-samples/s   background-only tiles {sky[k]} of {tiles}")
    lines.append(f"shutter over plain {med['shutter'] / med['plain']:.4f}   (LDS of a shutterless launch {lds} bytes per wave; a shutter launch stages 16 more)")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(out)


if __name__ == "__main__":
    main()
