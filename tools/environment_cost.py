#!/usr/bin/env python3
"""What environment lighting costs on BASELINE config 2: scenes/example_scene.yaml with the 69,451-triangle stand-in at
1024 x 768 x 50 spp, one GPU, one handle (the host builder's tree adopted first, as bench.py does), the tile pass on.

  gradient          the frame as it is without a map: rays that hit nothing see the sky gradient
  environment N     the same frame with the stand-in sky (rbrt_amd.standin.make_sky) converted to an N-node map on the
                    handle: every path that escapes reads four 16-byte nodes once ((N + 1)^2 * 16 bytes in all: 16.8 MB
                    at N = 1024, more than one XCD's 4 MiB L2)
  noise N           the same with white noise in the nodes: the image changes, the addresses do not (a check that the cost
                    is the map's size, not its content)

Each row is a STREAM of --frames rbrt_hip_render_device calls issued back to back and synchronised once (the frame
pipeline overlaps them), per-frame time = wall clock / frames; --repeats streams per row, alternating between the rows so
that drift hits all of them alike; one untimed stream per row first. Prints the median, the least and the most.

    python tools/environment_cost.py [--resolutions 1024] [--frames 20] [--repeats 5] [--out FILE]   (--out appends)
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
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--resolutions", default="1024", help="N of every environment row, comma separated")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    work = Path(tempfile.mkdtemp(prefix="rbrt_environment_cost_"))
    obj = standin.ensure_obj(work / "bunny.obj", standin.BUNNY_TRIANGLES)
    (work / "scene.yaml").write_text((ROOT / "scenes" / "example_scene.yaml").read_text().replace("obj_filepath: bunny.obj", f"obj_filepath: {obj}"))
    devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(1)
    os.dup2(devnull, 1)  # (the host prints the reference's loading lines)
    try:
        host = abi.HostScene(work / "scene.yaml", args.height, args.width)
    finally:
        os.dup2(saved, 1)
        os.close(devnull)
    w, h = args.width, args.height
    opts = abi.default_opts(spp=args.samples, seed=1)
    rad = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    sky = standin.make_sky(1024)
    rows = [("gradient", None)]
    for n in (int(v) for v in args.resolutions.split(",")):
        rows.append((f"environment N = {n}", abi.environment_nodes(sky, n)))
        rows.append((f"noise N = {n}", np.random.default_rng(n).uniform(0.0, 2.0, (n + 1, n + 1, 3)).astype(np.float32)))
    times = {name: [] for name, _ in rows}
    with rbrt_amd.HipScene(host) as hs:
        hs.refine_wait(300.0)
        for rep in range(args.repeats + 1):  # (the first round warms every row: buffers, tile tables, the map's first touch)
            for name, nodes in rows:
                hs.set_environment(nodes)  # (blocking: the upload is not in the timed part)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.frames):
                    hs.render_device(host.camera, opts, rad.data_ptr(), lens=host.lens)
                torch.cuda.synchronize()
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3 / args.frames)
        hs.check()
    base = statistics.median(times["gradient"])
    lines = [f"environment lighting on config 2: {w} x {h} x {args.samples} spp, {standin.BUNNY_TRIANGLES}-triangle stand-in, tile pass on, "
             f"ms per frame in a stream of {args.frames} frames, median (least - most) of {args.repeats} streams"]
    for name, nodes in rows:
        t = times[name]
        mb = 0.0 if nodes is None else nodes.shape[0] * nodes.shape[1] * 16 / 1e6
        lines.append(f"{name:24s} {statistics.median(t):8.3f} ms  ({min(t):.3f} - {max(t):.3f})   {statistics.median(t) / base * 100 - 100:+6.2f} %   map {mb:6.1f} MB")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
