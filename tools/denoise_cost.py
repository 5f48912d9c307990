#!/usr/bin/env python3
"""What the denoiser costs on BASELINE config 2: scenes/example_scene.yaml with the 69,451-triangle stand-in at 1024 x 768,
one GPU, one handle (the host builder's tree adopted first, as bench.py does).

  adaptive render   rbrt_hip_render_adaptive at --samples with threshold 0 in one round (what --denoise without --adaptive
                    runs): a blocking call, timed from the call to the synchronisation behind it
  denoise           rbrt_hip_scene_denoise on that render (both kernels: the half images, then the filter), for every (R, P)
                    of --params, between two events on the stream; each row warm (one untimed call first), the median, the
                    least and the most of --repeats
  arithmetic        per row the filter's divisions as the rule counts them -- 6 per delta (three channels, two guides), one
                    delta per pixel of every 16 x 16 tile plus its halo of P, per offset of the window -- and their rate

Prints a table; --out FILE also writes it there (profiles/denoise_config2.txt).

    python tools/denoise_cost.py [--samples 50] [--params 5,3:3,2:10,4] [--repeats 9] [--out FILE]
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
TILE = 16  # RBRT_DENOISE_TILE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--params", default="5,3:3,2:10,4", help="window radius, patch radius of every row")
    ap.add_argument("--strength", type=float, default=0.7)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    params = [tuple(int(v) for v in row.split(",")) for row in args.params.split(":")]

    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    work = Path(tempfile.mkdtemp(prefix="rbrt_denoise_cost_"))
    obj = standin.ensure_obj(work / "bunny.obj", standin.BUNNY_TRIANGLES)
    (work / "scene.yaml").write_text((ROOT / "scenes" / "example_scene.yaml").read_text().replace("obj_filepath: bunny.obj", f"obj_filepath: {obj}"))
    devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(1)
    os.dup2(devnull, 1)  # (the host prints the reference's loading lines)
    try:
        host = abi.HostScene(work / "scene.yaml", args.height, args.width)
    finally:
        os.dup2(saved, 1)
        os.close(devnull)
    w, h, n = args.width, args.height, args.samples
    opts = abi.default_opts(spp=n, seed=1)
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    rad = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    lines = [f"the denoiser on config 2: {w} x {h}, {n} spp in one round (threshold 0), {standin.BUNNY_TRIANGLES}-triangle stand-in, strength {args.strength:g}, "
             f"median (least - most) of {args.repeats} warm calls"]

    with rbrt_amd.HipScene(host) as hs:
        hs.refine_wait(300.0)
        ms = []
        for _ in range(args.repeats + 1):  # (the first one warms the handle: buffers, tile tables)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hs.render_adaptive(host.camera, opts, 0.0, n, n, rad.data_ptr(), rgb.data_ptr(), lens=host.lens)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"{'adaptive render (host clock)':34s} {statistics.median(ms[1:]):8.3f} ms  ({min(ms[1:]):.3f} - {max(ms[1:]):.3f})")
        tiles = ((w + TILE - 1) // TILE) * ((h + TILE - 1) // TILE)
        for R, P in params:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream = torch.cuda.current_stream().cuda_stream
            ms = []
            for _ in range(args.repeats + 1):
                e0.record()
                hs.denoise(rad.data_ptr(), rgb.data_ptr(), window_radius=R, patch_radius=P, strength=args.strength, stream=stream)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms[1:])
            divisions = 6.0 * tiles * (TILE + 2 * P) ** 2 * (2 * R + 1) ** 2  # (an upper bound: offsets and deltas outside the image do none)
            lines.append(f"{f'denoise R = {R}, P = {P} (events)':34s} {med:8.3f} ms  ({min(ms[1:]):.3f} - {max(ms[1:]):.3f})   "
                         f"{divisions / 1e9:6.2f} G divisions, {divisions / med / 1e9:6.2f} T divisions/s")
        hs.check()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
