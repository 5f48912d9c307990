#!/usr/bin/env python3
"""What smooth shading costs on BASELINE config 2: bench.py's frame (scenes/example_scene.yaml with the 69,451-triangle
stand-in, 1024 x 768 x 50 spp, one GPU) with the mesh flat and with `shading: smooth`, in alternating rounds of timed
render_device steps on one handle each (the host builder's tree adopted first, as bench.py does). Prints one JSON line:
median ms per step and Mray-samples/s of both, and the smooth frame's cost relative to the flat one.

    python tools/smooth_cost.py [--steps 20] [--warmup 3] [--rounds 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--spp", type=int, default=50)
    args = ap.parse_args()

    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    work = Path(tempfile.mkdtemp(prefix="rbrt_smooth_cost_"))
    obj = standin.ensure_obj(work / "bunny.obj", standin.BUNNY_TRIANGLES)
    text = (ROOT / "scenes" / "example_scene.yaml").read_text().replace("obj_filepath: bunny.obj", f"obj_filepath: {obj}")
    smooth_text = text.replace('    material_type: "dielectric"\n', '    material_type: "dielectric"\n    shading: smooth\n', 1)
    assert smooth_text != text
    (work / "flat.yaml").write_text(text)
    (work / "smooth.yaml").write_text(smooth_text)
    devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(1)
    os.dup2(devnull, 1)  # (the host prints the reference's loading lines)
    try:
        hosts = {k: abi.HostScene(work / f"{k}.yaml", args.height, args.width) for k in ("flat", "smooth")}
    finally:
        os.dup2(saved, 1)
        os.close(devnull)
    assert hosts["flat"].shading is None and hosts["smooth"].shading is not None
    handles = {k: rbrt_amd.HipScene(h) for k, h in hosts.items()}
    for h in handles.values():
        h.refine_wait(300.0)
    opts = abi.default_opts(spp=args.spp, seed=1)
    image = torch.empty((args.height, args.width, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ms = {k: [] for k in handles}
    for _ in range(args.rounds):
        for k, h in handles.items():
            cam = hosts[k].camera
            for _ in range(args.warmup):
                h.render_device(cam, opts, image.data_ptr(), None, stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                h.render_device(cam, opts, image.data_ptr(), None, stream)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
            h.check()
    for h in handles.values():
        h.close()
    samples = args.width * args.height * args.spp
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                      "mray_samples_per_s": {k: round(samples / (m * 1e-3) / 1e6, 1) for k, m in med.items()},
                      "smooth_over_flat": round(med["smooth"] / med["flat"], 4),
                      "config": f"{args.width}x{args.height}x{args.spp} spp, {standin.BUNNY_TRIANGLES}-triangle stand-in, "
                                f"{args.rounds} rounds of {args.steps} steps"}))


if __name__ == "__main__":
    main()
