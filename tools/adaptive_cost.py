#!/usr/bin/env python3
"""What adaptive sampling buys and what its rounds cost on BASELINE config 2: scenes/example_scene.yaml with the
69,451-triangle stand-in at 1024 x 768, --samples 256, one GPU, one handle (the host builder's tree adopted first, as
bench.py does). Blocking calls, each timed from the call to the synchronisation behind it, the median of --repeats:

  fixed           rbrt_hip_render_device at spp = samples
  threshold 0     rbrt_hip_render_adaptive that stops nothing: the same image; the difference to `fixed` is what the rounds
                  cost (a drain and a 4-byte read-back each), reported per round, for every --step given
  thresholds      for every --step: time, samples traced / samples a fixed render traces, rounds, and the mean absolute
                  RGB8 difference to the fixed image

Prints a table; --out FILE also writes it there (profiles/adaptive_config2.txt).

    python tools/adaptive_cost.py [--samples 256] [--thresholds 0.05,0.02,0.01] [--steps 16,32,64] [--repeats 3] [--out FILE]
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
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--steps", default="16,32,64", help="round lengths to compare")
    ap.add_argument("--thresholds", default="0.05,0.02,0.01")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    steps = [int(x) for x in args.steps.split(",")]
    thresholds = [float(x) for x in args.thresholds.split(",")]

    import numpy as np
    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin, tiles

    work = Path(tempfile.mkdtemp(prefix="rbrt_adaptive_cost_"))
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
    counts = torch.zeros((tiles.n_tiles(w, h),), dtype=torch.int32, device="cuda")
    lines = [f"adaptive sampling on config 2: {w} x {h}, limit {n} spp, min_samples {args.min_samples}, {standin.BUNNY_TRIANGLES}-triangle stand-in, "
             f"blocking calls, median of {args.repeats}"]

    def timed(fn):
        ms, last = [], None
        for _ in range(args.repeats + 1):  # (the first one warms the handle: buffers, tile tables)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms[1:]), last

    with rbrt_amd.HipScene(host) as hs:
        hs.refine_wait(300.0)
        cull = hs.primary_cull(host.camera)
        lines.append(f"background-only tiles: {int((cull >> 31).sum())} of {cull.size} ({100.0 * float((cull >> 31).mean()):.1f} %)")
        fixed_ms, _ = timed(lambda: hs.render_device(host.camera, opts, rad.data_ptr(), rgb.data_ptr(), lens=host.lens))
        fixed8 = rgb.cpu().numpy().astype(np.int32)
        fixed_rad = rad.cpu().numpy()
        lines.append(f"{'':24s} {'ms':>9s} {'vs fixed':>9s} {'rounds':>6s} {'samples / fixed':>16s} {'mean |dRGB8|':>13s}")
        lines.append(f"{'fixed (render_device)':24s} {fixed_ms:9.2f} {1.0:9.3f} {'-':>6s} {1.0:16.4f} {0.0:13.4f}")
        for step in steps:
            ms, res = timed(lambda: hs.render_adaptive(host.camera, opts, 0.0, args.min_samples, step, rad.data_ptr(), rgb.data_ptr(),
                                                       counts.data_ptr(), lens=host.lens))
            same = bool(np.array_equal(rad.cpu().numpy().view(np.uint32), fixed_rad.view(np.uint32)))
            lines.append(f"{f'threshold 0, step {step}':24s} {ms:9.2f} {ms / fixed_ms:9.3f} {res['rounds']:6d} {res['samples'] / res['samples_fixed']:16.4f} "
                         f"{float(np.abs(rgb.cpu().numpy().astype(np.int32) - fixed8).mean()):13.4f}   image {'identical' if same else 'DIFFERS'}; "
                         f"{(ms - fixed_ms) / res['rounds']:.3f} ms per round over the fixed render")
        for thr in thresholds:
            for step in steps:
                ms, res = timed(lambda: hs.render_adaptive(host.camera, opts, thr, args.min_samples, step, rad.data_ptr(), rgb.data_ptr(),
                                                           counts.data_ptr(), lens=host.lens))
                active = hs.adaptive_rounds()
                lines.append(f"{f'threshold {thr:g}, step {step}':24s} {ms:9.2f} {ms / fixed_ms:9.3f} {res['rounds']:6d} {res['samples'] / res['samples_fixed']:16.4f} "
                             f"{float(np.abs(rgb.cpu().numpy().astype(np.int32) - fixed8).mean()):13.4f}   active tiles per round {active}")
        hs.check()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
