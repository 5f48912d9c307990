#!/usr/bin/env python3
"""What the glare stage costs on BASELINE config 2: scenes/example_scene.yaml with the 69,451-triangle stand-in at
1024 x 768, one GPU, one handle (the host builder's tree adopted first, as bench.py does).

  render      rbrt_hip_render_device at --samples, a blocking frame: timed from the call to the synchronisation behind it
  denoise     rbrt_hip_scene_denoise with the default options on the half images of the same frame rendered in one adaptive
              round, between two events
  tonemap     rbrt_hip_tonemap on that frame's radiance, automatic exposure and ACES, between two events
  glare       rbrt_hip_glare on that frame's radiance (float in, float out), between two events on the stream, at 1, 5 and 8
              levels: 2 L launches. The threshold is the frame's 90th percentile luminance: a tenth of its pixels are bright.
              Each row warm (one untimed call first), the median, the least and the most of --repeats, and the bytes the
              kernels move over the median: the image read twice (bright pass, composite) and written once, 12 B a pixel,
              and every level of the pyramid, 16 B a pixel, written once and read once or twice

Prints a table; --out FILE also writes it there (profiles/glare_config2.txt).

    python tools/glare_cost.py [--samples 50] [--repeats 9] [--out FILE]
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
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    work = Path(tempfile.mkdtemp(prefix="rbrt_glare_cost_"))
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
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    tws = torch.zeros(abi.TONEMAP_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda")
    lines = [f"the glare stage on config 2: {w} x {h}, {n} spp, {standin.BUNNY_TRIANGLES}-triangle stand-in, "
             f"median (least - most) of {args.repeats} warm calls"]

    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.repeats + 1):  # (the first one is not counted)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms[1:]), min(ms[1:]), max(ms[1:])

    with rbrt_amd.HipScene(host) as hs:
        hs.refine_wait(300.0)
        ms = []
        for _ in range(args.repeats + 1):  # (the first one warms the handle)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hs.render_device(host.camera, opts, rad.data_ptr(), rgb.data_ptr(), lens=host.lens)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        frame = statistics.median(ms[1:])
        lines.append(f"{'render, blocking (host clock)':44s} {frame:8.3f} ms  ({min(ms[1:]):.3f} - {max(ms[1:]):.3f})")
        hs.check()
        stream = torch.cuda.current_stream().cuda_stream
        # the denoiser needs the half images of an adaptive render: threshold 0 in one round is what --denoise alone renders
        hs.render_adaptive(host.camera, opts, 0.0, n, n, out.data_ptr(), rgb.data_ptr(), lens=host.lens)
        torch.cuda.synchronize()
        med, lo, hi = events(lambda: hs.denoise(out.data_ptr(), rgb.data_ptr(), window_radius=5, patch_radius=3, strength=0.7, stream=stream))
        lines.append(f"{'denoise: R = 5, P = 3 (events)':44s} {med:8.4f} ms  ({lo:.4f} - {hi:.4f})   {100.0 * med / frame:5.2f} % of the frame")
        hs.check()
        t = rbrt_amd.tonemap_opts(abi.TONE_ACES, exposure=0.0, white=1.0)
        med, lo, hi = events(lambda: rbrt_amd.tonemap(0, rad.data_ptr(), w * h, t, tws.data_ptr(), None, rgb.data_ptr(), stream=stream))
        lines.append(f"{'tonemap: automatic exposure, ACES (events)':44s} {med:8.4f} ms  ({lo:.4f} - {hi:.4f})   {100.0 * med / frame:5.2f} % of the frame")
        # the threshold that makes a tenth of the frame bright
        x = rad.cpu().numpy()
        lum = 0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]
        threshold = float(np.quantile(lum, 0.9))
        for levels in (1, 5, 8):
            g = rbrt_amd.glare_opts(threshold=threshold, intensity=0.1, levels=levels, spread=1.0)
            need = rbrt_amd.glare_workspace_bytes(w, h, levels)
            ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
            med, lo, hi = events(lambda: rbrt_amd.glare(0, rad.data_ptr(), w, h, g, ws.data_ptr(), out.data_ptr(), None, stream=stream))
            moved = w * h * 36 + need * 3  # (an upper bound for the pyramid: the last level is read once)
            changed = int((out.cpu().numpy() != x).any(axis=2).sum())
            lines.append(f"{f'glare: {levels} level(s), {2 * levels} launches (events)':44s} {med:8.4f} ms  ({lo:.4f} - {hi:.4f})   {100.0 * med / frame:5.2f} % of the frame, "
                         f"{moved / med / 1e6:7.1f} GB/s; workspace {need} B, threshold {threshold:.4g}, {changed} pixels changed")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
