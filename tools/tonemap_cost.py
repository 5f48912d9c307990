#!/usr/bin/env python3
"""What the display transform costs on BASELINE config 2: scenes/example_scene.yaml with the 69,451-triangle stand-in at
1024 x 768, one GPU, one handle (the host builder's tree adopted first, as bench.py does).

  render      rbrt_hip_render_device at --samples, a blocking frame: timed from the call to the synchronisation behind it
  tonemap     rbrt_hip_tonemap on that frame's radiance (float in, rgb8 out), between two events on the stream, for
                manual exposure, no curve      the apply kernel alone
                automatic exposure, ACES       histogram + select + apply (a manual white: ACES reads none)
                both automatic, Reinhard       histogram + select (both ranks) + apply
              each row warm (one untimed call first), the median, the least and the most of --repeats, and the bytes the
              kernels move (12 B read per pixel and kernel that reads the image, 3 B written) over the median

Prints a table; --out FILE also writes it there (profiles/tonemap_config2.txt).

    python tools/tonemap_cost.py [--samples 50] [--repeats 9] [--out FILE]
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

    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    work = Path(tempfile.mkdtemp(prefix="rbrt_tonemap_cost_"))
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
    ws = torch.zeros(abi.TONEMAP_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda")
    lines = [f"the display transform on config 2: {w} x {h}, {n} spp, {standin.BUNNY_TRIANGLES}-triangle stand-in, "
             f"median (least - most) of {args.repeats} warm calls"]
    rows = [("manual exposure, no curve", rbrt_amd.tonemap_opts(abi.TONE_LINEAR, exposure=1.5, white=1.0), 1),
            ("automatic exposure, ACES", rbrt_amd.tonemap_opts(abi.TONE_ACES, exposure=0.0, white=1.0), 2),
            ("both automatic, Reinhard", rbrt_amd.tonemap_opts(abi.TONE_REINHARD, exposure=0.0, white=0.0), 2)]

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
        lines.append(f"{'render, blocking (host clock)':34s} {frame:8.3f} ms  ({min(ms[1:]):.3f} - {max(ms[1:]):.3f})")
        hs.check()
        stream = torch.cuda.current_stream().cuda_stream
        for name, o, reads in rows:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = []
            for _ in range(args.repeats + 1):
                e0.record()
                rbrt_amd.tonemap(0, rad.data_ptr(), w * h, o, ws.data_ptr(), None, rgb.data_ptr(), stream=stream)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms[1:])
            moved = w * h * (12 * reads + 3)
            res = abi.TonemapResult.from_buffer_copy(ws.cpu().numpy()[abi.TONEMAP_RESULT_OFFSET:].tobytes())
            lines.append(f"{f'tonemap: {name} (events)':44s} {med:8.4f} ms  ({min(ms[1:]):.4f} - {max(ms[1:]):.4f})   {100.0 * med / frame:5.2f} % of the frame, "
                         f"{moved / med / 1e6:7.1f} GB/s; e = {res.exposure:.6g}, w = {res.white:.6g}, {res.counted} counted")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
