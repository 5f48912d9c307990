#!/usr/bin/env python3
"""What temporal accumulation costs on BASELINE config 2: scenes/example_scene.yaml with the 69,451-triangle stand-in at
1024 x 768, one GPU, one handle (the host builder's tree adopted first, as bench.py does).

  blocking frame    rbrt_hip_render_device at --samples and the synchronisation behind it, on the host's clock
  features          rbrt_hip_render_features at --feature-samples, between two events
  guided            rbrt_hip_scene_denoise_guided at its defaults on an adaptive render and those features, between two events:
                    the stage to compare with (five levels of 25 taps against one pass of four)
  temporal          rbrt_hip_temporal_accumulate with every output, between two events around --inner calls in a row (one call is
                    too short a window for the events' own resolution), per call:
                      first frame     no history: the halves pass through and the history is written
                      static camera   K' = K: every pixel reprojects onto itself
                      drift           K' = K moved by --drift along x (tools/moving_camera.py's 0.002 a frame), and ten times that
                    with the achieved bytes per second for the 170 bytes a pixel the stage has to move (A, B and N 36 in, depth
                    and coverage 8 in, four taps of the history's three records at most 192 but, the taps of neighbouring pixels
                    being the same records, 48 from memory; A', B' and len 28 out, the next history 48 out: 168, rounded), and
                    the share of pixels with a valid history (len > 1).
Every row warm (one untimed call first): the median, the least and the most of --repeats.

Prints a table; --out FILE also writes it there (profiles/temporal_config2.txt).

    python tools/temporal_cost.py [--samples 50] [--repeats 9] [--inner 20] [--out FILE]
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

BYTES_PER_PIXEL = 170


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--feature-samples", type=int, default=8)
    ap.add_argument("--drift", type=float, default=0.002)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    work = Path(tempfile.mkdtemp(prefix="rbrt_temporal_cost_"))
    obj = standin.ensure_obj(work / "bunny.obj", standin.BUNNY_TRIANGLES)
    (work / "scene.yaml").write_text((ROOT / "scenes" / "example_scene.yaml").read_text().replace("obj_filepath: bunny.obj", f"obj_filepath: {obj}"))
    devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(1)
    os.dup2(devnull, 1)  # (the host prints the reference's loading lines)
    try:
        host = abi.HostScene(work / "scene.yaml", args.height, args.width)
    finally:
        os.dup2(saved, 1)
        os.close(devnull)
    assert host.lens is None  # (a pinhole: the moved cameras below are plain copies)
    w, h, n = args.width, args.height, args.samples
    npix = w * h
    opts = abi.default_opts(spp=n, seed=1)
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    rad, out, ha, hb, oa, ob, albedo, normal = (new(h, w, 3) for _ in range(8))
    depth, coverage, length = (new(h, w) for _ in range(3))
    ws = torch.zeros((rbrt_amd.guided_workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
    hist = [torch.zeros((rbrt_amd.temporal_history_bytes(w, h),), dtype=torch.uint8, device="cuda") for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"temporal accumulation on config 2: {w} x {h}, {n} spp in one round (threshold 0), {standin.BUNNY_TRIANGLES}-triangle stand-in, "
             f"features at {args.feature_samples} samples, median (least - most) of {args.repeats} warm measurements",
             f"the temporal rows: events around {args.inner} calls in a row, per call; {BYTES_PER_PIXEL} bytes a pixel"]

    def row(name, ms, note=""):
        lines.append(f"{name:44s} {statistics.median(ms):8.3f} ms  ({min(ms):.3f} - {max(ms):.3f}){note}")
        return statistics.median(ms)

    def host_clock(call):
        ms = []
        for _ in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[1:]

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

    def cam_at(dx):
        c = type(host.camera).from_buffer_copy(host.camera)
        c.position[0] += dx
        c.img_center_point[0] += dx
        return c

    def accumulate(cam, prev, hin, hout):
        rbrt_amd.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), normal.data_ptr(), depth.data_ptr(), coverage.data_ptr(), cam, prev,
                                     hin.data_ptr() if hin is not None else None, hout.data_ptr(), oa.data_ptr(), ob.data_ptr(), length.data_ptr(),
                                     stream=stream)

    def temporal_row(name, cam, prev, hin, hout):
        ms = events(lambda: accumulate(cam, prev, hin, hout), args.inner)
        valid = float((length > 1).float().mean().item())
        t = statistics.median(ms)
        row(name, ms, f"   {BYTES_PER_PIXEL * npix / (t * 1e-3) / 1e12:5.2f} TB/s, valid history {100 * valid:6.2f} %, {t / guided:5.2f} x the guided filter")

    with rbrt_amd.HipScene(host) as hs:
        hs.refine_wait(300.0)
        row("blocking frame (host clock)", host_clock(lambda: hs.render_device(host.camera, opts, rad.data_ptr(), rgb.data_ptr())))
        hs.render_adaptive(host.camera, opts, 0.0, n, n, rad.data_ptr(), rgb.data_ptr())
        hs.denoise(None, None, ha.data_ptr(), hb.data_ptr())
        features = lambda cam: hs.render_features(cam, opts, args.feature_samples, albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(),
                                                  coverage.data_ptr(), stream=stream)
        row(f"features, {args.feature_samples} samples (events)", events(lambda: features(host.camera)))
        guided = row("guided L = 5, the library's default (events)",
                     events(lambda: hs.denoise_guided(albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(), coverage.data_ptr(), ws.data_ptr(),
                                                      out.data_ptr(), rgb.data_ptr(), stream=stream)))
        # the last frame's history: the same halves under each K' (what the stage costs does not depend on their values)
        temporal_row("temporal, first frame (events)", host.camera, None, None, hist[1])
        for name, dx in (("static camera", 0.0), (f"drift {args.drift:g}", args.drift), (f"drift {10 * args.drift:g}", 10 * args.drift)):
            prev = cam_at(-dx)
            features(prev)
            accumulate(prev, None, None, hist[0])
            features(host.camera)
            torch.cuda.synchronize()
            temporal_row(f"temporal, {name} (events)", host.camera, prev, hist[0], hist[1])
        hs.check()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
