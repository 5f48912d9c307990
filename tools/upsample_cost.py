#!/usr/bin/env python3
"""What guided upsampling costs, and what a frame traced at half size saves, on BASELINE config 2: scenes/example_scene.yaml with
the 69,451-triangle stand-in at 1024 x 768, one GPU, one handle (the host builder's tree adopted first, as bench.py does).

  full frame        rbrt_hip_render_device with the full camera at --samples and the synchronisation behind it, on the host's clock
  features          rbrt_hip_render_features with the full camera at --feature-samples, between two events
  full + features   the two in a row, one synchronisation, on the host's clock: what a frame for the guided filter costs today
  low frame         rbrt_hip_render_device with the low camera of rbrt_hip_upsample_camera(f = 2), on the host's clock
  --upscale 2 frame the low frame, the full-size features and rbrt_hip_upsample_halves in a row, one synchronisation, on the host's
                    clock; and its ratio to `full + features`
  upsample, f       rbrt_hip_upsample_halves (its reduce and its gather kernel) with every output, between two events around
                    --inner calls in a row (one call is too short a window for the events' own resolution), per call, for
                    f = 2 and f = 4, with the achieved bytes per second for the stage's algorithmic bytes: every input read
                    once (the low halves 24 bytes a low pixel, the features 32 bytes a full pixel) and every output written
                    once (28 bytes a full pixel). The workspace (64 bytes a low pixel written and read) and the second reading
                    of the features are the stage's own choice and not counted.
  yardstick, f      a device-to-device copy of a buffer of that many bytes (which reads and writes each of them), the same
                    window; `ratio` is the stage's time over it
Every row warm (one untimed call first): the median, the least and the most of --repeats.
--kernels-only runs nothing but the stage, --inner times for f = 2 and for f = 4, for a kernel trace made around this program.

Prints a table; --out FILE also writes it there (profiles/upsample_config2.txt).

    python tools/upsample_cost.py [--samples 50] [--repeats 9] [--inner 20] [--out FILE] [--kernels-only]
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


def algorithmic_bytes(w, h, f):
    lw, lh = (w + f - 1) // f, (h + f - 1) // f
    return 24 * lw * lh + (32 + 28) * w * h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--feature-samples", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    w, h, n = args.width, args.height, args.samples
    npix = w * h
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    albedo, normal, oa, ob = (new(h, w, 3) for _ in range(4))
    depth, coverage, ow = (new(h, w) for _ in range(3))
    ws = torch.zeros((rbrt_amd.upsample_workspace_bytes(w, h, 1),), dtype=torch.uint8, device="cuda")
    low_halves = {}
    for f in (2, 4):
        lw, lh = (w + f - 1) // f, (h + f - 1) // f
        low_halves[f] = (torch.rand((lh, lw, 3), dtype=torch.float32, device="cuda"), torch.rand((lh, lw, 3), dtype=torch.float32, device="cuda"))

    def upsample(f, la, lb):
        rbrt_amd.upsample_halves(0, la.data_ptr(), lb.data_ptr(), None, albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(), coverage.data_ptr(),
                                 w, h, ws.data_ptr(), oa.data_ptr(), ob.data_ptr(), ow.data_ptr(), rbrt_amd.upsample_opts(factor=f), stream=stream)

    if args.kernels_only:  # (synthetic features: a slope and two albedos, so that taps are both accepted and rejected)
        x = torch.arange(w, dtype=torch.float32, device="cuda")[None, :].expand(h, w)
        depth.copy_(5.0 + 0.01 * x)
        coverage.fill_(1.0)
        normal[..., 2] = 1.0
        albedo[:, : w // 2] = 0.8
        albedo[:, w // 2:] = 0.2
        for f in (2, 4):
            for _ in range(args.inner + 1):
                upsample(f, *low_halves[f])
        torch.cuda.synchronize()
        print(f"ran the stage {args.inner + 1} times for f = 2 and for f = 4 at {w} x {h}")
        return

    work = Path(tempfile.mkdtemp(prefix="rbrt_upsample_cost_"))
    obj = standin.ensure_obj(work / "bunny.obj", standin.BUNNY_TRIANGLES)
    (work / "scene.yaml").write_text((ROOT / "scenes" / "example_scene.yaml").read_text().replace("obj_filepath: bunny.obj", f"obj_filepath: {obj}"))
    devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(1)
    os.dup2(devnull, 1)  # (the host prints the reference's loading lines)
    try:
        host = abi.HostScene(work / "scene.yaml", args.height, args.width)
    finally:
        os.dup2(saved, 1)
        os.close(devnull)
    assert host.lens is None
    opts = abi.default_opts(spp=n, seed=1)
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    rad = new(h, w, 3)
    low = rbrt_amd.upsample_camera(host.camera, 2)
    lw, lh = low.img_width_pix, low.img_height_pix
    la, lb, lrad = new(lh, lw, 3), new(lh, lw, 3), new(lh, lw, 3)
    lines = [f"guided upsampling on config 2: {w} x {h}, {n} spp, {standin.BUNNY_TRIANGLES}-triangle stand-in, features at {args.feature_samples} samples, "
             f"median (least - most) of {args.repeats} warm measurements",
             f"the upsample and yardstick rows: events around {args.inner} calls in a row, per call"]

    def row(name, ms, note=""):
        lines.append(f"{name:52s} {statistics.median(ms):8.3f} ms  ({min(ms):.3f} - {max(ms):.3f}){note}")
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

    with rbrt_amd.HipScene(host) as hs:
        hs.refine_wait(300.0)
        features = lambda: hs.render_features(host.camera, opts, args.feature_samples, albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(),
                                              coverage.data_ptr(), stream=stream)
        full = lambda: hs.render_device(host.camera, opts, rad.data_ptr(), rgb.data_ptr())
        small = lambda: hs.render_device(low, opts, lrad.data_ptr(), rgb.data_ptr())
        # the low halves of a real render, for the stage's rows at f = 2
        hs.render_adaptive(low, opts, 0.0, n, n, lrad.data_ptr(), rgb.data_ptr())
        hs.denoise(None, None, la.data_ptr(), lb.data_ptr())
        features()
        torch.cuda.synchronize()
        low_halves[2] = (la, lb)
        row("full frame, blocking (host clock)", host_clock(full))
        row(f"features, {args.feature_samples} samples (events)", events(features))
        both = row("full frame + features, blocking (host clock)", host_clock(lambda: (full(), features())))
        row(f"low frame {lw} x {lh}, blocking (host clock)", host_clock(small))
        ms = host_clock(lambda: (small(), features(), upsample(2, la, lb)))
        t = statistics.median(ms)
        row("--upscale 2 frame: low + features + upsample (host)", ms, f"   {t / both:5.3f} x the full frame + features")
        for f in (2, 4):
            a, b = low_halves[f]
            nbytes = algorithmic_bytes(w, h, f)
            t = row(f"upsample, f = {f} (events)", events(lambda: upsample(f, a, b), args.inner), f"   {nbytes / 1e6:6.1f} MB")
            lines[-1] += f", {nbytes / (t * 1e-3) / 1e12:5.2f} TB/s"
            src = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
            dst = torch.zeros_like(src)
            ys = events(lambda: dst.copy_(src), args.inner)
            row(f"yardstick: copy of {nbytes / 1e6:.1f} MB (events)", ys, f"   the stage is {t / statistics.median(ys):.2f} x it")
            del src, dst
        hs.check()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
