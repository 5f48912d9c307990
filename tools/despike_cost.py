#!/usr/bin/env python3
"""What spike removal costs on BASELINE config 2: scenes/example_scene.yaml with the 69,451-triangle stand-in at 1024 x 768, one
GPU, one handle (the host builder's tree adopted first, as bench.py does).

  frame             rbrt_hip_render_adaptive (one round that stops nothing) at --samples, the handle's two half images
                    (rbrt_hip_scene_denoise) and their plain mix (rbrt_hip_denoise_halves, window radius 0), one
                    synchronisation, on the host's clock: what the command line's per-frame path does without the stage
  --despike frame   the same with rbrt_hip_despike_halves (defaults, every output) between the half images and the mix; and
                    its ratio to `frame`
  despike, R        rbrt_hip_despike_halves on that render's half images with every output, between two events around --inner
                    calls in a row (one call is too short a window for the events' own resolution), per call, for R = 1 and
                    R = 2 at rank 2, with the achieved bytes per second for the stage's algorithmic bytes: both halves read
                    once (24 bytes a pixel) and both halves and the mask written once (25 bytes a pixel). The halo that
                    neighbouring workgroups read again and each thread's second reading of its own two pixels are the
                    stage's own choice and not counted.
  yardstick         a device-to-device copy that moves as many bytes: a buffer of half of them, read and written, in the same
                    window; `ratio` is the stage's time over it
Every row warm (one untimed call first): the median, the least and the most of --repeats.
--kernels-only runs nothing but the stage on random halves, --inner times for R = 1 and for R = 2, for a kernel trace made around
this program.

Prints a table; --out FILE also writes it there (profiles/despike_config2.txt).

    python tools/despike_cost.py [--samples 50] [--repeats 9] [--inner 20] [--out FILE] [--kernels-only]
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


def algorithmic_bytes(w, h):
    return (24 + 25) * w * h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    w, h, n = args.width, args.height, args.samples
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ra, rb, oa, ob, rad = (new(h, w, 3) for _ in range(5))
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    res = torch.zeros((4,), dtype=torch.int32, device="cuda")

    def despike(radius=2):
        rbrt_amd.despike_halves(0, ra.data_ptr(), rb.data_ptr(), w, h, oa.data_ptr(), ob.data_ptr(), mask.data_ptr(), res.data_ptr(),
                                rbrt_amd.despike_opts(radius=radius), stream=stream)

    if args.kernels_only:
        ra.copy_(torch.rand_like(ra)), rb.copy_(torch.rand_like(rb))
        for radius in (1, 2):
            for _ in range(args.inner + 1):
                despike(radius)
        torch.cuda.synchronize()
        print(f"ran the stage {args.inner + 1} times for R = 1 and for R = 2 at {w} x {h}")
        return

    work = Path(tempfile.mkdtemp(prefix="rbrt_despike_cost_"))
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
    lines = [f"spike removal on config 2: {w} x {h}, {n} spp, {standin.BUNNY_TRIANGLES}-triangle stand-in, "
             f"median (least - most) of {args.repeats} warm measurements",
             f"the despike and yardstick rows: events around {args.inner} calls in a row, per call"]

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

        def frame(with_stage):
            hs.render_adaptive(host.camera, opts, 0.0, n, n, rad.data_ptr(), rgb.data_ptr())
            hs.denoise(None, None, ra.data_ptr(), rb.data_ptr(), stream=stream)
            if with_stage:
                despike()
            a, b = (oa, ob) if with_stage else (ra, rb)
            rbrt_amd.denoise_halves(0, a.data_ptr(), b.data_ptr(), None, w, h, rad.data_ptr(), rgb.data_ptr(), window_radius=0, stream=stream)

        plain = row("frame: render, halves, plain mix (host clock)", host_clock(lambda: frame(False)))
        ms = host_clock(lambda: frame(True))
        row("--despike frame: the same with the stage (host)", ms, f"   {statistics.median(ms) / plain:5.3f} x the frame without")
        torch.cuda.synchronize()
        counts = res.cpu().numpy()
        lines.append(f"(the stage limits {int(counts[0])} pixels of A and {int(counts[1])} of B in this render)")
        nbytes = algorithmic_bytes(w, h)
        src = torch.zeros((nbytes // 2,), dtype=torch.uint8, device="cuda")
        dst = torch.zeros_like(src)
        for radius in (1, 2):
            t = row(f"despike, R = {radius}, k = 2 (events)", events(lambda: despike(radius), args.inner), f"   {nbytes / 1e6:6.1f} MB")
            lines[-1] += f", {nbytes / (t * 1e-3) / 1e12:5.2f} TB/s"
            ys = events(lambda: dst.copy_(src), args.inner)
            row(f"yardstick: copy moving {nbytes / 1e6:.1f} MB (events)", ys, f"   the stage is {t / statistics.median(ys):.2f} x it")
        hs.check()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
