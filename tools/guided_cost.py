#!/usr/bin/env python3
"""What the guided denoiser costs on BASELINE config 2: scenes/example_scene.yaml with the 69,451-triangle stand-in at
1024 x 768, one GPU, one handle (the host builder's tree adopted first, as bench.py does).

  blocking frame    rbrt_hip_render_device at --samples and the synchronisation behind it, on the host's clock
  adaptive render   rbrt_hip_render_adaptive at --samples with threshold 0 in one round (what --denoise-guided runs)
  features          rbrt_hip_render_features at --feature-samples, between two events
  NLM               rbrt_hip_scene_denoise at its defaults on that render, between two events: the filter to compare with
  guided            rbrt_hip_scene_denoise_guided on that render and those features (the half images, the prepare kernel and
                    the levels) for every L of --levels, between two events, with the level kernel reading global memory
  staging           the same at --staging-levels with the levels up to step 1, 2 and 4 staging their tile in LDS
                    (rbrt_hip_debug_guided_staging): what LDS gains or loses at each step
Every row warm (one untimed call first): the median, the least and the most of --repeats.

Prints a table; --out FILE also writes it there (profiles/guided_config2.txt).

    python tools/guided_cost.py [--samples 50] [--levels 1,5,6] [--repeats 9] [--out FILE]
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
    ap.add_argument("--feature-samples", type=int, default=8)
    ap.add_argument("--levels", default="1,5,6")
    ap.add_argument("--staging-levels", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    levels = [int(v) for v in args.levels.split(",")]

    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    work = Path(tempfile.mkdtemp(prefix="rbrt_guided_cost_"))
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
    albedo, normal = (torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    depth, coverage = (torch.zeros((h, w), dtype=torch.float32, device="cuda") for _ in range(2))
    ws = torch.zeros((rbrt_amd.guided_workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    default_staging = rbrt_amd.guided_staging()
    lines = [f"the guided denoiser on config 2: {w} x {h}, {n} spp in one round (threshold 0), {standin.BUNNY_TRIANGLES}-triangle stand-in, "
             f"features at {args.feature_samples} samples, median (least - most) of {args.repeats} warm calls",
             f"the library's default: levels up to step {default_staging} stage their tile in LDS"]

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

    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.repeats + 1):
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms[1:]

    def guided(L):
        hs.denoise_guided(albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(), coverage.data_ptr(), ws.data_ptr(), out.data_ptr(),
                          rgb.data_ptr(), rbrt_amd.guided_opts(levels=L), stream=stream)

    with rbrt_amd.HipScene(host) as hs:
        hs.refine_wait(300.0)
        row("blocking frame (host clock)", host_clock(lambda: hs.render_device(host.camera, opts, rad.data_ptr(), rgb.data_ptr(), lens=host.lens)))
        row("adaptive render (host clock)", host_clock(lambda: hs.render_adaptive(host.camera, opts, 0.0, n, n, rad.data_ptr(), rgb.data_ptr(), lens=host.lens)))
        row(f"features, {args.feature_samples} samples (events)",
            events(lambda: hs.render_features(host.camera, opts, args.feature_samples, albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(),
                                              coverage.data_ptr(), lens=host.lens, stream=stream)))
        nlm = row("NLM R = 5, P = 3 (events)", events(lambda: hs.denoise(out.data_ptr(), rgb.data_ptr(), stream=stream)))
        taps = 25.0 * w * h
        rbrt_amd.guided_staging(0)
        for L in levels:
            ms = events(lambda: guided(L))
            row(f"guided L = {L}, global reads (events)", ms,
                f"   {4 * taps * L / 1e9:5.2f} G divisions (an upper bound), {statistics.median(ms) / nlm:5.2f} x the NLM")
        L = args.staging_levels
        for m in (0, 1, 2, 4):
            rbrt_amd.guided_staging(m)
            row(f"guided L = {L}, LDS up to step {m} (events)", events(lambda: guided(L)))
        rbrt_amd.guided_staging(default_staging)
        row(f"guided L = 5, the library's default (events)", events(lambda: guided(5)))
        hs.check()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
