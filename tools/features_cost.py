#!/usr/bin/env python3
"""What the feature buffers cost on BASELINE config 2: scenes/example_scene.yaml with the 69,451-triangle stand-in at
1024 x 768, one GPU, one handle (the host builder's tree adopted first, as bench.py does), all in one session.

  render      rbrt_hip_render_device at --samples, a blocking frame: timed from the call to the synchronisation behind it;
              and that frame's rays per pixel, from one run with RBRT_FLAG_COLLECT_STATS (rays / (width * height))
  features    rbrt_hip_render_features with all five outputs at n = 1, 4, 8 samples a pixel, between two events on the
              stream, warm (one untimed call first): the median, the least and the most of --repeats. Once with the pinhole
              camera and once with the lens of scenes/defocus_spheres.yaml (its aperture and focus distance on this camera),
              each against a frame rendered with the same camera
  yardstick   n * frame_ms / rays_per_pixel: what the trace kernel pays for as many rays. `ratio` is the measured time over it
  and what decides a call's time: n = 1 with seeds 2..8 (other rays, the same work), and n = 8 with the same view at a
  quarter of the pixels (a quarter of the work)

Prints a table; --out FILE also writes it there (profiles/features_config2.txt).

    python tools/features_cost.py [--samples 50] [--repeats 9] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
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

    work = Path(tempfile.mkdtemp(prefix="rbrt_features_cost_"))
    obj = standin.ensure_obj(work / "bunny.obj", standin.BUNNY_TRIANGLES)
    text = (ROOT / "scenes" / "example_scene.yaml").read_text().replace("obj_filepath: bunny.obj", f"obj_filepath: {obj}")
    (work / "scene.yaml").write_text(text)
    # the same scene and camera with defocus_spheres.yaml's lens
    defocus = (ROOT / "scenes" / "defocus_spheres.yaml").read_text()
    lens_keys = ""
    for k in ("camera_aperture_mm", "camera_focus_distance"):
        lens_keys += "\n  " + k + ": " + re.search(r"^  " + k + r": *(\S+)", defocus, re.M).group(1)
    (work / "scene_lens.yaml").write_text(re.sub(r"^(  camera_focal_length_mm: *\S+)", lambda m: m.group(1) + lens_keys, text, count=1, flags=re.M))
    devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(1)
    os.dup2(devnull, 1)  # (the host prints the reference's loading lines)
    try:
        host = abi.HostScene(work / "scene.yaml", args.height, args.width)
        host_lens = abi.HostScene(work / "scene_lens.yaml", args.height, args.width)
        host_quarter = abi.HostScene(work / "scene.yaml", args.height // 2, args.width // 2)  # (its camera: the same view, a quarter of the pixels)
    finally:
        os.dup2(saved, 1)
        os.close(devnull)
    assert host.lens is None and host_lens.lens is not None
    w, h, spp = args.width, args.height, args.samples
    opts = abi.default_opts(spp=spp, seed=1)
    rad = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    albedo, normal = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"), torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    depth, coverage = torch.zeros((h, w), dtype=torch.float32, device="cuda"), torch.zeros((h, w), dtype=torch.float32, device="cuda")
    objects = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    lines = [f"the feature buffers on config 2: {w} x {h}, {spp} spp, {standin.BUNNY_TRIANGLES}-triangle stand-in, "
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
        info = hs.info()
        lines.append(f"traversal stack: {info['bvh_stack_need']} entries a lane, {info['bvh_stack_need'] * 256} B of LDS a wave")
        stream = torch.cuda.current_stream().cuda_stream
        for name, lens in (("pinhole", None), ("lens (defocus_spheres.yaml's)", host_lens.lens)):
            ms = []
            for _ in range(args.repeats + 1):  # (the first one warms the handle)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hs.render_device(host.camera, opts, rad.data_ptr(), lens=lens)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            frame = statistics.median(ms[1:])
            hs.check()
            counting = abi.default_opts(spp=spp, seed=1, flags=abi.FLAG_COLLECT_STATS)
            hs.render_device(host.camera, counting, rad.data_ptr(), lens=lens)
            torch.cuda.synchronize()
            rays_per_pixel = hs.stats()["rays"] / float(w * h)
            lines.append(f"{name}: render, blocking (host clock) {frame:8.3f} ms  ({min(ms[1:]):.3f} - {max(ms[1:]):.3f}), "
                         f"{rays_per_pixel:.2f} rays a pixel, {frame / rays_per_pixel * 1e3:.2f} us per ray-per-pixel")
            for n in (1, 4, 8):
                med, lo, hi = events(lambda: hs.render_features(host.camera, opts, n, albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(),
                                                                coverage.data_ptr(), objects.data_ptr(), lens=lens, stream=stream))
                yard = n * frame / rays_per_pixel
                lines.append(f"  {f'features, n = {n} (events)':32s} {med:8.4f} ms  ({lo:.4f} - {hi:.4f})   {100.0 * med / frame:5.2f} % of the frame; "
                             f"yardstick {yard:.4f} ms, ratio {med / yard:.2f}; coverage {float(coverage.mean()):.4f}")
            # what decides a call's time: other rays (seeds 2..8 at n = 1), and a quarter of the pixels (n = 8, seed 1)
            by_seed = [events(lambda: hs.render_features(host.camera, abi.default_opts(spp=spp, seed=seed), 1, albedo.data_ptr(), normal.data_ptr(),
                                                         depth.data_ptr(), coverage.data_ptr(), objects.data_ptr(), lens=lens, stream=stream))[0]
                       for seed in range(2, 9)]
            lines.append(f"  {'n = 1, seeds 2..8 (medians)':32s} " + " ".join(f"{x:.4f}" for x in by_seed) + " ms")
            quarter = abi.Camera()
            C.memmove(C.byref(quarter), C.byref(host_quarter.camera), C.sizeof(abi.Camera))
            med, lo, hi = events(lambda: hs.render_features(quarter, opts, 8, albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(), coverage.data_ptr(),
                                                            objects.data_ptr(), lens=lens, stream=stream))
            lines.append(f"  {f'n = 8 at {w // 2} x {h // 2} (events)':32s} {med:8.4f} ms  ({lo:.4f} - {hi:.4f})")
            hs.check()
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if args.out:
        Path(args.out).write_text(out)


if __name__ == "__main__":
    main()
