#!/usr/bin/env python3
"""What image comparison costs, and what the reconstruction stages buy, on BASELINE config 2: scenes/example_scene.yaml with the
69,451-triangle stand-in at 1024 x 768, one GPU.

  compare           rbrt_hip_compare_images on two images of that size (random, 10 % apart) between two events around --inner
                    calls in a row (one call is too short a window for the events' own resolution), per call: with every
                    output, with the result alone and with the relative-error map alone (which makes no SSIM), and the achieved
                    bytes per second for the stage's algorithmic bytes: both images read once (24 bytes a pixel) and each map
                    that is asked for written once (4 bytes a pixel). The halo that neighbouring workgroups read again, each
                    thread's second reading of its own two pixels and the 48 bytes a tile of the workspace are the stage's own
                    choice and not counted.
  yardstick         a device-to-device copy that moves as many bytes as the call with every output: a buffer of half of them,
                    read and written, in the same window; `ratio` is the stage's time over it
  quality           the command line at --samples a pixel against a reference of --ref-samples from another seed
                    (--radiance), through --compare: plain, --denoise, --denoise-guided, --despike --denoise-guided and
                    --upscale 2 --denoise-guided. relMSE (epsilon 0.01), mean SSIM and PSNR are the report's compare_*; the
                    frame is the report's render_s + gather_s (the passes, the feature buffers and the filters; a fresh
                    process each, so the first launch of every kernel is in it), compare_ms the stage between its two events.
Every `compare` row warm (one untimed window first): the median, the least and the most of --repeats.

Prints a table; --out FILE also writes it there (profiles/compare_config2.txt).

    python tools/compare_cost.py [--samples 16] [--ref-samples 4096] [--repeats 9] [--inner 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
sys.path.insert(0, str(ROOT))

VARIANTS = [("plain", []), ("--denoise", ["--denoise"]), ("--denoise-guided", ["--denoise-guided"]),
            ("--despike --denoise-guided", ["--despike", "--denoise-guided"]), ("--upscale 2 --denoise-guided", ["--upscale", "2", "--denoise-guided"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--ref-samples", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    w, h = args.width, args.height
    stream = torch.cuda.current_stream().cuda_stream
    ref = torch.rand((h, w, 3), dtype=torch.float32, device="cuda")
    x = ref * (1.0 + 0.1 * (torch.rand_like(ref) - 0.5))
    rel, ssim = (torch.zeros((h, w), dtype=torch.float32, device="cuda") for _ in range(2))
    ws = torch.zeros((rbrt_amd.compare_workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
    res = torch.zeros((64,), dtype=torch.uint8, device="cuda")

    def compare(want):
        rbrt_amd.compare_images(0, x.data_ptr(), ref.data_ptr(), w, h, ws.data_ptr() if "result" in want else None, rel.data_ptr() if "rel" in want else None,
                                ssim.data_ptr() if "ssim" in want else None, res.data_ptr() if "result" in want else None, stream=stream)

    lines = [f"image comparison on config 2: {w} x {h}, median (least - most) of {args.repeats} warm measurements",
             f"the compare and yardstick rows: events around {args.inner} calls in a row, per call"]

    def row(name, ms, note=""):
        lines.append(f"{name:52s} {statistics.median(ms):8.3f} ms  ({min(ms):.3f} - {max(ms):.3f}){note}")
        return statistics.median(ms)

    def events(call, inner):
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

    full = 0.0
    for name, want, per_pixel in (("compare: result and both maps (events)", ("result", "rel", "ssim"), 32), ("compare: the result alone (events)", ("result",), 24),
                                  ("compare: the relative-error map alone (events)", ("rel",), 28)):
        nbytes = per_pixel * w * h
        t = row(name, events(lambda: compare(want), args.inner), f"   {nbytes / 1e6:6.1f} MB")
        lines[-1] += f", {nbytes / (t * 1e-3) / 1e12:5.2f} TB/s"
        full = full or t
    nbytes = 32 * w * h
    src = torch.zeros((nbytes // 2,), dtype=torch.uint8, device="cuda")
    dst = torch.zeros_like(src)
    ys = events(lambda: dst.copy_(src), args.inner)
    row(f"yardstick: copy moving {nbytes / 1e6:.1f} MB (events)", ys, f"   the stage with every output is {full / statistics.median(ys):.2f} x it")
    r = abi.CompareResult.from_buffer_copy(res.cpu().numpy().tobytes())
    s = rbrt_amd.compare_summary(r, w, h)
    lines.append(f"(these two images: relmse {s.relmse:.6g}, ssim {s.ssim:.6f}, {r.usable} pixels usable)")
    del src, dst, ref, x, rel, ssim, ws, res
    torch.cuda.synchronize()

    # ---- the quality table: the command line against a reference of many samples --------------------------------------------------
    work = Path(tempfile.mkdtemp(prefix="rbrt_compare_cost_"))
    obj = standin.ensure_obj(work / "bunny.obj", standin.BUNNY_TRIANGLES)
    (work / "scene.yaml").write_text((ROOT / "scenes" / "example_scene.yaml").read_text().replace("obj_filepath: bunny.obj", f"obj_filepath: {obj}"))
    common = [str(EXE), "-c", str(work / "scene.yaml"), "--height", str(h), "-w", str(w), "-t", str(work / "out.ppm")]
    ref_pfm = work / "ref.pfm"
    subprocess.run([*common, "-s", str(args.ref_samples), "--seed", "1000", "--radiance", str(ref_pfm)], check=True, capture_output=True, timeout=600)
    lines.append("")
    lines.append(f"quality at {args.samples} spp (seed 1) against a reference of {args.ref_samples} spp (seed 1000), {standin.BUNNY_TRIANGLES}-triangle stand-in; "
                 "the frame is render_s + gather_s of a fresh process")
    lines.append(f"{'':32s} {'relMSE':>12s} {'SSIM':>9s} {'PSNR dB':>9s} {'MSE':>12s} {'skipped':>8s} {'frame ms':>9s} {'compare ms':>11s}")
    for name, flags in VARIANTS:
        out = subprocess.run([*common, "-s", str(args.samples), "--seed", "1", *flags, "--compare", str(ref_pfm), "--report", str(work / "rep.json")], check=True,
                             capture_output=True, timeout=600)
        del out
        js = json.loads((work / "rep.json").read_text())
        frame_ms = (js["render_s"] + js["gather_s"]) * 1e3
        lines.append(f"{name:32s} {float(js['compare_relmse']):12.6g} {float(js['compare_ssim']):9.5f} {float(js['compare_psnr_db']):9.3f} {float(js['compare_mse']):12.6g} "
                     f"{js['compare_skipped']:8d} {frame_ms:9.3f} {js['compare_ms']:11.4f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
