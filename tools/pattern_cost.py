#!/usr/bin/env python3
"""What a solid checker costs, and what albedo demodulation buys on an image whose albedo changes inside an object.

  frame     BASELINE config 2 -- bench.py's frame: scenes/example_scene.yaml with the 69,451-triangle stand-in,
            1024 x 768 x 50 spp, one GPU -- with the ground plain and with the ground checkered (scenes/checker/checker_ground.yaml's
            keys on the ground sphere), in alternating rounds of timed render_device steps on one handle each, in one process
            (the host builder's tree adopted first, as bench.py does): ms per step of every round, the medians, their ratio.
  quality   the command line on scenes/checker/checker_ground.yaml at --samples a pixel against a reference of --ref-samples from
            another seed (--radiance), through --compare: plain, --denoise-guided (with demodulation) and --denoise-guided
            --guided-no-demodulation (RBRT_GUIDED_NO_DEMODULATION). relMSE (epsilon 0.01), mean SSIM and PSNR are the report's.
Nothing here is a threshold: the output is the record (profiles/pattern_config2.txt).

    python tools/pattern_cost.py [--steps 20] [--warmup 3] [--rounds 3] [--samples 16] [--ref-samples 4096] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
sys.path.insert(0, str(ROOT))

CHECKER_KEYS = ("    checker_albedo:\n      x: 0.8\n      y: 0.8\n      z: 0.7\n    checker_size: 2.0\n"
                "    checker_origin:\n      x: 0.0\n      y: -1.0\n      z: 0.0\n")
VARIANTS = [("plain", []), ("--denoise-guided", ["--denoise-guided"]),
            ("--denoise-guided --guided-no-demodulation", ["--denoise-guided", "--guided-no-demodulation"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--spp", type=int, default=50)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--ref-samples", type=int, default=4096)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import rbrt_amd
    from rbrt_amd import abi, standin

    w, h = args.width, args.height
    work = Path(tempfile.mkdtemp(prefix="rbrt_pattern_cost_"))
    obj = standin.ensure_obj(work / "bunny.obj", standin.BUNNY_TRIANGLES)
    text = (ROOT / "scenes" / "example_scene.yaml").read_text().replace("obj_filepath: bunny.obj", f"obj_filepath: {obj}")
    ground = "    albedo:\n      x: 0.02\n      y: 0.2\n      z: 0.1\n"  # the green earth's
    assert text.count(ground) == 1
    (work / "plain.yaml").write_text(text)
    (work / "checker.yaml").write_text(text.replace(ground, ground + CHECKER_KEYS))
    devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(1)
    os.dup2(devnull, 1)  # (the host prints the reference's loading lines)
    try:
        hosts = {k: abi.HostScene(work / f"{k}.yaml", h, w) for k in ("plain", "checker")}
    finally:
        os.dup2(saved, 1)
        os.close(devnull)
    assert hosts["plain"].patterns is None and hosts["checker"].patterns is not None
    handles = {k: rbrt_amd.HipScene(hs) for k, hs in hosts.items()}
    for hd in handles.values():
        hd.refine_wait(300.0)
    lds = {k: hd.info()["lds_bytes_per_wave"] for k, hd in handles.items()}
    opts = abi.default_opts(spp=args.spp, seed=1)
    image = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ms = {k: [] for k in handles}
    for _ in range(args.rounds):
        for k, hd in handles.items():
            cam = hosts[k].camera
            for _ in range(args.warmup):
                hd.render_device(cam, opts, image.data_ptr(), None, stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                hd.render_device(cam, opts, image.data_ptr(), None, stream)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
            hd.check()
    for hd in handles.values():
        hd.close()
    del image
    torch.cuda.synchronize()
    samples = w * h * args.spp
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [f"a solid checker on config 2's ground: {w} x {h} x {args.spp} spp, {standin.BUNNY_TRIANGLES}-triangle stand-in, "
             f"{args.rounds} alternating rounds of {args.steps} steps in one process"]
    for k in ("plain", "checker"):
        lines.append(f"{'ground ' + k:18s} {med[k]:8.4f} ms per step  ({', '.join(f'{x:.4f}' for x in ms[k])})   "
                     f"{samples / (med[k] * 1e-3) / 1e6:8.1f} Mray-samples/s   LDS {lds[k]} bytes per wave")
    lines.append(f"checker over plain {med['checker'] / med['plain']:.4f}")

    # ---- the quality rows: the shipped scene through the command line ---------------------------------------------------------------
    common = [str(EXE), "-c", str(ROOT / "scenes" / "checker" / "checker_ground.yaml"), "--height", str(h), "-w", str(w), "-t", str(work / "out.ppm")]
    ref_pfm = work / "ref.pfm"
    subprocess.run([*common, "-s", str(args.ref_samples), "--seed", "1000", "--radiance", str(ref_pfm)], check=True, capture_output=True, timeout=900)
    lines.append("")
    lines.append(f"quality of scenes/checker/checker_ground.yaml at {args.samples} spp (seed 1) against a reference of {args.ref_samples} spp (seed 1000); "
                 "the frame is render_s + gather_s of a fresh process")
    lines.append(f"{'':44s} {'relMSE':>12s} {'SSIM':>9s} {'PSNR dB':>9s} {'MSE':>12s} {'skipped':>8s} {'frame ms':>9s}")
    for name, flags in VARIANTS:
        subprocess.run([*common, "-s", str(args.samples), "--seed", "1", *flags, "--compare", str(ref_pfm), "--report", str(work / "rep.json")], check=True,
                       capture_output=True, timeout=900)
        js = json.loads((work / "rep.json").read_text())
        frame_ms = (js["render_s"] + js["gather_s"]) * 1e3
        lines.append(f"{name:44s} {float(js['compare_relmse']):12.6g} {float(js['compare_ssim']):9.5f} {float(js['compare_psnr_db']):9.3f} "
                     f"{float(js['compare_mse']):12.6g} {js['compare_skipped']:8d} {frame_ms:9.3f}")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(out)


if __name__ == "__main__":
    main()
