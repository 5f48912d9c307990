"""The display transform on the host side: the PFM writer of --radiance, the command line's options and refusals (no GPU),
and, on the GPU, what the CLI writes with them against the numpy restatement (np_tonemap.py) of the radiance it wrote."""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_tonemap as N
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
SCENE = ROOT / "scenes" / "emissive_spheres.yaml"
f32, u32 = np.float32, np.uint32
W, H, SPP = 72, 40, 8


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


# ---- the PFM writer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (7, 5), (64, 1), (1, 33)])
def test_pfm_round_trip_gives_the_bits_back(tmp_path, w, h):
    rng = np.random.default_rng(100 * w + h)
    img = (rng.normal(0.0, 1.0, (h, w, 3)) * 10.0 ** rng.uniform(-30, 30, (h, w, 3))).astype(f32)
    flat = img.reshape(-1)
    specials = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42, -1e-42, np.finfo(f32).max], f32)
    flat[:min(flat.size, specials.size)] = specials[:flat.size]
    if flat.size > 12:
        flat[10:12] = np.array([0x7FC12345, 0xFFABCDEF], u32).view(f32)  # NaN payloads
    p = tmp_path / "r.pfm"
    abi.write_pfm(p, img)
    raw = p.read_bytes()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + w * h * 12
    # rows bottom to top, little-endian: said with numpy, not with the reader
    assert np.array_equal(np.frombuffer(raw[len(head):], "<u4").reshape(h, w, 3)[::-1], bits(img))
    assert np.array_equal(bits(abi.read_pfm(p, any_value=True)), bits(img))
    if h * w > 1:  # the reader of environment maps still refuses what is no radiance map
        with pytest.raises(RuntimeError, match="texel"):
            abi.read_pfm(p)


def test_pfm_writer_refusals(tmp_path):
    with pytest.raises(RuntimeError, match="cannot write"):
        abi.write_pfm(tmp_path / "no" / "such" / "dir.pfm", np.zeros((2, 2, 3), f32))
    lib = abi.load_host()
    z = np.zeros(3, f32)
    assert lib.rbrt_host_write_pfm(str(tmp_path / "z.pfm").encode(), abi.fptr(z), 0, 1) != 0 and b"size" in lib.rbrt_host_last_error()
    assert not (tmp_path / "z.pfm").exists()


# ---- the command line, without a GPU -----------------------------------------------------------------------------------------
def test_help_lists_the_options():
    assert EXE.exists(), "build the CLI with `make`"
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for opt in ("--exposure <EV|auto>", "--exposure-key <x>", "--tonemap <curve>", "--white <x|auto>", "--radiance <file.pfm>"):
        assert opt in r.stdout, opt
    head = (ROOT / "rbrt_amd" / "host" / "main.cpp").read_text().split("#include")[0]
    for opt in ("--exposure", "--exposure-key", "--tonemap", "--white", "--radiance"):
        assert opt in head, opt


@pytest.mark.parametrize("argv,names", [
    (["--exposure", "bright"], ["--exposure", "bright"]),
    (["--exposure", "nan"], ["--exposure"]),
    (["--exposure", "1000"], ["--exposure"]),
    (["--exposure"], ["--exposure"]),
    (["--tonemap", "filmic"], ["--tonemap", "filmic", "reinhard", "aces"]),
    (["--white", "2.0"], ["--white", "--tonemap reinhard"]),
    (["--white", "auto", "--tonemap", "aces"], ["--white", "--tonemap reinhard"]),
    (["--white", "0", "--tonemap", "reinhard"], ["--white"]),
    (["--white", "-1", "--tonemap", "reinhard"], ["--white"]),
    (["--radiance", "x.png"], ["--radiance", ".pfm"]),
    (["--radiance", "pfm"], ["--radiance", ".pfm"]),
    (["--exposure-key", "0"], ["--exposure-key"]),
    (["--exposure-key", "-0.18"], ["--exposure-key"]),
    (["--exposure-key", "inf"], ["--exposure-key"]),
])
def test_parse_errors(tmp_path, argv, names):
    """Refused by name, with exit code 2, before a scene is read or a device touched: nothing is written."""
    out = tmp_path / "x.ppm"
    r = subprocess.run([str(EXE), *argv, "-t", str(out), "-c", str(tmp_path / "no_such_scene.yaml")], capture_output=True, text=True)
    assert r.returncode == 2, (r.returncode, r.stderr)
    for name in names:
        assert name in r.stderr, (name, r.stderr)
    assert not out.exists()


# ---- the command line on the GPU ---------------------------------------------------------------------------------------------
def ppm(p, w=W, h=H):
    raw = Path(p).read_bytes()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)


def cli(tmp_path, name, *extra, w=W, h=H, spp=SPP):
    """One run on the emissive spheres under a black sky; returns (target, report)."""
    out, rep = tmp_path / f"{name}.ppm", tmp_path / f"{name}.json"
    argv = [str(EXE), "-c", str(SCENE), "-t", str(out), "--height", str(h), "-w", str(w), "-s", str(spp), "--seed", "3", "--background", "0,0,0",
            "--report", str(rep), *extra]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out, json.loads(rep.read_text())


NEW_FIELDS = ("tonemap", "exposure", "white", "luminance_counted", "tonemap_ms")


@pytest.mark.gpu
def test_the_defaults_write_what_they_always_wrote(hip, tmp_path):
    plain, js = cli(tmp_path, "plain")
    named, _ = cli(tmp_path, "named", "--exposure", "0", "--tonemap", "none")
    assert plain.read_bytes() == named.read_bytes()
    assert not [k for k in NEW_FIELDS if k in js]
    # ... which is the library's own rgb8
    import torch
    hsn = abi.HostScene(SCENE, H, W)
    o = abi.default_opts(spp=SPP, seed=3, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    with hip.HipScene(hsn) as hs:
        hs.render_device(hsn.camera, o, None, rgb.data_ptr(), lens=hsn.lens)
        torch.cuda.synchronize()
        hs.check()
    assert np.array_equal(ppm(plain), rgb.cpu().numpy())


@pytest.mark.gpu
def test_radiance_file_holds_the_librarys_radiance(hip, tmp_path):
    import torch
    pfm = tmp_path / "r.pfm"
    out, js = cli(tmp_path, "r", "--radiance", str(pfm), "--exposure", "1.5", "--tonemap", "aces")
    hsn = abi.HostScene(SCENE, H, W)
    o = abi.default_opts(spp=SPP, seed=3, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    with hip.HipScene(hsn) as hs:
        hs.render_device(hsn.camera, o, rad.data_ptr(), lens=hsn.lens)
        torch.cuda.synchronize()
        hs.check()
    got = abi.read_pfm(pfm, any_value=True)
    assert np.array_equal(bits(got), bits(rad.cpu().numpy())) and (got > 1.0).any()  # linear: the exposure is not in it
    # a manual exposure: 2^1.5 as a float, no histogram
    e = f32(2.0 ** 1.5)
    assert js["tonemap"] == "aces" and f32(js["exposure"]) == e and js["luminance_counted"] == 0 and 0.0 < js["tonemap_ms"] < 1000.0
    assert np.array_equal(ppm(out), N.quantise(N.apply(got, N.ACES, e, 1.0)))


@pytest.mark.gpu
def test_automatic_exposure_and_reinhard_equal_the_restatement(hip, tmp_path):
    pfm = tmp_path / "r.pfm"
    out, js = cli(tmp_path, "auto", "--radiance", str(pfm), "--exposure", "auto", "--tonemap", "reinhard")
    rad = abi.read_pfm(pfm, any_value=True)
    exp_rad, exp_rgb, ch = N.tonemap(rad, N.REINHARD, exposure=0.0, white=0.0)
    assert ppm(out).tobytes() == exp_rgb.tobytes()
    assert f32(js["exposure"]) == ch.exposure and f32(js["white"]) == ch.white and js["luminance_counted"] == ch.counted > 0
    assert js["tonemap"] == "reinhard"
    plain, _ = cli(tmp_path, "plain")
    assert not np.array_equal(ppm(plain), ppm(out))
    # a white point and a key of one's own
    out2, js2 = cli(tmp_path, "own", "--exposure", "auto", "--exposure-key", "0.3", "--tonemap", "reinhard", "--white", "4")
    _, exp2, ch2 = N.tonemap(rad, N.REINHARD, exposure=0.0, key=0.3, white=4.0)
    assert ppm(out2).tobytes() == exp2.tobytes() and f32(js2["exposure"]) == ch2.exposure and js2["white"] == 4.0


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_write_the_same_bytes(hip, tmp_path):
    args = ("--exposure", "auto", "--tonemap", "aces")
    one, js1 = cli(tmp_path, "one", *args, "--radiance", str(tmp_path / "one.pfm"))
    two, js2 = cli(tmp_path, "two", *args, "--radiance", str(tmp_path / "two.pfm"), "--gpus", "2", "--oversubscribe", "--gather", "host")
    assert js2["gpus"] == 2 and js2["gather"] == "host"
    assert one.read_bytes() == two.read_bytes() and (tmp_path / "one.pfm").read_bytes() == (tmp_path / "two.pfm").read_bytes()
    assert js1["exposure"] == js2["exposure"] and js1["luminance_counted"] == js2["luminance_counted"] > 0
    _, exp_rgb, _ = N.tonemap(abi.read_pfm(tmp_path / "one.pfm", any_value=True), N.ACES, exposure=0.0, white=1.0)
    assert ppm(one).tobytes() == exp_rgb.tobytes()


@pytest.mark.gpu
def test_the_noisy_file_gets_the_target_files_exposure_and_white(hip, tmp_path):
    import torch
    pfm, noisy = tmp_path / "r.pfm", tmp_path / "noisy.ppm"
    out, js = cli(tmp_path, "dn", "--denoise", "--denoise-radius", "3", "--denoise-patch", "2", "--noisy", str(noisy), "--radiance", str(pfm),
                  "--exposure", "auto", "--tonemap", "reinhard")
    filtered = abi.read_pfm(pfm, any_value=True)
    ch = N.choose(filtered, exposure=0.0, white=0.0)  # chosen on the target image, the filtered one
    assert f32(js["exposure"]) == ch.exposure and f32(js["white"]) == ch.white
    assert ppm(out).tobytes() == N.quantise(N.apply(filtered, N.REINHARD, ch.exposure, ch.white)).tobytes()
    # the unfiltered radiance: --denoise without --adaptive is the fixed render
    hsn = abi.HostScene(SCENE, H, W)
    o = abi.default_opts(spp=SPP, seed=3, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
    rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    with hip.HipScene(hsn) as hs:
        hs.render_device(hsn.camera, o, rad.data_ptr(), lens=hsn.lens)
        torch.cuda.synchronize()
        hs.check()
    unfiltered = rad.cpu().numpy()
    assert not np.array_equal(bits(unfiltered), bits(filtered))
    assert ppm(noisy).tobytes() == N.quantise(N.apply(unfiltered, N.REINHARD, ch.exposure, ch.white)).tobytes()
