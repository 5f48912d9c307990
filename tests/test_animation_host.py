"""The animation in the C++ host, without a GPU: --motion-step's refusals, the shipped scene, and the documents that describe the
flag (the --help text is a recorded yardstick and stays as it is). What needs a render -- the report's motion_step, the frames,
PREFIX.motion.pfm -- is in test_animation_gpu.py."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
CFG = ROOT / "scenes" / "motion" / "animated_spheres.yaml"
f32 = np.float32


def refused(*args):
    r = subprocess.run([str(EXE), "-c", str(CFG), "-t", "unused.png", *args], capture_output=True, text=True)
    assert r.returncode == 2, (args, r.returncode, r.stderr[-500:])
    return r.stderr


def test_motion_step_needs_frames():
    err = refused("--motion-step", "1")
    assert "'--motion-step' needs '--frames'" in err
    assert "'--motion-step' needs '--frames'" in refused("--motion-step", "0")  # (a step of 0 is still the flag)
    assert "'--motion-step' needs '--frames'" in refused("--motion-step", "1", "--no-motion")


@pytest.mark.parametrize("value", ["nan", "inf", "-inf", "x", "1,2,3", ""])
def test_motion_step_takes_a_finite_number(value):
    err = refused("--frames", "3", f"--motion-step={value}")
    assert "--motion-step" in err and "a finite number" in err


def test_motion_step_needs_its_value_and_a_finite_last_phase():
    assert "a value is required for '--motion-step'" in refused("--frames", "3", "--motion-step")
    assert "is not finite" in refused("--frames", "3", "--motion-step", "3e38")  # float(2) * 3e38
    # --frames keeps its own conflicts with the flag beside it
    assert "--frames" in refused("--frames", "3", "--motion-step", "1", "--gpus", "2")


def test_the_shipped_scene():
    hs = abi.HostScene(CFG, 24, 32)
    assert hs.shutter_travel is None and hs.motion is not None  # a static camera, moving spheres
    moving = np.nonzero(hs.motion.any(axis=1))[0]
    assert len(moving) >= 2 and not hs.motion[0].any()  # (the ground stays)
    text = CFG.read_text()
    assert "--motion-step" in text and "--frames" in text


def test_the_documents_describe_the_flag():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert "--motion-step" in text and "rbrt_hip_temporal_accumulate_moving" in text, doc
