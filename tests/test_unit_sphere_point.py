"""random_point_in_unit_sphere (rbrt_amd/csrc/kernels.hip; materials.rs:14-30) computes a component of its candidate point
with ONE fused multiply-add, fma(float(k), 2^-23, -1), where the reference computes 2.0 * (float(k) * 2^-24) - 1.0 in three
rounded float operations, k = the 24 random bits of the draw. Both are the exact number (k - 2^23) * 2^-23, so they are the
same float for every k: checked here over all 2^24 values, without a GPU. The scatter-event and image parity tests cover the
device side."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def test_one_fma_equals_the_reference_form_for_every_draw():
    k = np.arange(1 << 24, dtype=np.uint32)
    kf = k.astype(np.float32)
    assert np.array_equal(kf.astype(np.uint32), k)  # float(k) is exact below 2^24
    # the reference's form, every step rounded to float32 (rand's Standard f32, then materials.rs:22)
    x = kf * np.float32(1.0 / 16777216.0)
    assert x.dtype == np.float32
    two_x = np.float32(2.0) * x
    ref = two_x - np.float32(1.0)
    assert two_x.dtype == np.float32 and ref.dtype == np.float32
    # the fused form: the product and the sum in one rounding -- float64 holds k * 2^-23 - 1 exactly (25 bits)
    exact = k.astype(np.float64) * 2.0 ** -23 - 1.0
    fused = exact.astype(np.float32)
    assert np.array_equal(fused.astype(np.float64), exact)  # nothing was rounded: the exact value is a float32
    assert np.array_equal(ref.view(np.uint32), fused.view(np.uint32))  # bit for bit, the sign of zero included
    assert ref.min() == -1.0 and ref.max() < 1.0 and ref[1 << 23] == 0.0 and not np.signbit(ref[1 << 23])


def test_the_kernel_source_uses_that_form_in_this_function_only():
    text = (ROOT / "rbrt_amd" / "csrc" / "kernels.hip").read_text()
    body = text[text.index("V3 random_point_in_unit_sphere(Rng& rng)"):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"__builtin_fmaf\(float\(rng\.next_u32\(\) >> 8\), 0x1p-23f, -1\.0f\)", body)
    assert "s > 1.00000011920928955078125f" in body  # the accept / reject test is what it was
    nxt = text[text.index("float next_f32()"):]
    assert "float(next_u32() >> 8) * (1.0f / 16777216.0f)" in nxt[:nxt.index("}")]  # next_f32 itself is untouched
