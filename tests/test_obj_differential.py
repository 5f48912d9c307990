"""The C++ host's .obj loader against tests/np_obj.py, a plain Python restatement of what it is documented to do, on .obj
texts generated from a seed: HostScene.mesh_arrays == oracle.mesh_prep of the restatement's triangles, bit for bit, flat and
smooth; and a table of texts the loader must refuse with file:line."""
import random

import numpy as np
import pytest

import np_obj
import np_smooth
import test_smooth_shading_host as S
from rbrt_amd import abi

f32 = np.float32
SCALE, ROT, TRANS = 1.5, (0.3, -0.7, 1.1), (0.5, -1.0, -9.0)  # (what test_smooth_shading_host's YAML template holds)
N_SEEDS = 40


def number(r: random.Random) -> str:
    x = r.uniform(-2.0, 2.0)
    return r.choice([f"{x:.9g}", f"{x:.3f}", f"{x:.17g}", f"{x:.4e}", f"{x:.2E}", f"+{abs(x):.5g}", f"{int(x * 3)}", f"{int(x * 3)}.",
                     f"{abs(x) % 1:.3f}"[1:], f"{x:.6g}"])


def obj_text(seed: int, refuse: str | None = None):
    """An .obj text from a seed: vertices, normals and faces interleaved, every corner form, polygons of 3 to 6 corners,
    positive and negative indices, group lines, comments, blanks and tabs, LF or CRLF. `refuse` plants one statement that
    must be refused and returns its line number too."""
    r = random.Random(seed)
    sep = lambda: r.choice([" ", " ", "  ", "\t", " \t "])  # noqa: E731
    lines, n_v, n_vn, n_vt = [], 0, 0, 0

    def emit(toks):
        lines.append(r.choice(["", "", " ", "\t", "   "]) + sep().join(toks) + r.choice(["", "", " ", "\t"]))

    def vertex():
        nonlocal n_v
        extra = r.choice([0, 0, 0, 1, 3])  # (a w, or a colour)
        emit(["v"] + [number(r) for _ in range(3 + extra)])
        n_v += 1

    def corner():
        v = r.randint(1, n_v)
        v = v if r.random() < 0.6 else v - n_v - 1
        form = r.choice(["v", "v/vt", "v//vn", "v/vt/vn"])
        vt = str(r.randint(1, max(1, n_vt))) if r.random() < 0.8 else str(-r.randint(1, max(1, n_vt)))
        vn = r.randint(1, max(1, n_vn))
        vn = str(r.choice([vn, vn, vn, -r.randint(1, max(1, n_vn)), 0, n_vn + 1 + r.randint(0, 3), -n_vn - 1]))
        return {"v": f"{v}", "v/vt": f"{v}/{vt}", "v//vn": f"{v}//{vn}", "v/vt/vn": f"{v}/{vt}/{vn}"}[form]

    all_vn = r.random() < 0.4  # every corner names a valid vn: the file's normals are used
    for _ in range(r.randint(3, 5)):
        vertex()
    for _ in range(r.randint(12, 30)):
        k = r.random()
        if k < 0.25:
            vertex()
        elif k < 0.35:
            emit(["vn"] + r.choice([[number(r) for _ in range(3)]] * 4 + [["a", "0", "1"], ["0", "nan", "0"], ["1", "2"], ["inf", "0", "0"]]))
            n_vn += 1
        elif k < 0.4:
            emit(["vt", number(r), number(r)])
            n_vt += 1
        elif k < 0.5:
            emit(r.choice([["o", "thing"], ["g"], ["g", "a", "b"], ["o"], ["usemtl", "m1"], ["g", "again"]]))
            if r.random() < 0.3:
                emit(r.choice([["g"], ["o", "twice"]]))
        elif k < 0.58:
            lines.append(r.choice(["# a comment", "", "   ", "s off", "mtllib x.mtl", "\t# indented comment", "l 1 2", "vp 0.1 0.2"]))
        else:
            n = r.randint(3, 6)
            if all_vn and n_vn:
                emit(["f"] + [f"{r.randint(1, n_v)}//{r.randint(1, n_vn)}" for _ in range(n)])
            else:
                emit(["f"] + [corner() for _ in range(n)])
    emit(["f", "1", "2", "3"] if not (all_vn and n_vn) else ["f", "1//1", "2//1", "3//1"])  # (at least one triangle)
    lines.append("# the end")
    bad_line = None
    if refuse:
        stmt = {"later-vertex": f"f 1 2 {n_v + 1}", "zero": "f 1 0 2", "negative-too-far": f"f 1 2 {-n_v - 1}", "junk": "f 1 2abc 3",
                "junk-vn": "f 1//1x 2 3", "four-parts": "f 1/1/1/1 2 3", "word": "f 1 2 x", "float": "f 1 2 3.0", "two-numbers": "v 1 2",
                "vertex-junk": "v 1 2 3abc", "two-points": "v 1.0.0 2 3", "hex": "v 0x10 0 0", "comma": "v 1,5 0 0",
                "lone-sign": "v + 0 0", "double-sign": "v +-1 0 0", "empty-v": "f /1 2 3"}[refuse]
        bad_line = r.randint(n_v and 6, len(lines))
        lines.insert(bad_line, stmt)
        lines.append("v 9 9 9")  # (the vertex that `later-vertex` names, defined too late)
        bad_line += 1
    nl = "\r\n" if r.random() < 0.3 else "\n"
    return nl.join(lines) + (nl if r.random() < 0.8 else ""), bad_line


def expected_corner_normals(pos, nrm, models):
    out = []
    sign = f32(1.0 if SCALE > 0 else -1.0)
    for faces, nidx in models:
        if len(faces) == 0:
            continue
        if (nidx >= 0).all():
            out.append(np.stack([np.stack([S.rotate_point(sign * nrm[i], ROT) for i in tri]) for tri in nidx]))
        else:
            tv = np.stack([np.stack([S.transform(pos[i], SCALE, ROT, TRANS) for i in f]) for f in faces])
            out.append(np_smooth.area_weighted(tv, faces))
    return np.concatenate(out)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_generated_obj_files_load_as_the_restatement_says(oracle, tmp_path, seed):
    text, _ = obj_text(seed)
    pos, nrm, models = np_obj.load(text)
    tris = np.concatenate([pos[f] for f, _ in models if len(f)])
    n = len(tris)
    obj = tmp_path / "m.obj"
    obj.write_bytes(text.encode())
    exp = oracle.mesh_prep(tris, SCALE, ROT, TRANS)
    for shading in (None, "smooth"):
        hs = abi.HostScene(S._yaml(tmp_path, f"s{shading}", obj, shading, scale=SCALE, rot=ROT), 24, 32)
        got = hs.mesh_arrays(0)
        assert got["n_real"] == n and len(got["is_padding"]) == n + n % 8
        for k in abi.MeshData.FIELDS:
            assert np.array_equal(got[k].view(np.uint32), exp.arrays[k].view(np.uint32)), (k, text)
        assert np.array_equal(got["is_padding"], exp.is_padding)
        assert np.array_equal(got["bbox_lo"], exp.bbox_lo) and np.array_equal(got["bbox_hi"], exp.bbox_hi)
        if shading:
            cn = expected_corner_normals(pos, nrm, models)
            cn = np.concatenate([cn, np.repeat(cn[:1], n % 8, 0)])
            assert np.array_equal(S.corners(got).view(np.uint32), cn.view(np.uint32)), text
        else:
            assert "n0x" not in got
        hs.close()


def test_the_generator_reaches_every_form():
    texts = [obj_text(s)[0] for s in range(N_SEEDS)]
    both = "\n".join(texts)
    loaded = [np_obj.load(t) for t in texts]
    assert any("\r\n" in t for t in texts) and any("\r" not in t for t in texts) and "\t" in both
    assert any(len(m) > 2 for _, _, m in loaded)                                        # several models
    assert any((ni >= 0).all() and len(f) for _, _, m in loaded for f, ni in m)         # file normals
    assert any((ni >= 0).any() and not (ni >= 0).all() for _, _, m in loaded for f, ni in m)  # vn on some corners only
    assert any((f[1:, 0] != f[:-1, 0]).any() for _, _, m in loaded for f, _ in m if len(f) > 1)
    for form in ("//", "e-0", "E", "+"):
        assert form in both
    assert any(len(line.split()) in (5, 7) for t in texts for line in t.splitlines() if line.split()[:1] == ["v"])  # w, colours


REFUSED = ["later-vertex", "zero", "negative-too-far", "junk", "junk-vn", "four-parts", "word", "float", "two-numbers", "vertex-junk",
           "two-points", "hex", "comma", "lone-sign", "double-sign", "empty-v"]


@pytest.mark.parametrize("what", REFUSED)
def test_bad_statements_are_refused_with_file_and_line(tmp_path, what):
    """A face that names a vertex defined later, the index 0, an index past either end, a token with other text in it
    (`2abc` was once read as `2`), a vertex of two numbers or of something Rust's parse::<f32> does not read."""
    for seed in (100, 101, 102):
        text, line = obj_text(seed, refuse=what)
        with pytest.raises(np_obj.ObjRefused) as e:
            np_obj.load(text)
        assert e.value.line == line
        obj = tmp_path / f"bad{seed}.obj"
        obj.write_bytes(text.encode())
        with pytest.raises(RuntimeError) as e:
            abi.HostScene(S._yaml(tmp_path, f"bad{seed}", obj), 24, 32)
        assert f"{obj}:{line}: " in str(e.value), (what, str(e.value))


def test_numbers_of_a_vertex_are_rounded_once(oracle, tmp_path):
    """Decimal strings at float32 rounding boundaries, where rounding to double first gives the neighbour."""
    toks = ["1.00000005960464477539062500001", "1.0000000596046447753906250", "1.00000017881393432617187499999", "16777217", "16777219",
            "1e-45", "7.1e-46", "7e-46", "3.4028235677973366e38", "3.40282357e38", "1e39", "-1e-50", "0.1", "1.17549435e-38",
            "8.5e-46", "4.9e-324", "inf", "-Infinity", "1e999", "0.000000000000000000000000000000000000000000001"]
    rng = random.Random(5)
    toks += [f"{rng.uniform(-3, 3):.{rng.randint(1, 25)}f}" for _ in range(200)]
    toks += [f"{(1 + k * 2 ** -24 + rng.choice([-1, 0, 1]) * 2 ** -70) * 2 ** rng.randint(-30, 30):.60g}" for k in range(1, 60, 2)]
    while len(toks) % 3:
        toks.append("0")
    text = "".join(f"v {a} {b} {c}\n" for a, b, c in zip(toks[0::3], toks[1::3], toks[2::3]))
    text += "".join(f"f {3 * k + 1} {3 * k + 2} {3 * k + 3}\n" for k in range(len(toks) // 9))
    pos, _, models = np_obj.load(text)
    assert np.array_equal(pos.reshape(-1).view(np.uint32), np.array([np_obj.parse_f32(t) for t in toks], f32).view(np.uint32))
    (tmp_path / "n.obj").write_text(text)
    hs = abi.HostScene(S._yaml(tmp_path, "n", tmp_path / "n.obj", scale=1.0, rot=(0.0, 0.0, 0.0)), 24, 32)
    got = hs.mesh_arrays(0)
    exp = oracle.mesh_prep(pos[models[0][0]], 1.0, (0.0, 0.0, 0.0), TRANS)
    with np.errstate(all="ignore"):
        for k in ("v0x", "v0y", "v0z", "e1x", "e2z"):
            assert np.array_equal(got[k].view(np.uint32), exp.arrays[k].view(np.uint32)), k
