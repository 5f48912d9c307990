"""The C++ host's YAML reader (rbrt_amd/host/yaml_lite.cpp) against PyYAML's composer on the corpus of tests/yaml_cases.py:
agree or refuse, never differ. The texts and PyYAML's trees are read from tests/golden/yaml_corpus.json, so that nothing
here needs PyYAML; where it is installed the corpus is generated again and must equal the fixture. The reader's tree comes
through the test hook rbrt_host_yaml_dump. Also: one scene written in many styles loads to the same bytes."""
import ctypes as C
import hashlib
import json
import re
from pathlib import Path

import numpy as np
import pytest

import yaml_cases
from rbrt_amd import abi, standin

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "yaml_corpus.json"
LINE_NO = re.compile(r"^yaml: line [1-9][0-9]*: \S")


@pytest.fixture(scope="module")
def corpus():
    return json.loads(FIXTURE.read_text())["cases"]


def read(text):
    """("tree", tree) or ("refused", message) from the reader under test."""
    try:
        return "tree", json.loads(abi.yaml_dump(text))
    except RuntimeError as e:
        return "refused", str(e)


def duplicate_keys(tree) -> bool:
    """PyYAML's composer keeps both pairs of a duplicated key, and so would a dump: which of the two a lookup answers is
    what differs (YAML: an error, or the last; a first-match lookup: the first). Accepting such a text is a difference."""
    if not isinstance(tree, dict) or "s" in tree:
        return False
    if "map" in tree:
        keys = [k for k, _ in tree["map"]]
        return len(set(keys)) != len(keys) or any(duplicate_keys(v) for _, v in tree["map"])
    return any(duplicate_keys(v) for v in tree.get("list", tree.get("documents", [])))


def of_class(corpus, cls):
    cases = [c for c in corpus if c["cls"] == cls]
    assert cases
    return cases


def test_fixture_is_current(record_property):
    """Where PyYAML is installed: the generator and PyYAML give exactly the committed fixture."""
    try:
        import yaml  # noqa: F401
    except ImportError:
        record_property("pyyaml", "not installed: the fixture was not regenerated")
        assert FIXTURE.stat().st_size > 1000
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_yaml_corpus", ROOT / "tests" / "golden" / "make_yaml_corpus.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    assert mk.dumps(yaml_cases.corpus()) == FIXTURE.read_text(), "run tests/golden/make_yaml_corpus.py"
    assert FIXTURE.stat().st_size <= 281 * 1024  # (no larger than the largest golden before it)


def test_in_subset_texts_are_accepted_and_equal(corpus):
    """Every text built from the documented subset: accepted, and the same tree as PyYAML's. No refusal, no difference."""
    wrong = []
    for c in of_class(corpus, "in"):
        assert "tree" in c["expect"], c["id"]  # the generator defines the class: PyYAML accepts all of it
        kind, got = read(c["text"])
        if kind != "tree":
            wrong.append(f"{c['id']}: refused: {got}")
        elif got != c["expect"]["tree"]:
            wrong.append(f"{c['id']}: differs: {c['text']!r} -> {got} != {c['expect']['tree']}")
    assert not wrong, f"{len(wrong)} of the in-subset texts:\n" + "\n".join(wrong[:40])


def test_valid_yaml_outside_the_subset_is_equal_or_refused(corpus, record_property):
    """Valid YAML beyond the subset: the same tree, or a refusal that names a line. Never another tree."""
    wrong, equal, refused = [], 0, 0
    for c in of_class(corpus, "outside"):
        assert "tree" in c["expect"], c["id"]
        kind, got = read(c["text"])
        if kind == "refused":
            refused += 1
            if not LINE_NO.match(got):
                wrong.append(f"{c['id']}: refused without a line number: {got}")
        elif got == c["expect"]["tree"] and not duplicate_keys(got):
            equal += 1
        else:
            wrong.append(f"{c['id']}: accepted and different: {c['text']!r} -> {got} != {c['expect']['tree']}")
    record_property("outside_subset_refused", refused)
    record_property("outside_subset_equal", equal)
    print(f"outside the subset: {refused} refused, {equal} equal")
    assert not wrong, f"{len(wrong)} of the texts outside the subset:\n" + "\n".join(wrong[:40])


def test_malformed_table_is_refused(corpus):
    wrong = []
    for c in of_class(corpus, "bad-table"):
        kind, got = read(c["text"])
        if kind != "refused":
            wrong.append(f"{c['id']} ({c['why']}): accepted {c['text']!r} -> {got}")
        elif not LINE_NO.match(got):
            wrong.append(f"{c['id']}: refused without a line number: {got}")
    assert {"bad/table/value-in-value", "bad/table/seq-in-value", "bad/table/open-flow-seq", "bad/table/bad-indent-less",
            "bad/table/tab-indent"} <= {c["id"] for c in of_class(corpus, "bad-table")}
    assert not wrong, f"{len(wrong)} malformed texts:\n" + "\n".join(wrong)


def test_mutated_texts_do_not_crash_and_never_differ(corpus, record_property):
    """Truncations and character replacements of in-subset texts: the reader returns (it runs in this process); where both
    it and PyYAML accept the text the trees are equal. How many it accepts although PyYAML refuses is recorded, not asserted:
    PyYAML is stricter than YAML 1.2 in places (a tab as separation, `a:<TAB>1`)."""
    wrong, lenient, accepted, refused = [], [], 0, 0
    for c in of_class(corpus, "bad-mutation"):
        kind, got = read(c["text"])
        if kind == "refused":
            refused += 1
            if not LINE_NO.match(got):
                wrong.append(f"{c['id']}: refused without a line number: {got}")
            continue
        accepted += 1
        if "error" in c["expect"]:
            lenient.append(c["id"])
        elif got != c["expect"]["tree"] or duplicate_keys(got):
            wrong.append(f"{c['id']}: accepted and different: {c['text']!r} -> {got} != {c['expect']['tree']}")
    record_property("mutations_refused", refused)
    record_property("mutations_accepted", accepted)
    record_property("mutations_accepted_although_pyyaml_refuses", len(lenient))
    print(f"mutations: {refused} refused, {accepted} accepted, {len(lenient)} of them although PyYAML refuses: {lenient}")
    assert not wrong, f"{len(wrong)} mutated texts:\n" + "\n".join(wrong[:40])


def test_the_hook_reports_refusals_and_keeps_pairs():
    assert json.loads(abi.yaml_dump("b: 1\na: ['x', ~]\n")) == {"map": [["b", {"s": "1", "q": False}], ["a", {"list": [
        {"s": "x", "q": True}, {"s": "~", "q": False}]}]]}
    assert json.loads(abi.yaml_dump("# nothing\n")) is None
    assert json.loads(abi.yaml_dump(b'a: "\\0\\x01\\u00e9"')) == {"map": [["a", {"s": "\x00\x01é", "q": True}]]}
    # a tab separates as a blank does (YAML 1.2, 6.2 separation spaces; PyYAML refuses it, so the corpus cannot hold it):
    # `a:<TAB>1` is a pair, not the one string `a:<TAB>1`
    assert json.loads(abi.yaml_dump("a:\t1\nb: 2\t# c\n")) == {"map": [["a", {"s": "1", "q": False}], ["b", {"s": "2", "q": False}]]}
    with pytest.raises(RuntimeError, match=r"yaml: line 2: duplicate key `a` \(first on line 1\)"):
        abi.yaml_dump("a: 1\na: 2\n")
    with pytest.raises(RuntimeError, match="line 3: a second document"):
        abi.yaml_dump("---\na: 1\n---\nb: 2\n")
    for text, name in (("a: &x 1", "anchors"), ("a: *x", "aliases"), ("a: !!str 1", "tags"), ("a: |\n  x", "block scalars"),
                       ("a: >\n  x", "block scalars"), ("? a", "complex keys"), ("%YAML 1.2\n---\na: 1", "directives"), ("a: @x", "reserved")):
        with pytest.raises(RuntimeError, match=name):
            abi.yaml_dump(text)


# ---- one scene, many spellings ---------------------------------------------------------------------------------------------------
def scene_bytes(hs) -> bytes:
    """Everything the kernel is given from a loaded scene, as bytes: camera, lens, spheres, and every mesh array."""
    out = [bytes(hs.camera), bytes(hs.lens) if hs.lens is not None else b"pinhole"]
    out.append(C.string_at(hs.struct.spheres, hs.struct.n_spheres * C.sizeof(abi.Sphere)) if hs.struct.n_spheres else b"")
    for i in range(hs.struct.n_meshes):
        arrays = hs.mesh_arrays(i)
        for k in sorted(arrays):
            out.append(k.encode() + np.asarray(arrays[k]).tobytes())
        out.append(bytes(hs.struct.meshes[i].mat))
    return b"|".join(out)


def test_one_scene_in_many_styles_loads_to_the_same_bytes(tmp_path):
    """Key order, block against flow, the three quoting styles, comments and blank lines, LF against CRLF, indentation of 1
    to 8: whatever the spelling, rbrt_host_scene_load gives byte-identical camera, lens, spheres, materials and mesh arrays."""
    scene = yaml_cases.feature_scene(tmp_path)
    texts = {yaml_cases.spell_scene(scene, seed) for seed in range(60)}
    assert len(texts) >= 55
    assert any("\r\n" in t for t in texts) and any("{" in t for t in texts) and any("'" in t for t in texts)
    digests = set()
    for k, text in enumerate(sorted(texts)):
        (tmp_path / f"s{k}.yaml").write_bytes(text.encode())
        hs = abi.HostScene(tmp_path / f"s{k}.yaml", 30, 44)
        assert hs.struct.n_spheres == 5 and hs.struct.n_meshes == 2 and hs.lens is not None and hs.shading is not None
        digests.add(hashlib.sha256(scene_bytes(hs)).hexdigest())
        hs.close()
    assert len(digests) == 1


# ---- the scenes that loaded before the reader was made stricter still load to the same bytes -----------------------------------------
def known_scene_texts(tmp_path):
    """name -> YAML text: the shipped scenes/*.yaml and the YAML texts the other tests hold, on a 64-triangle stand-in mesh."""
    import test_emissive_host
    import test_host
    import test_scene_numbers
    import test_smooth_shading
    import test_smooth_shading_host
    import test_thin_lens_host
    v, f = standin.make_mesh(64)
    obj = tmp_path / "bunny.obj"
    standin.write_obj(obj, v, f)
    texts = {p.name: p.read_text().replace("bunny.obj", str(obj)) for p in sorted((ROOT / "scenes").glob("*.yaml"))}
    assert len(texts) == 5
    texts["test_host.YAML_MIN"] = test_host.YAML_MIN
    texts["test_host.YAML_MIN+mesh"] = test_host.YAML_MIN.replace(
        "mesh_blueprints: []", f"mesh_blueprints:\n  - obj_filepath: {obj}\n    scale: 2.0\n"
        "    translation: {x: 1, y: 2, z: 3}\n    rotation_rad: {x: 0.1, y: 0.2, z: 0.3}\n"
        "    material_type: lambertian\n    albedo: {x: 1, y: 1, z: 1}")
    texts["test_emissive_host.YAML"] = test_emissive_host.YAML
    texts["test_thin_lens_host.CAMERA_YAML"] = test_thin_lens_host.CAMERA_YAML.format(extra="")
    texts["test_thin_lens_host.CAMERA_YAML+lens"] = test_thin_lens_host.CAMERA_YAML.format(
        extra="  camera_aperture_mm: 7.0\n  camera_focus_distance: 10.0\n")
    for sh in ("", "    shading: flat\n", "    shading: smooth\n"):
        texts[f"test_smooth_shading_host.YAML{sh.strip()}"] = test_smooth_shading_host.YAML.format(
            obj=obj, scale=1.5, rx=0.3, ry=-0.7, rz=1.1, shading=sh)
        texts[f"test_smooth_shading.CLI_YAML{sh.strip()}"] = test_smooth_shading.CLI_YAML.format(obj=obj, shading=sh)
    texts["test_scene_numbers.SCENE"] = test_scene_numbers.SCENE.format(probe="0.5")
    return texts


# SHA-256 of scene_bytes() of each, recorded from the reader as it was before it refused anything it used to accept
PINNED = {
    "defocus_spheres.yaml": "2e10bc38e20cb5c0fdf859f0ab48599cc791992f55d8d4d5c669eb0f51b89533",
    "emissive_spheres.yaml": "63cabcb6c28b10610ff356b2b6bd1543f9c8356bf89619ed065422ad13133254",
    "example_scene.yaml": "94206f0294d8c5589dd7fd8115a6eeef525c7253df5371d2ab03b11e142bb410",
    "header_card.yaml": "74af84042315dba2b7abd412cd2b5bc8b12a4b1de91a92112d45938937bd7680",
    "smooth_mesh.yaml": "30878a9c38f4ddc38a1b8f3c998a333fdfd758089ec7fd05fc5acfc3aa8272dc",
    "test_host.YAML_MIN": "464c534f9fc83fef844c503fbc33fbd3080005ca0059112c219676c19389da0a",
    "test_host.YAML_MIN+mesh": "37f51d8155ba80a1563d43b01b35195214231153920409cc079760be375cc53e",
    "test_emissive_host.YAML": "4ad5081a53f81183fd6d219069f1635a88359346b88af293d9a0de8bf5af087c",
    "test_thin_lens_host.CAMERA_YAML": "b5010f8b9b9dfcaef2e12f72cb5d2c31f55661418d98078152e365287460dc2a",
    "test_thin_lens_host.CAMERA_YAML+lens": "4981728ea29d54c003f78330fff071b2d46528e5a508690d6eb18fbc7aacf1f8",
    "test_smooth_shading_host.YAML": "194d778d81d75eb8fb77d463d43e16e3e3d06aa0e904620b4fc0470c9cf9c9fc",
    "test_smooth_shading.CLI_YAML": "6d0ea7d68c469d80de7d6ed389ee41c03c4b14f77bc9e4983d5670df60d7bb58",
    "test_smooth_shading_host.YAMLshading: flat": "194d778d81d75eb8fb77d463d43e16e3e3d06aa0e904620b4fc0470c9cf9c9fc",
    "test_smooth_shading.CLI_YAMLshading: flat": "6d0ea7d68c469d80de7d6ed389ee41c03c4b14f77bc9e4983d5670df60d7bb58",
    "test_smooth_shading_host.YAMLshading: smooth": "8b10200d48d3bfff8492a88194569b2a2036937c4d9a1f8e5c4b0a684aee97eb",
    "test_smooth_shading.CLI_YAMLshading: smooth": "827c35c38623185f20034d2909149e9af0b031ca6715bb4f04eeb7d8ba17e958",
    "test_scene_numbers.SCENE": "0ff30b99e5d86b485a9014b89dc3255080098ad5242a9bc44178556e662bfbb8",
}


def test_known_scenes_load_to_the_bytes_they_loaded_to_before(tmp_path):
    got = {}
    for name, text in known_scene_texts(tmp_path).items():
        (tmp_path / "scene.yaml").write_text(text)
        hs = abi.HostScene(tmp_path / "scene.yaml", 30, 44)
        got[name] = hashlib.sha256(scene_bytes(hs)).hexdigest()
        hs.close()
    assert got == PINNED


# ---- the readers still feed the kernel what the oracle expects (GPU) -------------------------------------------------------------------
@pytest.mark.gpu
def test_styles_of_one_scene_render_to_the_oracles_image(hip, oracle, tmp_path):
    """A scene with an emitter, a constant background, a thin lens, a flat and a smooth mesh below a folder with an
    apostrophe in its name, written in six styles: the `rbrt` CLI renders every one to the same PNG bytes, and the
    pixels are the oracle's for the scene prepared without any YAML."""
    import subprocess

    from PIL import Image

    import np_lens
    import np_smooth
    import scenes
    n_flat, n_smooth, w, h, spp, seed, bg = 300, 500, 88, 60, 5, 7, (0.02, 0.03, 0.05)
    scene = yaml_cases.feature_scene(tmp_path, n_flat, n_smooth)
    exe = ROOT / "rbrt_amd" / "bin" / "rbrt"
    pngs = []
    texts = []
    for style in (0, 3, 7, 12, 21, 33):
        text = yaml_cases.spell_scene(scene, style)
        texts.append(text)
        cfg, out = tmp_path / f"style{style}.yaml", tmp_path / f"style{style}.png"
        cfg.write_bytes(text.encode())
        r = subprocess.run([str(exe), "-c", str(cfg), "-t", str(out), "--height", str(h), "-w", str(w), "-s", str(spp), "--seed", str(seed),
                            "--background", ",".join(str(c) for c in bg)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        pngs.append(out.read_bytes())
    assert len(set(texts)) == len(texts) and any("{" in t for t in texts) and any("\r\n" in t for t in texts)
    assert len(set(pngs)) == 1
    xyz = lambda d: (d["x"], d["y"], d["z"])  # noqa: E731
    c = scene["camera_blueprint"]
    cam = scenes.camera(oracle, w, h, position=xyz(c["camera_position"]), look_at=xyz(c["camera_look_at"]), up=xyz(c["camera_up"]),
                        focal_mm=c["camera_focal_length_mm"])
    lens = np_lens.lens_for(cam, xyz(c["camera_look_at"]), c["camera_focal_length_mm"], c["camera_aperture_mm"], c["camera_focus_distance"])
    kinds = (("metal", abi.MAT_METAL), ("lambert", abi.MAT_LAMBERTIAN), ("dielectric", abi.MAT_DIELECTRIC), ("emissive", abi.MAT_EMISSIVE))

    def mat(b):
        kind = next(k for name, k in kinds if name in b["material_type"].lower())
        return abi.material(kind, xyz(b["albedo"]) if "albedo" in b else (0.0, 0.0, 0.0), b.get("material_param", 0.0))
    flat, smooth = scene["mesh_blueprints"]
    meshes = [scenes.standin_mesh(oracle, n_flat, flat["scale"], xyz(flat["translation"]), (0.0, 0.0, 0.0), mat(flat)),
              np_smooth.standin_smooth(oracle, n_smooth, smooth["scale"], xyz(smooth["translation"]), mat(smooth), "computed")]
    sc = abi.SceneData(spheres=[(xyz(s["center"]), s["radius"], mat(s)) for s in scene["sphere_blueprints"]], meshes=meshes)
    opts = abi.default_opts(spp=spp, seed=seed, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=bg)
    exp, exp8, _ = oracle.render(cam, sc, opts, lens=lens)
    assert (exp > 1.0).any()  # (the emitter is in view)
    got = np.array(Image.open(tmp_path / "style0.png"))
    assert got.shape == exp8.shape and np.array_equal(got, exp8)
