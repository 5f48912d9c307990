"""A seeded generator of YAML texts for the differential test of the C++ host's reader (rbrt_amd/host/yaml_lite.cpp).

Every case carries one of three classes:

  in       built only from what yaml_lite.hpp says it reads: the reader must accept it and build PyYAML's tree
  outside  valid YAML outside the subset: the reader may build PyYAML's tree or refuse with a line number, never differ
  bad      malformed: a hand-curated table the reader must refuse (TABLE_BAD), and random truncations and character
           replacements of `in` texts, which must not crash it

Trees are written the way rbrt_host_yaml_dump writes them: None, {"s": text, "q": quoted}, {"list": [..]},
{"map": [[key, value], ..]} (pairs, so that order and duplicates stay visible). `expected()` builds that from PyYAML's
composer (BaseLoader: every scalar stays a string, so YAML 1.1 against 1.2 typing cannot interfere); only it needs PyYAML,
and only tests/golden/make_yaml_corpus.py and the currency check of tests/test_yaml_differential.py call it.
"""
from __future__ import annotations

import random

N_IN, N_OUTSIDE_CONTEXTS, N_MUTATIONS = 170, 3, 160  # sized so that tests/golden/yaml_corpus.json stays below 281 KB

NUMBERS = ["0", "1", "35", "-1.8", "0.0", "1.0e-1", ".5", "5.", "5e-1", "+1", "-12.5", "1e3", "-.inf", ".inf", ".nan", ".NaN", "2000.0",
           "0.001", "1_000", "-0", "1E+2", "0x10", "1e-45"]
WORDS = ["lambertian", "Shiny METAL thing", "bunny.obj", "/tmp/a b/c.obj", "dielectric", "smooth", "flat", "~", "null", "true", "no",
         "a#b", "x:y", "glass - blue", "http://h/p?q=1&r=2", "C:\\meshes\\bunny.obj", "50%", "é ü", "a.b-c_d", "<<", "=", "1 2 3",
         "x]y", "p{q", "-x", ":z"]
NEEDS_QUOTES = ["", " lead", "trail ", "a: b", "# not a comment", "x #y", "- item", "[1, 2]", "{k: v}", "a, b", "&anchor", "*alias",
                "!tag", "|", ">", "%YAML", "@at", "`tick", "key:", "---", "...", "? q", "tab\there", "two\nlines", "back\\slash\\n",
                ", x", "] x", "} x", ": x", "-", "?", ":"]
WITH_QUOTE_CHARS = ["it's", "say \"hi\"", "the 'quoted' one", "5\" pipe", "l'été"]
COMMENTS = ["# c", "#", "# a: b", "#- x", "# [", "# 'quote", "# \"dq", "#\tx", "# it's # nested", "# }"]
KEYS = ["x", "y", "z", "radius", "center", "material_type", "albedo", "camera_up", "k1", "k 2", "a.b", "obj_filepath", "0", "-k", "é"]

INDICATORS = set("-?:,[]{}#&*!|>'\"%@`")


def plain_ok(s: str, flow: bool) -> bool:
    if not s or s != s.strip() or any(ord(c) < 0x20 for c in s):
        return False
    if s[0] in INDICATORS and not (s[0] in "-?:" and len(s) > 1 and s[1] not in " \t" and not (flow and s[1] in ",[]{}")):
        return False
    if s.startswith(("---", "...")) or ": " in s or " #" in s or s.endswith(":"):
        return False
    if flow:
        if s[0] in "?:":  # (YAML 1.2 admits `:z` there; PyYAML does not)
            return False
        if any(c in s for c in ",[]{}"):
            return False
        if any(c == ":" and not s[i + 1].isalnum() for i, c in enumerate(s[:-1])):
            return False
    return True


class Gen:
    """One in-subset text from one seed: a random tree and a random spelling of it."""

    def __init__(self, seed: int):
        self.r = random.Random(seed)
        self.lines: list[str] = []
        self.plain_quote = False  # the line under construction holds a plain scalar with a quote character in it

    # ---- trees ----
    def scalar(self):
        r = self.r
        pool = r.choice([NUMBERS, NUMBERS, WORDS, WORDS, NEEDS_QUOTES, WITH_QUOTE_CHARS])
        return {"s": r.choice(pool)}

    def tree(self, depth: int):
        r = self.r
        k = r.random()
        if depth <= 0 or k < 0.35:
            return None if r.random() < 0.08 else self.scalar()
        if k < 0.75:
            keys = r.sample(KEYS + NEEDS_QUOTES[:12] + WITH_QUOTE_CHARS[:2], r.randint(0 if depth < 3 else 1, 4))
            return {"map": [[key, self.tree(depth - 1)] for key in keys]}
        return {"list": [self.tree(depth - 1) for _ in range(r.randint(0, 4))]}

    # ---- spellings ----
    def spell(self, s: str, flow: bool, plain: bool = False) -> str:
        """One of the spellings of the scalar that the subset admits (`plain`: a number, which no quotes may surround)."""
        r = self.r
        if plain:
            assert plain_ok(s, flow), s
            return s
        styles = []
        if plain_ok(s, flow):
            styles += ["plain", "plain"]
        if "'" not in s and not any(ord(c) < 0x20 for c in s):
            styles.append("single")
        if '"' not in s:
            styles.append("double")
        if not styles:  # both quote characters: plain was refused only where it had to be
            raise AssertionError(s)
        st = r.choice(styles)
        if st == "plain":
            self.plain_quote = self.plain_quote or "'" in s or '"' in s
            return s
        if st == "single":
            return "'" + s + "'"
        return '"' + s.replace("\\", "\\\\").replace("\n", "\\n").replace("\t", "\\t") + '"'

    def flowable(self, n) -> bool:
        if n is None:
            return False
        if "s" in n:
            return "'" not in n["s"] or '"' not in n["s"] or plain_ok(n["s"], True)
        return all(self.flowable(v) for v in (n["list"] if "list" in n else [v for _, v in n["map"]]))

    def flow(self, n) -> str:
        r = self.r
        sp = lambda: " " * r.choice([0, 0, 1, 1, 2])  # noqa: E731
        if "s" in n:
            return self.spell(n["s"], True, n.get("plain", False))
        if "list" in n:
            return "[" + sp() + ("," + sp() + " ").join(self.flow(v) for v in n["list"]) + sp() + "]"
        return "{" + sp() + ("," + sp() + " ").join(self.spell(k, True) + ":" + " " * r.choice([1, 1, 2]) + self.flow(v)
                                                  for k, v in n["map"]) + sp() + "}"

    def end(self, line: str) -> None:
        r = self.r
        if not self.plain_quote and r.random() < 0.25:
            line += " " * r.randint(1, 3) + r.choice(COMMENTS)
        if r.random() < 0.1:
            line += " " * r.randint(1, 3)
        self.plain_quote = False
        self.lines.append(line)
        if r.random() < 0.12:
            self.lines.append(r.choice(["", "   ", " " * r.randint(0, 9) + r.choice(COMMENTS)]))

    def can_spell(self, n) -> bool:
        """Scalars with both quote characters and no plain spelling cannot be written inside the subset."""
        if n is None:
            return True
        if "s" in n:
            s = n["s"]
            return "'" not in s or '"' not in s or plain_ok(s, True)
        return all(self.can_spell(v) for v in (n["list"] if "list" in n else [v for _, v in n["map"]]))

    def block(self, n, indent: int, width: int, head: str | None = None) -> None:
        """Writes the collection `n` as a block at `indent`; `head` replaces the indentation of its first line (`- `)."""
        r = self.r
        pad = " " * indent
        first = True

        def start() -> str:
            nonlocal first
            p = head if (first and head is not None) else pad
            first = False
            return p
        if "map" in n:
            for k, v in n["map"]:
                line = start() + self.spell(k, False) + " " * r.choice([0, 0, 0, 1]) + ":"
                self.value(line, v, indent, width, in_map=True)
        else:
            for v in n["list"]:
                gap = r.choice([1, 1, 1, 2, 3])
                if v is not None and "s" not in v and (v.get("map") or v.get("list")) and r.random() < 0.7 and (
                        "map" in v or r.random() < 0.5):
                    self.block(v, indent + 1 + gap, width, head=start() + "-" + " " * gap)  # `- key: value` / `- - item`
                else:
                    self.value(start() + "-", v, indent, width, in_map=False)

    def value(self, line: str, v, indent: int, width: int, in_map: bool) -> None:
        r = self.r
        if v is None:
            self.end(line)
        elif "s" in v:
            self.end(line + " " * r.choice([1, 1, 1, 2, 4]) + self.spell(v["s"], False, v.get("plain", False)))
        elif not (v.get("map") or v.get("list")) or (self.flowable(v) and r.random() < 0.4):
            self.end(line + " " + self.flow(v))
        else:
            self.end(line)
            same = in_map and "list" in v and r.random() < 0.3  # a sequence at its parent key's indentation
            self.block(v, indent if same else indent + width, width)

    def text(self) -> str:
        r = self.r
        while True:
            root = self.tree(r.choice([2, 3, 3, 4]))
            if root is not None and "s" not in root and (root.get("map") or root.get("list")) and self.can_spell(root):
                break
        return self.write(root)

    def write(self, root) -> str:
        r = self.r
        if r.random() < 0.25:
            self.lines.append(r.choice(["---", "--- # scene", "# header\n---"]))
        if r.random() < 0.15 and self.flowable(root):
            self.end(self.flow(root))
        else:
            self.block(root, 0, r.randint(1, 8))
        if r.random() < 0.08:
            self.lines.append("...")
        nl = "\r\n" if r.random() < 0.2 else "\n"
        out = nl.join(nl.join(line.split("\n")) for line in self.lines)
        return out + (nl if r.random() < 0.8 else "")


def in_subset_cases():
    fixed = [
        ("in/numbers", "".join(f"n{i}: {s}\n" for i, s in enumerate(NUMBERS)) + "v: [" + ", ".join(NUMBERS) + "]\n"),
        ("in/hash-without-blank", "a#b: c#d\ne: [f#g, h] #i\n"),
        ("in/quoted-keys", "\"a: b\": 1\n'# k': 2\n\"- x\" : 3\n'': 4\n"),
        ("in/dash-map", "- a: 1\n  b: 2\n-   c: 3\n    d:\n    - 4\n    - {e: 5}\n- - 6\n  - 7\n-\n  f: 8\n"),
        ("in/crlf", "a: 1 # c\r\nb:\r\n  - x\r\n  - 'y' \r\n\r\nc: \"z\"\r\n"),
        ("in/document-markers", "# first\n---\na: 1\n...\n"),
        ("in/comment-only", "# nothing\n\n   # here\n"),
        ("in/empty", ""),
        ("in/nested-flow", "a: {b: [1, {c: [2, 3], d: {}}], e: []}\n"),
    ]
    return fixed + [(f"in/seed{seed}", Gen(seed).text()) for seed in range(N_IN)]


# ---- one scene in many spellings (the metamorphic tests) ----------------------------------------------------------------------------
def feature_scene(directory, n_flat: int = 300, n_smooth: int = 500) -> dict:
    """A scene that uses every feature (an emitter, a thin lens, a flat and a smooth mesh, every material kind), as plain
    Python values; writes its two stand-in .obj files below `directory`, in a folder with an apostrophe and blanks in its name."""
    from pathlib import Path

    from rbrt_amd import standin
    d = Path(directory) / "it's a mesh dir"
    d.mkdir(exist_ok=True)
    for n in (n_flat, n_smooth):
        v, f = standin.make_mesh(n)
        standin.write_obj(d / f"bunny {n}.obj", v, f)
    xyz = lambda x, y, z: {"x": x, "y": y, "z": z}  # noqa: E731
    return {
        "camera_blueprint": {"camera_up": xyz(0.0, 1.0, -0.4), "camera_look_at": xyz(0.0, -0.1, -1.0), "camera_position": xyz(0.0, 5.0, 4.0),
                             "camera_focal_length_mm": 28.0, "camera_aperture_mm": 9.0, "camera_focus_distance": 12.5},
        "mesh_blueprints": [
            {"obj_filepath": str(d / f"bunny {n_flat}.obj"), "scale": 30.0, "translation": xyz(-4.0, -1.5, -10.0),
             "rotation_rad": xyz(0.0, 0.0, 0.0), "material_type": "dielectric", "material_param": 1.5},
            {"obj_filepath": str(d / f"bunny {n_smooth}.obj"), "scale": 45.0, "translation": xyz(5.0, -1.8, -12.5),
             "rotation_rad": xyz(0.0, 0.0, 0.0), "material_type": "Shiny METAL thing's", "material_param": 0.01,
             "albedo": xyz(0.9, 0.8, 0.6), "shading": "smooth"}],
        "sphere_blueprints": [
            {"radius": 1000.0, "center": xyz(0.0, -1001.0, -10.0), "material_type": "lambertian", "albedo": xyz(0.5, 0.5, 0.5)},
            {"radius": 1.5, "center": xyz(0.0, 6.0, -11.0), "material_type": "emissive", "albedo": xyz(9.0, 8.0, 6.5)},
            {"radius": 1.25, "center": xyz(-1.0, 0.25, -7.5), "material_type": "dielectric", "material_param": 1.8},
            {"radius": 0.75, "center": xyz(2.0, -0.25, -6.0), "material_type": "metal", "albedo": xyz(0.8, 0.3, 0.3), "material_param": 0.125},
            {"radius": 0.5, "center": xyz(0.5, -0.5, -4.5), "material_type": "a \"lambert\" one", "albedo": xyz(0.1, 0.7, 0.2)}],
    }


def spell_scene(scene: dict, seed: int) -> str:
    """The scene as YAML in the style seed `seed` picks: key order, block or flow, quoting, comments and blank lines, the
    spelling of each number, indentation width, LF or CRLF."""
    g = Gen(seed)
    r = g.r

    def number(x: float) -> str:
        forms = [repr(x)]
        if x > 0:
            forms.append("+" + repr(x))
        if x == int(x):
            forms += [str(int(x)), str(int(x)) + "."]
        if "." in repr(x) and "e" not in repr(x):
            forms += [repr(x) + "0", repr(x).lstrip("0") if 0 < x < 1 else repr(x)]
        return r.choice(forms)

    def tree(v):
        if isinstance(v, dict):
            pairs = [[k, tree(x)] for k, x in v.items()]
            r.shuffle(pairs)
            return {"map": pairs}
        if isinstance(v, list):
            return {"list": [tree(x) for x in v]}
        if isinstance(v, str):
            return {"s": v}
        return {"s": number(float(v)), "plain": True}
    return g.write(tree(scene))


# ---- outside the subset, valid YAML ---------------------------------------------------------------------------------------------
OUTSIDE = [
    ("flow-seq-next-line", "a: [1, 2,\n  3]"),
    ("flow-map-next-line", "a: {x: 1,\n  y: 2}"),
    ("flow-seq-comment-next-line", "a: [1, # one\n  2]"),
    ("single-quote-escape", "a: 'it''s'"),
    ("single-quote-escape-key", "'it''s': 1"),
    ("single-quote-escape-flow", "a: ['it''s', 'x''', '''']"),
    ("double-quote-escape", 'a: "x\\"y"'),
    ("double-quote-escape-hash", 'a: "x\\" # y" # c'),
    ("double-quote-escape-flow", 'a: {"k\\"": "v\\"", b: 2}'),
    ("literal-block", "a: |\n  line one\n  line two\nb: 1"),
    ("folded-block", "a: >\n  line one\n  line two\nb: 1"),
    ("literal-block-chomp", "a: |-\n  text\n"),
    ("multi-line-plain", "a: one\n  two\nb: 1"),
    ("multi-line-single", "a: 'one\n  two'\nb: 1"),
    ("multi-line-double", 'a: "one\n  two"\nb: 1'),
    ("multi-line-double-folded", 'a: "one\\\n  two"'),
    ("complex-key", "? key\n: value"),
    ("complex-key-alone", "? key"),
    ("flow-map-key-only", "a: {k}"),
    ("flow-map-key-only-2", "a: {k, j: 1}"),
    ("flow-map-adjacent", "a: {k:1}"),
    ("flow-map-null-value", "a: {k: , j: 1}"),
    ("anchor-alias", "a: &anc 5\nb: *anc"),
    ("anchor-on-map", "a: &m\n  x: 1\nb: *m"),
    ("anchor-in-flow", "a: [&p 1, *p]"),
    ("merge-key", "base: &b {x: 1}\nc:\n  <<: *b\n  y: 2"),
    ("tag-str", "a: !!str 5"),
    ("tag-local", "a: !sphere {r: 1}"),
    ("tag-on-block", "a: !!map\n  x: 1"),
    ("tag-in-flow", "a: [!!float 1, 2]"),
    ("two-documents", "---\na: 1\n---\nb: 2"),
    ("two-documents-implicit", "a: 1\n---\nb: 2"),
    ("two-documents-end-marker", "a: 1\n...\n---\nb: 2"),
    ("document-with-content-on-marker", "--- a"),
    ("document-marker-map", "--- {a: 1}"),
    ("empty-documents", "---\n---\n"),
    ("directive", "%YAML 1.1\n---\na: 1"),
    ("escape-x", 'a: "\\x41\\xe9"'),
    ("escape-u", 'a: "\\u00e9\\u2028"'),
    ("escape-U", 'a: "\\U0001F600"'),
    ("escape-0", 'a: "x\\0y"'),
    ("escape-others", 'a: "\\a\\b\\e\\f\\r\\v\\/\\ \\_\\N\\L\\P"'),
    ("escape-mixed", 'a: "é\\x41\\n"'),
    ("escape-in-key", '"k\\x41": 1'),
    ("trailing-comma-seq", "a: [1, 2,]"),
    ("trailing-comma-seq-blank", "a: [x, y, z, ]"),
    ("trailing-comma-map", "a: {x: 1, y: 2,}"),
    ("trailing-comma-nested", "a: [[1,], {k: v,},]"),
    ("single-pair-in-seq", "a: [a:b, c: d]"),
    ("single-pair-in-seq-2", "a: [x: 1, y: 2]"),
    ("single-pair-quoted", 'a: ["k": v]'),
    ("single-pair-nested", "a: [[p: q]]"),
    ("duplicate-key", "a: 1\na: 2"),
    ("duplicate-key-nested", "s:\n  - radius: 1\n    center: 0\n    radius: 2"),
    ("duplicate-key-flow", "a: {x: 1, x: 2}"),
    ("duplicate-key-quoted", "a: 1\n'a': 2\n\"a\": 3"),
    ("apostrophe-before-comment", "a: it's # c"),
    ("apostrophe-before-comment-key", "it's: 1 # c"),
    ("double-quote-before-comment", 'a: 5" pipe # c'),
    ("apostrophes-before-comment", "a: l'un # c'est\nb: x # y"),
    ("apostrophe-before-comment-list", "- it's # c\n- b"),
    ("apostrophe-before-comment-flow", "a: [it's, b] # c"),
    ("apostrophe-then-quoted", "a: [it's, 'b # c'] # d"),
    ("plain-with-dash", "a: b - c"),
    ("plain-with-colon", "a: b:c"),
    ("plain-ends-bracket", "a: 1]"),
    ("plain-question", "a: ?x"),
    ("flow-top-level-map-key", "[a, b]: 1"),
    ("indented-top-level", "  a: 1\n  b: 2"),
    ("comment-glued-to-flow", "a: [1]#c"),
    ("quoted-adjacent-colon-flow", 'a: {"k":1}'),
    ("null-in-flow-seq", "a: [~, null, '']"),
    ("dash-dash", "- - - 1\n    - 2"),
    ("bom", "\ufeffa: 1"),
]


def _nest(text: str, r: random.Random) -> str:
    w = r.randint(1, 6)
    return "outer:\n" + "".join(" " * w + line + "\n" for line in text.split("\n")) + f"after: {r.choice(NUMBERS)}\n"


def _item(text: str, r: random.Random) -> str:
    lines = text.split("\n")
    return f"- {r.choice(WORDS[:6])}\n- " + "".join(("  " if i else "") + line + "\n" for i, line in enumerate(lines)) + "- last\n"


def outside_cases():
    out = []
    r = random.Random(20240)
    nestable = lambda t: not t.startswith(("---", "%", "  ", "\ufeff")) and "\n---" not in t and "\n..." not in t  # noqa: E731
    for name, text in OUTSIDE:
        out.append((f"outside/{name}", text + r.choice(["", "\n", "\r\n" if "\n" not in text else "\n"])))
        if nestable(text) and N_OUTSIDE_CONTEXTS >= 2:
            out.append((f"outside/{name}/nested", _nest(text, r)))
        if nestable(text) and N_OUTSIDE_CONTEXTS >= 3:
            out.append((f"outside/{name}/item", _item(text, r)))
    return out


# ---- malformed -----------------------------------------------------------------------------------------------------------------------
# Each entry is refused by YAML 1.2 whatever the reader: (name, text, why).
TABLE_BAD = [
    ("value-in-value", "a: b: c", "a mapping value inside a plain scalar on one line (7.3.3: `: ` ends a plain scalar)"),
    ("value-in-value-2", "a: x: y", "the same"),
    ("value-in-value-end", "a: b:", "the same, with an empty value"),
    ("seq-in-value", "a: - 1", "a block sequence cannot start behind a key on its line (8.2.1)"),
    ("seq-in-value-alone", "a: -", "the same, with an empty entry"),
    ("open-flow-seq", "a: [1, 2", "unbalanced bracket"),
    ("open-flow-map", "a: {x: 1", "unbalanced brace"),
    ("mismatched-flow", "a: [1, 2}", "a sequence closed by a brace"),
    ("mismatched-flow-2", "a: {x: 1]", "a mapping closed by a bracket"),
    ("close-after-flow", "a: [1, 2]]", "content behind the collection"),
    ("text-after-flow", "a: [1, 2] x", "content behind the collection"),
    ("text-after-quoted", "a: 'x' y", "content behind a quoted scalar"),
    ("open-double-quote", 'a: "x', "an unterminated double-quoted scalar"),
    ("open-single-quote", "a: 'x", "an unterminated single-quoted scalar"),
    ("open-single-quote-escape", "a: 'x''", "`''` is an escaped quote: the scalar is not terminated"),
    ("two-scalars", '"a" 1', "two scalars on one line without an indicator between them"),
    ("bad-indent-less", "a:\n    b: 1\n  c: 2", "indentation that matches no open block"),
    ("bad-indent-more", "a: 1\n  b: 2", "a deeper key behind a finished value"),
    ("bad-indent-seq", "a:\n  - 1\n - 2", "a sequence entry at an indentation between two blocks"),
    ("tab-indent", "a:\n\tb: 1", "a tab as indentation (6.1)"),
    ("tab-indent-2", "a:\n  b: 1\n\tc: 2", "a tab as indentation (6.1)"),
    ("seq-then-map", "- a\nb: 1", "a mapping entry inside a block sequence's indentation"),
    ("map-then-seq", "a: 1\n- b", "a sequence entry inside a block mapping's indentation"),
    ("reserved-at", "a: @x", "`@` is reserved and cannot start a plain scalar (5.3)"),
    ("reserved-tick", "a: `x", "'`' is reserved and cannot start a plain scalar (5.3)"),
    ("percent-start", "a: %x", "`%` is an indicator and cannot start a plain scalar (7.3.3)"),
    ("comma-start", "a: , x", "a flow indicator cannot start a plain scalar (7.3.3)"),
    ("bracket-start", "a: ] x", "a flow indicator cannot start a plain scalar (7.3.3)"),
    ("brace-start", "a: }", "a flow indicator cannot start a plain scalar (7.3.3)"),
    ("unknown-escape", 'a: "\\q"', "`\\q` is no escape (5.7)"),
    ("unknown-escape-apostrophe", "a: \"\\'\"", "`\\'` is no escape (5.7)"),
    ("short-escape-x", 'a: "\\x4"', "`\\x` needs two hexadecimal digits"),
    ("short-escape-u", 'a: "\\u12"', "`\\u` needs four hexadecimal digits"),
    ("bad-escape-U", 'a: "\\U0000zzzz"', "`\\U` needs eight hexadecimal digits"),
    ("undefined-alias", "a: *nowhere", "an alias without its anchor"),
    ("empty-anchor", "a: & 1", "an anchor without a name"),
    ("scalar-then-key", "a\n  b: 1", "a mapping value inside a multi-line plain scalar"),
    ("double-comma", "a: [1,, 2]", "an empty entry in a flow sequence (7.4.1)"),
    ("leading-comma", "a: [, 1]", "an empty entry in a flow sequence (7.4.1)"),
    ("dash-in-flow", "a: [- 1]", "a block sequence entry inside a flow sequence"),
    ("key-in-flow-value", "a: {x: y: z}", "a mapping value inside a flow-mapping value"),
    ("directive-without-document", "%YAML 1.2\na: 1", "a directive that no `---` follows (9.1.2)"),
    ("content-after-end-marker-flow", "a: [1\n...\n]", "a document end marker inside a flow collection"),
]

FLIPS = " :-[]{}#x\n\t0'\",&*!|>?%@`\\"


def mutation_cases(in_cases):
    r = random.Random(777)
    pool = [t for _, t in in_cases if len(t) > 20]
    out = []
    for k in range(N_MUTATIONS):
        t = r.choice(pool)
        if k % 4 == 0:
            t = t[:r.randrange(1, len(t))]
        else:
            for _ in range(r.choice([1, 1, 2])):
                p = r.randrange(len(t))
                t = t[:p] + r.choice(FLIPS) + t[p + 1:]
        out.append((f"bad/mutation{k}", t))
    return out


# ---- the expected trees (PyYAML) -------------------------------------------------------------------------------------------------
def expected(text: str):
    """{"tree": ..} as PyYAML's composer sees the text, or {"error": "<the exception's class>"}."""
    import yaml

    def conv(n):
        if isinstance(n, yaml.ScalarNode):
            if n.style is None and n.value == "":
                return None
            return {"s": n.value, "q": n.style is not None}
        if isinstance(n, yaml.SequenceNode):
            return {"list": [conv(v) for v in n.value]}
        return {"map": [[k.value if isinstance(k, yaml.ScalarNode) else "<collection>", conv(v)] for k, v in n.value]}
    try:
        docs = list(yaml.compose_all(text, Loader=yaml.BaseLoader))
    except yaml.YAMLError as e:
        return {"error": type(e).__name__}
    if len(docs) > 1:
        return {"tree": {"documents": [conv(d) for d in docs]}}
    return {"tree": conv(docs[0]) if docs else None}


def corpus():
    """The whole corpus, as tests/golden/yaml_corpus.json holds it."""
    ins = in_subset_cases()
    cases = [dict(id=i, cls="in", text=t, expect=expected(t)) for i, t in ins]
    cases += [dict(id=i, cls="outside", text=t, expect=expected(t)) for i, t in outside_cases()]
    cases += [dict(id=f"bad/table/{n}", cls="bad-table", text=t, expect=expected(t), why=w) for n, t, w in TABLE_BAD]
    cases += [dict(id=i, cls="bad-mutation", text=t, expect=expected(t)) for i, t in mutation_cases(ins)]
    assert len({c["id"] for c in cases}) == len(cases)
    return {"format": 1, "pyyaml": "BaseLoader, compose_all", "cases": cases}
