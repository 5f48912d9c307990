"""A plain Python restatement of what the C++ host's .obj loader (rbrt_amd/host/scene.cpp) is documented to do, for
tests/test_obj_differential.py. Nothing here shares code with the loader.

  * lines end at '\\n'; blanks, tabs and a '\\r' separate tokens; leading blanks are skipped; unknown statements are ignored
  * `v x y z [more]`: three numbers, read as Rust's str::parse::<f32> reads them (one correct rounding); more are ignored
  * `vn x y z`: a normal; valid when all three are finite numbers (an invalid one still takes its index)
  * `f c c c ...`: corners `v`, `v/vt`, `v//vn`, `v/vt/vn`; 1-based, negative = relative to what was read so far; a corner
    whose position index is 0, out of range or not an integer, or whose token has other text in it, refuses the file
    with `path:line`; a missing, out-of-range or invalid `vn` only leaves the corner without a normal
  * tobj's models: `o`, `g` and `usemtl` close the current model if it has faces; a model's corner indices form one run,
    polygons included (triangulate = false), which is cut into triples; an incomplete last triple is dropped
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

f32 = np.float32


class ObjRefused(Exception):
    def __init__(self, line: int, what: str):
        super().__init__(f"line {line}: {what}")
        self.line = line


def parse_f32(tok: str):
    """The token as a float32 with one rounding (None: no number). Exact: the decimal value against its float32 neighbours."""
    t = tok[1:] if tok[:1] in "+-" else tok
    neg = tok[:1] == "-"
    if t.lower() in ("inf", "infinity", "nan"):
        v = f32(np.nan) if t.lower() == "nan" else f32(np.inf)
        return -v if neg else v
    mant, _, exp = t.lower().partition("e")
    ip, dot, fp = mant.partition(".")
    if not (ip + fp).isdigit() or not (ip + fp).isascii() or ("e" in t.lower() and not (exp.lstrip("+-").isdigit() and exp.isascii()
                                                                                         and len(exp) - len(exp.lstrip("+-")) <= 1)):
        return None
    e = int(exp) if exp else 0
    if abs(e) > 400:
        q = Fraction(0) if (e < 0 or int(ip + fp) == 0) else None
    else:
        q = Fraction(int(ip + fp)) * Fraction(10) ** (e - len(fp))
    big = Fraction(2) ** 128 - Fraction(2) ** 103  # the midpoint between the largest float32 and 2^128
    if q is None or q >= big:
        v = f32(np.inf)
    else:
        with np.errstate(over="ignore"):
            c = f32(float(q))  # (rounded twice: at most one step off)
        cands = [x for x in (np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))) if np.isfinite(x)]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - q), int(x.view(np.uint32)) & 1))
        v = f32(best)
    return -v if neg else v


def _index(v: int, n: int) -> int:
    i = v - 1 if v > 0 else n + v
    return -1 if (v == 0 or i < 0 or i >= n) else i


def _int(s: str):
    body = s[1:] if s[:1] in "+-" else s
    return int(s) if body.isdigit() and body.isascii() else None


def load(text: str):
    """-> (positions (P, 3) float32, normals (Q, 3) float32, models), models = [(faces (N, 3) int, normal_idx (N, 3) int, -1: none)]
    for every model with at least one complete triple... and those without (N = 0), in file order. Raises ObjRefused."""
    pos, nrm, nrm_ok = [], [], []
    models = [([], [])]
    for no, raw in enumerate(text.split("\n"), 1):
        if raw == "" and no == len(text.split("\n")):
            break
        toks = raw.replace("\r", " ").replace("\t", " ").split(" ")
        toks = [t for t in toks if t]
        if not toks:
            continue
        head = toks[0]
        if head == "v":
            vals = [parse_f32(t) for t in toks[1:4]]
            if len(vals) < 3 or any(v is None for v in vals):
                raise ObjRefused(no, "bad vertex")
            pos.append(vals)
        elif head == "vn":
            vals = [parse_f32(t) for t in toks[1:4]]
            ok = len(vals) == 3 and all(v is not None and np.isfinite(v) for v in vals)
            nrm.append([v if v is not None else f32(0) for v in vals] + [f32(0)] * (3 - len(vals)))
            nrm_ok.append(ok)
        elif head == "f":
            for t in toks[1:]:
                parts = t.split("/")
                ints = [(_int(p) if p else None) for p in parts]
                if len(parts) > 3 or any(p and i is None for p, i in zip(parts, ints)) or ints[0] is None:
                    raise ObjRefused(no, "bad face index")
                vi = _index(ints[0], len(pos))
                if vi < 0:
                    raise ObjRefused(no, "bad face index")
                ni = _index(ints[2], len(nrm)) if len(ints) == 3 and ints[2] is not None else -1
                if ni >= 0 and not nrm_ok[ni]:
                    ni = -1
                models[-1][0].append(vi)
                models[-1][1].append(ni)
        elif head in ("o", "g") or head.startswith("usemtl"):
            if models[-1][0]:
                models.append(([], []))
    out = []
    for idx, nidx in models:
        n = len(idx) // 3
        out.append((np.array(idx[:3 * n], np.int64).reshape(n, 3), np.array(nidx[:3 * n], np.int64).reshape(n, 3)))
    return np.array(pos, f32).reshape(-1, 3), np.array(nrm, f32).reshape(-1, 3), out
