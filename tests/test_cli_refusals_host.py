"""The command line's refusals, pinned byte for byte: exit code, whole stderr and whole stdout of `rbrt` for every way an
argument can be refused before anything is loaded -- a missing or invalid value of every option, a flag with a value, an unknown
argument, every combination check with its order of precedence -- for the refusals after the scene file is read that need no
device, and for --help and --version. tests/golden/cli_refusals.json has the expected values; `python
tests/test_cli_refusals_host.py --record` writes that file from the binary that is built (the test never does).

No row needs a device. Every check runs before anything is loaded and the last one refuses '--background' with '--environment',
so a row that ends in that pair (SENTINEL) reaches that message exactly when everything in front of it was accepted. The rows run
in an empty directory: every file name in them is relative, "{ROOT}" stands for the repository."""
import json
import struct
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
GOLDEN = Path(__file__).resolve().parent / "golden" / "cli_refusals.json"
SENTINEL = ["--environment", "x.pfm", "--background", "0,0,0"]
PLAIN_SCENE = ["-c", "{ROOT}/scenes/shutter/shutter_spheres.yaml"]
ENV_SCENE = ["-c", "{ROOT}/scenes/environment/environment_spheres.yaml"]

ROWS = []  # argv tails


def row(*argv):  # (the sections overlap here and there: a row stands once)
    if [str(a) for a in argv] not in ROWS:
        ROWS.append([str(a) for a in argv])


def accepted(*argv):  # (or refused by what stands in front of the sentinel)
    row(*argv, *SENTINEL)


# ---- every valued option: (long name, short name, what has to be on for it to be accepted, values) ----------------------------
JUNK = ["", "1x", "nan", "inf", "-0"]
U32 = ["0", "4294967295", "4294967296", "-1", *JUNK]
FLOAT = ["0", "-1", "1e-45", "-1e-45", *JUNK]
U32_MORE = ["0", "1", "1.5", " 1", "+1", *U32[1:]]  # (what the readers share is tried on one option of a kind)
FLOAT_MORE = ["0", "1", "1e39", "-inf", "0x1p-1", " 1", *FLOAT[1:]]
TRIPLE = ["0,0,0", "1,2,3", "-1,0,0", "-0,0,0", "1,2", "1,2,3,4", "1,2,3x", "nan,0,0", "inf,0,0", "0,0,inf", "0,-inf,0", "1e39,0,0", "1 ,2,3", " 1, 2, 3", "1,,3", ""]


def u32_range(lo, hi):
    return [str(v) for v in (lo - 1, lo, hi, hi + 1) if v >= 0] + ["4294967296", *JUNK]


OPTIONS = [
    ("--target_file", "-t", [], ["o.png", ""]),
    ("--height", None, [], U32_MORE),
    ("--width", "-w", [], U32),
    ("--config", "-c", [], ["s.yaml", ""]),
    ("--samples", "-s", [], U32),
    ("--seed", None, [], ["7", "banana", "", "-1", "5x", "18446744073709551616"]),
    ("--gpus", None, [], U32),
    ("--gather", None, [], ["host", "rccl", "Host", "x", ""]),
    ("--report", None, [], ["r.json", "-", ""]),
    ("--pass-samples", None, [], U32),
    ("--checkpoint", None, [], ["c.bin", ""]),
    ("--checkpoint-every", None, [], U32),
    ("--background", None, [], TRIPLE),
    ("--environment", None, [], ["e.pfm", "none", ""]),
    ("--environment-rotation", None, [], FLOAT),
    ("--environment-intensity", None, [], FLOAT),
    ("--environment-resolution", None, [], u32_range(1, 4096)),
    ("--aperture", None, [], FLOAT_MORE),
    ("--focus-distance", None, [], FLOAT),
    ("--shading", None, [], ["flat", "smooth", "Smooth", "x", ""]),
    ("--adaptive", None, [], FLOAT_MORE),
    ("--min-samples", None, ["--adaptive", "0.1"], U32),
    ("--adaptive-step", None, ["--adaptive", "0.1"], U32),
    ("--sample-map", None, ["--adaptive", "0.1"], ["m.png", ""]),
    ("--denoise-radius", None, ["--denoise"], u32_range(0, 10)),
    ("--denoise-patch", None, ["--denoise"], u32_range(0, 4)),
    ("--denoise-strength", None, ["--denoise"], FLOAT),
    ("--noisy", None, ["--denoise"], ["n.png", ""]),
    ("--guided-levels", None, ["--denoise-guided"], u32_range(1, 6)),
    ("--guided-colour", None, ["--denoise-guided"], FLOAT),
    ("--guided-normal", None, ["--denoise-guided"], FLOAT),
    ("--guided-depth", None, ["--denoise-guided"], FLOAT),
    ("--guided-albedo", None, ["--denoise-guided"], FLOAT),
    ("--frames", None, [], ["0", "1", "4294967295", "4294967296", *JUNK]),
    ("--camera-step", None, ["--frames", "2"], TRIPLE),
    ("--shutter-travel", None, [], ["0,0,0", "-1,0,0", "1,2", "nan,0,0", ""]),  # (--camera-step's reader)
    ("--shutter", None, ["--frames", "2", "--camera-step", "1,0,0"], FLOAT),
    ("--temporal-max-history", None, ["--frames", "2"], [*FLOAT, "1", "0.99999994", "0.999999999"]),
    ("--temporal-depth", None, ["--frames", "2"], FLOAT),
    ("--temporal-normal", None, ["--frames", "2"], FLOAT),
    ("--history-map", None, ["--frames", "2"], ["h.png", ""]),
    ("--upscale", None, [], u32_range(2, 4)),
    ("--upscale-normal", None, ["--upscale", "2"], FLOAT),
    ("--upscale-depth", None, ["--upscale", "2"], FLOAT),
    ("--upscale-albedo", None, ["--upscale", "2"], FLOAT),
    ("--despike-threshold", None, ["--despike"], [*FLOAT, "1", "0.99999994", "0.999999999"]),
    ("--despike-rank", None, ["--despike"], u32_range(1, 4)),
    ("--despike-radius", None, ["--despike"], u32_range(1, 2)),
    ("--spike-map", None, ["--despike"], ["k.png", ""]),
    ("--compare", None, [], [""]),  # (a file that is there: below)
    ("--compare-epsilon", None, ["--compare", "ref2x2.pfm", "--width", "2", "--height", "2"], FLOAT),
    ("--error-map", None, ["--compare", "ref2x2.pfm", "--width", "2", "--height", "2"], ["e.png", ""]),
    ("--ssim-map", None, ["--compare", "ref2x2.pfm", "--width", "2", "--height", "2"], ["s.png", ""]),
    ("--exposure", None, [], ["auto", "Auto", "0", "-0", "1.5", "127", "128", "-149", "-150", "nan", "inf", "-inf", "", "1x"]),
    ("--exposure-key", None, [], FLOAT),
    ("--tonemap", None, [], ["none", "reinhard", "aces", "ACES", "x", ""]),
    ("--white", None, ["--tonemap", "reinhard"], ["auto", "Auto", *FLOAT]),
    ("--glare", None, [], [*FLOAT, "1", "1.00000001", "1.0000001"]),
    ("--glare-threshold", None, ["--glare", "0.5"], FLOAT),
    ("--glare-levels", None, ["--glare", "0.5"], u32_range(1, 8)),
    ("--glare-spread", None, ["--glare", "0.5"], FLOAT),
    ("--radiance", None, [], ["r.pfm", ".pfm", "pfm", "r.PFM", "r.pfm.png", ""]),
    ("--features", None, [], ["f", ""]),
    ("--feature-samples", None, ["--features", "f"], u32_range(1, 65536)),
]
for name, short, on, values in OPTIONS:
    row(name)  # the value is missing: the last argument
    if short:
        row(short)
        accepted(*on, short, values[0])
        row(f"{short}={values[0]}")  # (only "--" arguments split at "=")
    for v in values:
        accepted(*on, name, v)
    accepted(*on, f"{name}={values[0]}")
    accepted(*on, f"{name}={values[-1]}")
    accepted(*on, f"{name}=")
# a dash-led token after a valued option is its value
accepted("--target_file", "--denoise")
accepted("--noisy", "--denoise")
accepted("--denoise-radius", "--denoise")
accepted("--samples", "-1")
accepted("--aperture", "-1")
accepted("--aperture", "--focus-distance", "2")
accepted("--seed", "--seed")

# ---- flags: with a value, with an empty value, bare -------------------------------------------------------------------------------
for flag in ("--oversubscribe", "--denoise", "--denoise-guided", "--guided-no-demodulation", "--despike"):
    on = ["--denoise-guided"] if flag == "--guided-no-demodulation" else []
    accepted(*on, flag)
    accepted(*on, f"{flag}=1")
    accepted(*on, f"{flag}=")
    accepted(*on, flag, "1")  # (the value is an argument of its own: unknown)
accepted("--despike=3", "--despike-rank", "1")
accepted("--glare", "1", "--glare-levels", "8", "--despike=3", "--oversubscribe=1")

# ---- --help, --version, unknown arguments, two bad arguments in both orders ----------------------------------------------------------
for a in ("-h", "--help", "-V", "--version", "--help=1", "--version=1", "-h=1"):
    row(a)
for a in ("--bogus", "bogus", "-x", "--bogus=1", "--", "-", "", "=", "--=", "---help", "--Help", "--target-file", "--denoise-guide"):
    row(a)
BAD = [["--width", "x"], ["--bogus"], ["--glare", "2"], ["--denoise=1"], ["--gather", "x"], ["--background", "1,2"], ["--compare", ""]]
for i, a in enumerate(BAD):
    for b in BAD[i + 1:]:
        row(*a, *b)
        row(*b, *a)
for a in BAD:
    row(*a, "--samples")  # an invalid value in front of a missing one
    row("--help", *a)
    row(*a, "--help")
    row(*a, "--version")
    row("--denoise-radius", "3", *a)  # a parse error wins over a combination check, wherever it stands
    row(*a, "--denoise-radius", "3")
row("--help", "--version")
row("--version", "--help")
row("--denoise-radius", "3", "--help")

# ---- the five groups of one shape: conflicts, --samples below 2, dependants ---------------------------------------------------------
CONFLICT = {"--gpus > 1": ["--gpus", "2"], "--checkpoint": ["--checkpoint", "c.bin"], "--pass-samples": ["--pass-samples", "4"],
            "--adaptive": ["--adaptive", "0.1"], "--sample-map": ["--sample-map", "m.png"], "--denoise": ["--denoise"]}
ADAPTIVE_PATH = ["--gpus > 1", "--checkpoint", "--pass-samples"]
GROUPS = [
    (["--denoise"], ADAPTIVE_PATH,
     [["--denoise-radius", "3"], ["--denoise-patch", "2"], ["--denoise-strength", "0.5"], ["--noisy", "n.png"]]),
    (["--denoise-guided"], ["--denoise", *ADAPTIVE_PATH],
     [["--guided-levels", "3"], ["--guided-colour", "1"], ["--guided-normal", "0.2"], ["--guided-depth", "0.1"], ["--guided-albedo", "0.3"],
      ["--guided-no-demodulation"]]),
    (["--frames", "2"], ["--adaptive", *ADAPTIVE_PATH],
     [["--camera-step", "1,0,0"], ["--temporal-max-history", "4"], ["--temporal-depth", "0.1"], ["--temporal-normal", "0.2"], ["--history-map", "h.png"]]),
    (["--upscale", "2"], ["--adaptive", *ADAPTIVE_PATH, "--sample-map"],
     [["--upscale-normal", "0.4"], ["--upscale-depth", "0.2"], ["--upscale-albedo", "0.3"]]),
    (["--despike"], ["--adaptive", *ADAPTIVE_PATH, "--sample-map"],
     [["--despike-threshold", "2"], ["--despike-rank", "1"], ["--despike-radius", "1"], ["--spike-map", "k.png"]]),
]


def group_rows(owner, conflicts, dependants):
    accepted(*owner)
    for a in conflicts:
        accepted(*owner, *CONFLICT[a])
        accepted(*CONFLICT[a], *owner)
    for a, b in zip(conflicts, conflicts[1:]):  # the earlier one of the chain is named
        accepted(*owner, *CONFLICT[a], *CONFLICT[b])
        accepted(*owner, *CONFLICT[b], *CONFLICT[a])
    accepted(*owner, *CONFLICT[conflicts[0]], *CONFLICT[conflicts[-1]])
    for s in ("0", "1", "2"):
        accepted(*owner, "-s", s)
    accepted(*owner, "-s", "1", *CONFLICT[conflicts[0]])  # a conflict wins over --samples below 2
    accepted(*owner, "-s", "1", *CONFLICT[conflicts[-1]])
    for d in dependants:
        accepted(*d)
        accepted(*owner, *d)
        accepted(*d, *owner)
    for a, b in zip(dependants, dependants[1:]):
        accepted(*a, *b)
        accepted(*b, *a)
    accepted(*dependants[0], *dependants[-1])
    everything = [x for d in dependants for x in d]
    accepted(*everything)
    accepted(*owner, *everything)
    accepted(*owner, "-s", "1", *dependants[0])


for g in GROUPS:
    group_rows(*g)

# ---- the four variations -----------------------------------------------------------------------------------------------------------
# adaptive: conflicts, then the two counts in one message, else --sample-map
accepted("--adaptive", "0")
for a in ADAPTIVE_PATH:
    accepted("--adaptive", "0.1", *CONFLICT[a])
for a, b in zip(ADAPTIVE_PATH, ADAPTIVE_PATH[1:]):
    accepted("--adaptive", "0.1", *CONFLICT[a], *CONFLICT[b])
    accepted("--adaptive", "0.1", *CONFLICT[b], *CONFLICT[a])
for m, k in (("2", "1"), ("1", "1"), ("2", "0"), ("1", "0"), ("0", "64"), ("4294967295", "4294967295")):
    accepted("--adaptive", "0.1", "--min-samples", m, "--adaptive-step", k)
accepted("--adaptive", "0.1", "--min-samples", "1", "--gpus", "2")
accepted("--adaptive", "0.1", "--adaptive-step", "0", "--pass-samples", "4")
accepted("--adaptive", "0.1", "-s", "1")
accepted("--adaptive", "0.1", "-s", "0")
accepted("--min-samples", "1")  # (looked at with --adaptive only)
accepted("--adaptive-step", "0")
accepted("--min-samples", "1", "--sample-map", "m.png")
# glare: dependants only
GLARE = [["--glare-threshold", "2"], ["--glare-levels", "3"], ["--glare-spread", "0.5"]]
for d in GLARE:
    accepted(*d)
    accepted("--glare", "0.5", *d)
for a, b in zip(GLARE, GLARE[1:]):
    accepted(*a, *b)
    accepted(*b, *a)
accepted(*GLARE[0], *GLARE[2])
accepted("--glare", "0.5", *[x for d in GLARE for x in d])
# compare: dependants, else the reference is read and its size checked
COMPARE = [["--compare-epsilon", "0.1"], ["--error-map", "e.png"], ["--ssim-map", "s.png"]]
SIZE2 = ["--width", "2", "--height", "2"]
for d in COMPARE:
    accepted(*d)
    accepted("--compare", "ref2x2.pfm", *SIZE2, *d)
    accepted("--compare", "missing.pfm", *d)
for a, b in zip(COMPARE, COMPARE[1:]):
    accepted(*a, *b)
    accepted(*b, *a)
accepted(*COMPARE[0], *COMPARE[2])
accepted("--compare", "ref2x2.pfm", *SIZE2, *[x for d in COMPARE for x in d])
accepted("--compare", "ref2x2.pfm", *SIZE2)
accepted("--compare", "missing.pfm")
accepted("--compare", "ref2x2.pfm")  # 2 x 2 against 800 x 600
accepted("--compare", "ref2x2.pfm", "--width", "2")
accepted("--compare", "ref2x2.pfm", "--height", "2")
accepted("--compare", "ref2x2.pfm", "--width", "2", "--height", "3")
accepted("--compare", "ref2x2.pfm", "--width", "0", "--height", "0")
accepted("--compare", "ref3x2.pfm", "--width", "3", "--height", "2")
accepted("--compare", "ref3x2.pfm", "--width", "2", "--height", "3")
accepted("--compare", "nan2x2.pfm", *SIZE2)  # (any value may stand in a reference)
accepted("--compare", "grey2x2.pfm", *SIZE2)
accepted("--compare", "short2x2.pfm", *SIZE2)
accepted("--compare", "junk.pfm", *SIZE2)
accepted("--compare", "ref2x2.pfm", *SIZE2, "--upscale", "2", "--frames", "2", "--despike", "--denoise")
# features: one conflict, else --feature-samples, which four owners accept
accepted("--features", "f")
accepted("--features", "f", "--gpus", "2")
accepted("--features", "f", "--gpus", "1")
accepted("--features", "f", "--feature-samples", "3")
accepted("--features", "f", "--feature-samples", "3", "--gpus", "2")
accepted("--feature-samples", "3")
accepted("--feature-samples", "3", "--gpus", "2")
for owner in (["--denoise-guided"], ["--frames", "2"], ["--upscale", "2"], ["--denoise"], ["--despike"], ["--adaptive", "0.1"]):
    accepted("--feature-samples", "3", *owner)

# ---- the cross-group special cases ----------------------------------------------------------------------------------------------------
accepted("--noisy", "n.png")
for owner in (["--denoise"], ["--denoise-guided"], ["--upscale", "2"], ["--despike"], ["--frames", "2"], ["--adaptive", "0.1"]):
    accepted("--noisy", "n.png", *owner)
accepted("--noisy", "n.png", "--denoise-radius", "3")
accepted("--noisy", "n.png", "--despike", "--denoise-strength", "1")
accepted("--sample-map", "m.png")
for owner in (["--adaptive", "0.1"], ["--upscale", "2"], ["--despike"], ["--upscale", "2", "--despike"], ["--denoise"], ["--frames", "2"]):
    accepted("--sample-map", "m.png", *owner)
accepted("--sample-map", "m.png", "--adaptive", "0.1", "--upscale", "2")
accepted("--sample-map", "m.png", "--upscale", "2", "--denoise-radius", "3")
accepted("--sample-map", "m.png", "--upscale-normal", "0.4", "--despike")
SHUTTER = ["--frames", "2", "--camera-step", "1,0,0", "--shutter", "0.5"]
accepted(*SHUTTER)
accepted("--shutter", "0.5")
accepted("--frames", "2", "--shutter", "0.5")
accepted("--shutter", "0.5", "--camera-step", "1,0,0")  # (--camera-step needs --frames first)
accepted(*SHUTTER, "--shutter-travel", "1,0,0")
accepted("--shutter", "0.5", "--shutter-travel", "1,0,0")
accepted("--frames", "2", "--shutter", "0.5", "--shutter-travel", "1,0,0")
accepted("--shutter-travel", "1,0,0")
accepted("--shutter-travel", "1,0,0", "--frames", "2", "--camera-step", "1,0,0")
accepted("--shutter-travel", "1,0,0", "--gpus", "2", "--adaptive", "0.1")
accepted("--frames", "2", "--camera-step", "3e38,0,0", "--shutter", "2")
accepted("--frames", "2", "--camera-step", "0,0,-3e38", "--shutter", "2")
accepted("--frames", "2", "--camera-step", "3e38,0,0", "--shutter", "1")
accepted("--frames", "2", "--camera-step", "3e38,0,0", "--shutter", "0")
accepted("--frames", "2", "--camera-step", "0,0,0", "--shutter", "3e38")
accepted("--white", "2")
accepted("--white", "auto")
for curve in ("none", "reinhard", "aces"):
    accepted("--white", "2", "--tonemap", curve)
    accepted("--white", "auto", "--tonemap", curve)
accepted("--tonemap", "reinhard", "--white", "2", "--tonemap", "aces")  # the last one counts
accepted("--radiance", "r.png")
accepted("--radiance", "r")
accepted("--radiance", "dir.pfm/r")

# ---- precedence between the blocks of checks: each block's refusal alone, then each with the next one's ------------------------------
BLOCKS = [
    ("adaptive", ["--sample-map", "m.png"]),
    ("denoise", ["--denoise-radius", "3"]),
    ("denoise-guided", ["--guided-levels", "3"]),
    ("frames", ["--temporal-depth", "0.1"]),
    ("shutter with shutter-travel", ["--shutter", "0.5", "--shutter-travel", "1,0,0"]),
    ("shutter without camera-step", ["--shutter", "0.5"]),
    ("upscale", ["--upscale-normal", "0.4"]),
    ("despike", ["--despike-rank", "1"]),
    ("compare", ["--compare-epsilon", "0.1"]),
    ("glare", ["--glare-levels", "3"]),
    ("features", ["--feature-samples", "3"]),
    ("white", ["--white", "2"]),
    ("radiance", ["--radiance", "r.png"]),
]
for (_, a), (_, b) in zip(BLOCKS, BLOCKS[1:]):
    accepted(*a, *b)
    accepted(*b, *a)
PRODUCT = ["--frames", "2", "--camera-step", "3e38,0,0", "--shutter", "2"]  # (it needs --frames: it stands behind that block by itself)
accepted(*PRODUCT, "--upscale-normal", "0.4")
accepted(*PRODUCT, "--adaptive", "0.1")  # the frames block is in front of it
accepted(*PRODUCT, "--shutter-travel", "1,0,0")
accepted("--despike-rank", "1", "--compare", "missing.pfm")
accepted("--compare", "missing.pfm", "--glare-levels", "3")
accepted("--compare", "ref2x2.pfm", "--glare-levels", "3")
row("--radiance", "r.png", "--environment", "none", "--background", "0,0,0")
row("--environment", "x.pfm", "--background", "1,2")
row("--environment", "none", "--background", "0,0,0", "-c", "missing.yaml")  # nothing refuses: the scene file is read
accepted("--environment", "none")  # (the later --environment counts)

# ---- refusals after the scene file is read that need no device: exit code 101 -------------------------------------------------------
row("-c", "missing.yaml")
row("--config=missing.yaml", "--denoise")
row("-c", "")
ENV_ONLY = [["--environment-rotation", "10"], ["--environment-intensity", "2"], ["--environment-resolution", "64"]]
for d in ENV_ONLY:
    row(*PLAIN_SCENE, *d)
    row(*ENV_SCENE, "--environment", "none", *d)
row(*PLAIN_SCENE, *[x for d in ENV_ONLY for x in d])
row(*PLAIN_SCENE, "--background", "0,0,0", "--environment-rotation", "10")
row(*ENV_SCENE, "--background", "0,0,0")
row(*ENV_SCENE, "--background", "0,0,0", "--environment-rotation", "10")
row(*ENV_SCENE, "--background=1,1,1", "--denoise")


def key(argv):  # (a "+" at the end stands for the sentinel)
    argv = [*argv[:-len(SENTINEL)], "+"] if argv[-len(SENTINEL):] == SENTINEL else argv
    return " ".join(a if a and " " not in a else f"'{a}'" for a in argv)


# The golden groups the rows by what they give: a list of [exit code, stderr, stdout, [rows]].
def grouped(got):
    groups = {}
    for k, v in got.items():
        groups.setdefault(json.dumps(v), []).append(k)
    blocks = []
    for v, keys in groups.items():
        lines, line = [], ""
        for k in map(json.dumps, keys):
            if line and len(line) + len(k) > 150:
                lines.append(line)
                line = ""
            line += (", " if line else "") + k
        blocks.append(" " + v[:-1] + (", [" + line if not lines else ", [\n  " + ",\n  ".join(lines + [line])) + "]]")
    return "[\n" + ",\n".join(blocks) + "\n]\n"


def ungrouped(text):
    return {k: [rc, err, out] for rc, err, out, keys in json.loads(text) for k in keys}


def pfm(path, magic, width, height, values):
    path.write_bytes(f"{magic}\n{width} {height}\n-1.0\n".encode() + struct.pack(f"<{len(values)}f", *values))


def run_rows(exe, cwd):
    """{row: [exit code, stderr, stdout]} of every row, run in the empty directory cwd."""
    assert not any(cwd.iterdir())
    pfm(cwd / "ref2x2.pfm", "PF", 2, 2, [0.5] * 12)
    pfm(cwd / "ref3x2.pfm", "PF", 3, 2, [0.25] * 18)
    pfm(cwd / "nan2x2.pfm", "PF", 2, 2, [float("nan"), -1.0, float("inf")] * 4)
    pfm(cwd / "grey2x2.pfm", "Pf", 2, 2, [0.5] * 4)
    pfm(cwd / "short2x2.pfm", "PF", 2, 2, [0.5] * 11)
    (cwd / "junk.pfm").write_bytes(b"not a picture\n")
    before = sorted(p.name for p in cwd.iterdir())

    def one(argv):
        r = subprocess.run([str(exe), *(a.replace("{ROOT}", str(ROOT)) for a in argv)], cwd=cwd, capture_output=True, text=True, timeout=60)
        return key(argv), [r.returncode, r.stderr, r.stdout]

    with ThreadPoolExecutor(8) as pool:
        got = dict(pool.map(one, ROWS))
    assert len(got) == len(ROWS)
    assert sorted(p.name for p in cwd.iterdir()) == before  # a refused run wrote nothing
    return got


def test_every_cli_refusal_is_what_was_recorded(tmp_path):
    expected = ungrouped(GOLDEN.read_text())
    got = run_rows(EXE, tmp_path)
    assert got.keys() == expected.keys(), sorted(got.keys() ^ expected.keys())[:10]
    wrong = {k: (got[k], v) for k, v in expected.items() if got[k] != v}
    assert not wrong, (len(wrong), list(wrong.items())[:5])
    for k, (rc, err, out) in expected.items():  # (what was recorded: 0 says something on stdout alone, a refusal on stderr alone)
        assert (rc == 0 and out and not err) or (rc in (2, 101) and err and not out), k
        assert str(ROOT) not in err + out, k


if __name__ == "__main__":
    import tempfile

    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_cli_refusals_host.py --record")
    with tempfile.TemporaryDirectory() as d:
        recorded = run_rows(EXE, Path(d))
    for k, (rc, err, out) in recorded.items():
        assert (rc == 0 and out and not err) or (rc in (2, 101) and err and not out), (k, rc, err, out)
    GOLDEN.write_text(grouped(recorded))
    print(f"recorded {len(recorded)} rows in {GOLDEN}")
