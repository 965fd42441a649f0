"""Which kernel kn_timemap_conv and kn_stream_segments launch, pinned without a
GPU (tests/test_nnet2_routes.py's counterpart for the time-shared streaming
step, with a case table of its own).

scripts/stream_shared_launch_log.cc loads libkcnn.so, defines hipLaunchKernel
itself and logs what a launcher launches for the operands of a case (fake
device pointers of the stated alignment).  Every case must launch exactly the
kernel it names, with its grid and block; every instantiation the dispatch can
pick must have a case and be in the library; the arguments a launcher refuses
launch nothing."""
import os
import re
import subprocess
import sys

import pytest

import kcnn
from test_nnet2_routes import ROOT, SCRIPTS, build, parse

INVALID = 1  # hipErrorInvalidValue


def ceil(a, b):
    return -(-a // b)


def conv(name, rows, channels, group, kw, delta, layout, in_extra=0, in_lead=0, relu=0,
         swap=None):
    """A kn_timemap_conv case: `in` holds exactly the rows the highest tap
    reads, W exactly kw x C rows; vec: 16-byte loads of `in`.  swap: operands
    ("in", "w", "out") and arguments given other values, for the refusals."""
    wc, wd = (1, channels) if layout == "splice" else (kw, 1)
    ops = {"in": (rows + delta * (kw - 1), channels, channels + in_extra, in_lead),
           "w": (kw * channels, group, group + 1, 0), "out": (rows, group, group + 3, 0)}
    args = {"bias_null": 0, "rows": rows, "kw": kw, "delta": delta, "wc": wc, "wd": wd,
            "relu": relu}
    for k, v in (swap or {}).items():
        assert k in ops or k in args
        (ops if k in ops else args)[k] = v
    vec = channels % 4 == 0 and (channels + in_extra) % 4 == 0 and in_lead % 4 == 0
    kernel = f"timemap_conv_kernel<{str(vec).lower()}, {str(bool(relu)).lower()}>"
    line = [0, *ops["in"], *ops["w"], *ops["out"], *(args[k] for k in (
        "bias_null", "rows", "kw", "delta", "wc", "wd", "relu"))]
    return {"name": name, "line": " ".join(map(str, line)),
            "kernels": [(kernel, (ceil(group, 32), ceil(rows, 32), 1), (256, 1, 1), 0)]}


def segments(name, arena_rows, map_rows, cols, arena_extra=0, arena_lead=0, map_extra=0,
             map_lead=0, num=3, swap=None):
    ops = {"arena": (arena_rows, cols, cols + arena_extra, arena_lead),
           "map": (map_rows, cols, cols + map_extra, map_lead)}
    args = {"desc_null": 0, "num": num}
    for k, v in (swap or {}).items():
        assert k in ops or k in args
        (ops if k in ops else args)[k] = v
    vec = cols % 4 == 0 and all(v % 4 == 0 for v in (arena_extra, arena_lead, map_extra, map_lead))
    units = cols // (4 if vec else 1)
    rpb = max(1, min(64, 1024 // units))
    line = [1, *ops["arena"], *ops["map"], args["desc_null"], args["num"]]
    return {"name": name, "line": " ".join(map(str, line)),
            "kernels": [(f"stream_segments_kernel<{4 if vec else 1}>",
                         (min(ceil(map_rows, rpb), 1024), 1, 1), (256, 1, 1), 0)]}


CASES = [
    # nnet.config's levels at the bench's 1152 rows: the Splice level, a 128-, a
    # 256- and a 512-channel one (576 blocks on 256 CUs)
    conv("conv-splice-1152", 1152 - 3, 40, 128, 4, 1, "splice", relu=1),
    conv("conv-128-1152", 1152 - 5, 128, 128, 3, 1, "above", relu=1),
    conv("conv-256-pool", 1152 - 9, 256, 256, 3, 1, "above"),
    conv("conv-512-1152", 1152 - 17, 512, 512, 3, 2, "above", relu=1),
    # the ragged edges: one row, a partial row and column block, C % 4 != 0
    conv("conv-1x3x1", 1, 3, 1, 1, 1, "above"),
    conv("conv-33x20x48", 33, 20, 48, 4, 4, "above", relu=1),
    conv("conv-c3-splice", 33, 3, 5, 4, 2, "splice", relu=1),
    # 4-byte loads by the stride and by the base
    conv("conv-stride", 70, 40, 128, 4, 1, "splice", in_extra=3),
    conv("conv-base", 31, 16, 32, 3, 1, "above", in_lead=1, relu=1),
    conv("conv-base-2", 31, 16, 32, 3, 1, "above", in_lead=2),
    segments("segments-40", 2 * 32 * 36, 1152, 40),
    segments("segments-pitched", 40, 34, 8, arena_extra=4, map_extra=4),
    segments("segments-stride", 40, 34, 8, arena_extra=3),
    segments("segments-map-stride", 40, 34, 8, map_extra=2),
    segments("segments-arena-base", 40, 34, 8, arena_lead=1),
    segments("segments-map-base", 40, 34, 8, map_lead=1),
    segments("segments-cols-5", 40, 34, 5),
    segments("segments-wide", 40, 34, 4100),         # a row a group
    segments("segments-many-groups", 40, 70000, 64),  # more groups than blocks
]

_C = (5, 8, 8, 3, 2, "above")   # in [9 x 8], w [24 x 8], out [5 x 8]
_S = (40, 34, 8)
REFUSALS = [conv(name, *_C, swap=swap) for name, swap in (
    ("no in", {"in": (9, 8, 8, -1)}),
    ("no w", {"w": (24, 8, 9, -1)}),
    ("no out", {"out": (5, 8, 11, -1)}),
    ("no bias", {"bias_null": 1}),
    ("rows 0", {"rows": 0}),
    ("kw 0", {"kw": 0}),
    ("delta 0", {"delta": 0}),
    ("wc 0", {"wc": 0}),
    ("wd 0", {"wd": 0}),
    ("the highest tap is no row of in", {"in": (8, 8, 8, 0)}),
    ("one row more than in holds", {"rows": 6, "out": (6, 8, 11, 0)}),
    ("the highest weight row is no row of w", {"w": (23, 8, 9, 0)}),
    ("the Splice layout on fewer weight rows", {"wc": 1, "wd": 9}),
    ("out of fewer rows", {"out": (4, 8, 11, 0)}),
    ("out of other columns", {"out": (5, 9, 11, 0)}),
    ("in stride < cols", {"in": (9, 8, 7, 0)}),
    ("w stride < cols", {"w": (24, 8, 7, 0)}),
    ("out stride < cols", {"out": (5, 8, 7, 0)}),
)] + [conv("more row blocks than a grid holds", 65535 * 32 + 1, 4, 4, 1, 1, "above")] + [
    segments(name, *_S, swap=swap) for name, swap in (
        ("no arena", {"arena": (40, 8, 8, -1)}),
        ("no map", {"map": (34, 8, 8, -1)}),
        ("no descriptors", {"desc_null": 1}),
        ("no segments", {"num": 0}),
        ("map of other columns", {"map": (34, 7, 8, 0)}),
        ("arena stride < cols", {"arena": (40, 8, 7, 0)}),
        ("map stride < cols", {"map": (34, 8, 7, 0)}),
        ("no map rows", {"map": (0, 8, 8, 0)}),
        ("an arena of 2^31 elements", {"arena": (1 << 28, 8, 8, 0)}),
    )]


def name_of(c):
    return c["name"]


@pytest.fixture(scope="module")
def log(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("sharedlog"))
    exe = build(tmp, "stream_shared_launch_log",
                ["-I" + os.path.join(ROOT, "kaldi-cnn_amd", "src", "nnet2")])
    assert os.path.exists(kcnn.LIB_PATH), "libkcnn.so is not built"
    cases = CASES + REFUSALS
    raw = os.path.join(tmp, "log.raw")
    with open(raw, "w") as f:
        subprocess.run([exe, kcnn.LIB_PATH], input="".join(c["line"] + "\n" for c in cases),
                       stdout=f, text=True, check=True)
    named = subprocess.run([sys.executable, os.path.join(SCRIPTS, "conv_launch_names.py"),
                            "--short", kcnn.LIB_PATH, raw], capture_output=True, text=True,
                           check=True)
    assert named.stderr.strip() == "unnamed handles: 0", named.stderr
    records = parse(named.stdout)
    assert len(records) == len(cases)
    return {c["name"]: r for c, r in zip(cases, records)}


@pytest.mark.parametrize("case", CASES, ids=name_of)
def test_case_launches_its_kernel(log, case):
    rc, launched = log[case["name"]]
    assert rc == 0, f"returned {rc}"
    assert launched == case["kernels"]


@pytest.mark.parametrize("case", REFUSALS, ids=name_of)
def test_refusal_launches_nothing(log, case):
    rc, launched = log[case["name"]]
    assert rc == INVALID
    assert launched == []


EXPECTED = {f"timemap_conv_kernel<{v}, {r}>" for v in ("true", "false") for r in ("true", "false")}
EXPECTED |= {"stream_segments_kernel<4>", "stream_segments_kernel<1>"}


def test_every_reachable_instantiation_has_a_case(log):
    named = {k[0] for c in CASES for k in c["kernels"]}
    launched = {k[0] for c in CASES for k in log[c["name"]][1]}
    assert named == EXPECTED == launched


def test_expected_set_is_what_the_library_holds():
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "-t", "-C", kcnn.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    held = set()
    for m in re.finditer(r"__device_stub__([A-Za-z0-9_]+)(<[^(]*>)?\(", out):
        if m.group(1) in ("timemap_conv_kernel", "stream_segments_kernel"):
            held.add(m.group(1) + (m.group(2) or ""))
    assert held == EXPECTED


def test_the_grid_at_nnet_configs_widest_level():
    """1152 map rows of 512 channels: more blocks than the 256 CUs."""
    (_, grid, _, _), = next(c for c in CASES if c["name"] == "conv-512-1152")["kernels"]
    assert grid == (16, 36, 1) and grid[0] * grid[1] >= 2 * 256
    (_, grid, _, _), = next(c for c in CASES if c["name"] == "segments-many-groups")["kernels"]
    assert grid[0] == 1024 < ceil(70000, 64)
