"""Which kernel every kn_* launcher of src/nnet2/ launches, pinned without a GPU
(test_conv_routes.py's counterpart).

scripts/nnet2_launch_log.cc loads libkcnn.so, defines hipLaunchKernel itself and
logs what a launcher launches for the operands of a case (fake device pointers
of the stated alignment).  Every case of tests/nnet2_kernel_cases.py must launch
exactly the kernels it names, with their grid, block and dynamic LDS, so a GPU
case cannot go green on another instantiation than the one it is for; every
instantiation the dispatch can pick must have a case; and the arguments a
launcher refuses are given here, where nothing can run.
"""
import os
import re
import subprocess
import sys

import pytest

import kcnn
import nnet2_kernel_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")


def build(tmp, name, extra=()):
    exe = os.path.join(tmp, name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(ROOT, "include"), *extra,
                    os.path.join(SCRIPTS, name + ".cc"), "-o", exe, "-rdynamic", "-ldl"],
                   check=True)
    return exe


def parse(text):
    """[(return code, [(kernel, grid, block, lds), ...]), ...], one a case."""
    out, launches = [], None
    for ln in text.splitlines():
        if re.match(r"case \d+$", ln):
            assert launches is None, "a case without a return code"
            launches = []
            continue
        m = re.match(r"  K (.*) grid (\d+),(\d+),(\d+) block (\d+),(\d+),(\d+) lds (\d+)$", ln)
        if m:
            v = [int(x) for x in m.groups()[1:]]
            launches.append((m.group(1), tuple(v[:3]), tuple(v[3:6]), v[6]))
            continue
        m = re.match(r" rc (-?\d+)$", ln)
        assert m, f"unexpected line {ln!r}"
        out.append((int(m.group(1)), launches))
        launches = None
    assert launches is None
    return out


@pytest.fixture(scope="module")
def log(tmp_path_factory):
    """name -> (return code, launches) of every case and refusal of the table."""
    tmp = str(tmp_path_factory.mktemp("nnet2log"))
    exe = build(tmp, "nnet2_launch_log", ["-I" + os.path.join(ROOT, "kaldi-cnn_amd", "src", "nnet2")])
    assert os.path.exists(kcnn.LIB_PATH), "libkcnn.so is not built"
    cases = T.CASES + T.REFUSALS
    raw = os.path.join(tmp, "log.raw")
    with open(raw, "w") as f:
        subprocess.run([exe, kcnn.LIB_PATH], input="".join(T.line(c) + "\n" for c in cases),
                       stdout=f, text=True, check=True)
    named = subprocess.run([sys.executable, os.path.join(SCRIPTS, "conv_launch_names.py"),
                            "--short", kcnn.LIB_PATH, raw], capture_output=True, text=True,
                           check=True)
    assert named.stderr.strip() == "unnamed handles: 0", named.stderr
    records = parse(named.stdout)
    assert len(records) == len(cases)
    return {c["name"]: r for c, r in zip(cases, records)}


@pytest.mark.parametrize("case", T.CASES, ids=T.name_of)
def test_case_launches_its_kernels(log, case):
    rc, launched = log[case["name"]]
    assert rc == 0, f"returned {rc}"
    assert launched == case["kernels"]


@pytest.mark.parametrize("case", T.REFUSALS, ids=T.name_of)
def test_refusal_launches_nothing(log, case):
    rc, launched = log[case["name"]]
    assert rc == T.HIP_ERROR_INVALID_VALUE
    assert launched == []


def test_refusals_name_every_launcher():
    assert {c["launcher"] for c in T.REFUSALS} == set(T.LAUNCHERS) - {"kn_dvec_update"}
    # (kn_dvec_update has no argument it refuses: n <= 0 is nothing to do)


# ---- every instantiation the dispatch can pick ---------------------------------------------
# From the launchers (dispatch_kernel<...> with lane_width's 1 | 2 | 4, with_bool,
# the if-ladders), not from the log.
V = (1, 2, 4)
BOOL = ("false", "true")
SOFTMAX_TOT = (4, 16, 64)          # dispatch_kernel<4, 16, 64>
NORM_WAVE_TOT = (4, 16, 32, 64)    # dispatch_kernel<4, 16, 32, 64>
NORM_BLOCK_TOT = (32, 64)          # dispatch_kernel<32, 64>

EXPECTED = set()
for v in V:
    for tot in SOFTMAX_TOT:
        EXPECTED |= {f"softmax_prop_wave_kernel<{v}, {tot}>",
                     f"softmax_loglikes_wave_kernel<{v}, {tot}>"}
        EXPECTED |= {f"{k}<{v}, {tot}, {flag}>" for flag in BOOL
                     for k in ("softmax_backprop_wave_kernel", "softmax_xent_wave_kernel",
                               "objf_accuracy_wave_kernel")}
    for which in ("prop", "backprop"):
        EXPECTED |= {f"normalize_{which}_wave_kernel<{v}, {tot}>" for tot in NORM_WAVE_TOT}
        EXPECTED |= {f"normalize_{which}_block_kernel<{v}, {tot}>" for tot in NORM_BLOCK_TOT}
EXPECTED |= {"softmax_prop_block_kernel", "softmax_backprop_block_kernel",
             "softmax_xent_block_kernel", "softmax_loglikes_block_kernel",
             "objf_accuracy_block_kernel<false>", "objf_accuracy_block_kernel<true>",
             "colsum_part_kernel", "colsum_final_kernel", "objf_final_kernel",
             "prob_final_kernel", "comp_objf_kernel", "loglikes_kernel",
             "normalize_prop_reread_kernel", "normalize_backprop_reread_kernel",
             "relu_prop_kernel", "relu_prop4_kernel", "relu_backprop_kernel",
             "relu_backprop4_kernel", "relu_stats_final_kernel", "splice_prop_kernel",
             "splice_backprop_kernel", "dvec_update_kernel"}
EXPECTED |= {f"timemap_epilogue_kernel<{v}, {p}, {r}>" for v in (1, 4)
             for p, r in (("true", "true"), ("true", "false"), ("false", "true"))}
EXPECTED |= {f"timemap_gather_kernel<{vl}, {vs}>" for vl in BOOL for vs in BOOL}
# No exemption: every instantiation above is reachable.  (timemap_epilogue_kernel
# <V, false, false> does not exist: the launcher refuses a call with neither output.)


def named_kernels():
    return {k[0] for c in T.CASES for k in c["kernels"]}


def test_every_reachable_instantiation_has_a_case(log):
    launched = {k[0] for c in T.CASES for k in log[c["name"]][1]}
    missing = EXPECTED - named_kernels()
    assert not missing, f"no case for {sorted(missing)}"
    assert EXPECTED - launched == set()
    assert named_kernels() <= EXPECTED, sorted(named_kernels() - EXPECTED)


def test_expected_set_is_what_the_library_holds():
    """The kernels of the templates above that libkcnn.so was built with are the
    enumeration: an instantiation added to a dispatcher shows up here."""
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "-t", "-C", kcnn.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    stems = {k.split("<")[0] for k in EXPECTED}
    held = set()
    for m in re.finditer(r"__device_stub__([A-Za-z0-9_]+)(<[^(]*>)?\(", out):
        if m.group(1) in stems:
            held.add(m.group(1) + (m.group(2) or ""))
    assert held == EXPECTED, (sorted(held - EXPECTED), sorted(EXPECTED - held))


@pytest.mark.parametrize("launcher,cuts", [(n, T.NORM_CUTS if n.startswith("kn_normalize")
                                            else T.SOFTMAX_CUTS) for n in T.ROW_LAUNCHERS])
def test_both_sides_of_every_cut(launcher, cuts):
    cols = {c["cols"] for c in T.select(launcher)}
    for cut in cuts:
        assert {cut, cut + 1} <= cols, (launcher, cut)
    # and at each step in the values a lane holds, every access width on both sides
    for cut in cuts[:-1]:
        for side in (cut, cut + 1):
            assert {c["v"] for c in T.select(launcher) if c["cols"] == side} == {1, 2, 4}


# the paths of the copy kernels that the geometry of a launch does not show by a
# template argument: each is a tag on the case that is shaped for it
PATHS = {
    "kn_timemap_gather": ["VL+VS", "VL off", "VL off, VS off", "VS off: stride", "VS off: lead",
                          "tc 128", "partial last tile", "run with a 2-float tail", "tc 2",
                          "tc 1", "two tiles at tc 256", "row stride",
                          "utterances with ext > 0"],
    "kn_timemap_epilogue": ["both levels", "scalar: base", "pool_channel 4", "special values",
                            "V 4, two column blocks", "scalar, two column blocks", "row stride",
                            "p_dim.rows > rows"],
    "kn_splice_prop": ["pitched", "const tail", "table with a const tail",
                       "non-monotone in_index", "grid_for cap"],
    "kn_splice_backprop": ["pitched", "const tail", "table with a const tail",
                           "non-monotone in_index", "grid_for cap"],
}


@pytest.mark.parametrize("launcher", list(PATHS))
def test_listed_paths_have_cases(launcher):
    tags = {t for c in T.select(launcher) for t in c["paths"]}
    assert set(PATHS[launcher]) <= tags


def test_path_cases_have_the_geometry_they_are_named_for():
    by = {c["name"]: c for c in T.CASES}

    def grid(name):
        return by[name]["kernels"][0][1]
    # gather: grid.y tiles of tc channels, rows capped at 32768 blocks
    assert grid("gather-d")[1] == 2 and by["gather-d"]["channels"] - 128 == 4
    assert grid("gather-e")[1] == 2 and (by["gather-e"]["channels"] - 128) * 33 == 66
    assert grid("gather-f")[1] == 2 and grid("gather-g")[1] == 2 and grid("gather-h")[1] == 2
    assert grid("gather-i")[0] == 32768 < by["gather-i"]["ops"][1][0]
    assert by["gather-j"]["ext"] > 0 and by["gather-j"]["dilation"] == 2
    for name, c in by.items():
        if c["launcher"] == "kn_timemap_gather":
            assert c["tc"] * c["positions"] <= 8192 and (c["tc"] == 256 or
                                                          2 * c["tc"] * c["positions"] > 8192)
    # epilogue and ReLU: a second column block; fewer row blocks than rows
    assert grid("epilogue-1028")[0] == 2 and grid("epilogue-257")[0] == 2
    assert grid("epilogue-8200-v4")[1] == 8193 == grid("epilogue-8200-v1")[1]
    assert grid("relu_prop-8200x8")[1] == 8193 == grid("relu_prop-8200x5")[1]
    assert grid("relu_prop-2x1028")[0] == 2 == grid("relu_prop-2x257")[0]
    assert grid("relu_backprop-stats-1089x260") == (2, 18, 1)
    # splice: one pass of 8192 blocks does not cover the elements
    for name in ("splice_prop-big", "splice_backprop-big"):
        assert grid(name)[0] == 8192 and 8192 * 256 < 2112000
    tab = by["splice_prop-table"]["in_index"]
    assert any(a > b for a, b in zip(tab, tab[1:])) and by["splice_prop-table"]["const_dim"] > 0


def test_conv_launch_log_still_builds_from_the_shared_header(tmp_path):
    """conv_launch_log.cc and nnet2_launch_log.cc include one launch_log.h."""
    for name in ("conv_launch_log.cc", "nnet2_launch_log.cc"):
        assert '#include "launch_log.h"' in open(os.path.join(SCRIPTS, name)).read()
    exe = build(str(tmp_path), "conv_launch_log")
    out = subprocess.run([exe, kcnn.LIB_PATH, "3,4,1,2,2,3,0,0"], capture_output=True, text=True,
                         check=True).stdout
    assert out.startswith("shape 3 4 1 2 2 3 0 0 R 9 mis 0\n ws ") and "  K " in out
