"""Which kernels the convolution dispatch launches, pinned without a GPU.

scripts/conv_launch_log.cc is a host program that loads libkcnn.so, defines
hipLaunchKernel itself and logs every launch the hipF_conv2d* entry points make
for a geometry; scripts/conv_launch_names.py names the kernels.  The GPU parity
cases say "this shape reaches that kernel" in a comment; here it is asserted, so
a dispatch change that unreaches a kernel cannot leave its parity case green and
vacuous.  Routes are for 9 rows (5 for the 40 x 61 map), aligned operands, the
full workspace, as the parity tests call them.
"""
import os
import re
import subprocess
import sys

import pytest

import kcnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("conv2d concat", "wgrad", "dgrad", "backward", "backward nodx")
FAMILY_ENV = {"fwd_x6": "KCNN_FWD_X6", "bwd_x6": "KCNN_BWD_X6", "igemm_x6": "KCNN_IGEMM_X6",
              "wgrad_x6": "KCNN_WGRAD_X6"}

FLIP = "elem2d_kernel<(anonymous namespace)::FlipMat>"
RED = "reduce_splits_kernel"
WF1 = ["conv_wgrad_frame_kernel<1>", RED]
WF2 = ["conv_wgrad_frame_kernel<2>", RED]


def bwd_frame(nch):
    """The register-staged fused backward in the three entries with a gradient:
    conv_bwd_frame_kernel needs it, the data gradient alone goes its own ladder."""
    return {"wgrad": [f"conv_bwd_frame_kernel<{nch}, false>", RED],
            "backward": [f"conv_bwd_frame_kernel<{nch}, true>", RED],
            "backward nodx": [f"conv_bwd_frame_kernel<{nch}, false>", RED]}


def unfused(dgrad, wgrad):
    """No fused backward: the data gradient's ladder, then the weight gradient's."""
    return {"wgrad": wgrad, "dgrad": dgrad, "backward": dgrad + wgrad, "backward nodx": wgrad}


# (family setting or None, (H, W, C, kh, kw, G, pad_h, pad_w[, rows])): the
# ordered kernel templates of each entry point that the case is about
ROUTES = {
    # short kernels past the fused backward's map limits (tests/test_gpu_components.py
    # FUSED_BWD bigmap_* and P*): C*H*W > 2048 takes the register-staged kernel ...
    "bigmap_G32": (None, (20, 13, 8, 3, 1, 32, 0, 0), dict(
        bwd_frame(1), dgrad=[FLIP, "conv_direct_smallg_kernel<8>"])),
    "bigmap_pad": (None, (22, 12, 8, 3, 1, 32, 1, 0), dict(
        bwd_frame(1), dgrad=[FLIP, "conv_direct_smallg_kernel<8>"])),
    "bigmap_G64_P480": (None, (33, 16, 4, 2, 2, 64, 0, 0), dict(
        bwd_frame(2), dgrad=["conv_dgrad_frame_kernel<32>"])),
    # ... which takes one filter chunk only: with two, no fused backward at all
    "bigmap_G256": (None, (20, 13, 8, 3, 1, 256, 0, 0),
                    unfused([FLIP, "conv_direct_smallg_kernel<8>"], WF2)),
    "bigmap_G160": (None, (20, 13, 8, 3, 1, 160, 0, 0),
                    unfused([FLIP, "conv_direct_smallg_kernel<8>"], WF2)),
    # P > 512
    "P544_C1": (None, (36, 16, 1, 3, 1, 32, 0, 0),
                unfused([FLIP, "conv_direct_smallg_kernel<1>"], WF1)),
    "P784_G64": (None, (30, 30, 2, 3, 3, 64, 0, 0), unfused(["conv_dgrad_frame_kernel<32>"], WF1)),
    "P578_pad": (None, (33, 16, 4, 2, 2, 64, 1, 1), unfused(["conv_dgrad_frame_kernel<32>"], WF1)),
    "P1947_G256": (None, (40, 61, 1, 8, 3, 256, 0, 0, 5),
                   unfused([FLIP, "conv_direct_smallg_kernel<1>"], WF2)),
    # 384 < P <= 512: the fp32 DMA kernel (the bf16x6 one stops at 384)
    "P504_G128": (None, (43, 13, 1, 2, 2, 128, 0, 0), {
        "wgrad": ["conv_bwd_dma_kernel<4, false, true, 0>", RED],
        "dgrad": ["conv_bwd_dma_kernel<4, true, false, 0>"],
        "backward": ["conv_bwd_dma_kernel<4, true, true, 0>", RED],
        "backward nodx": ["conv_bwd_dma_kernel<4, false, true, 0>", RED]}),
}

TRANSPOSE, COL2IM = "conv_transpose_kernel", "conv_col2im_kernel"
COL2IM_PLANE = "conv_col2im_plane_kernel"
IG_X6_128P = "conv_igemm_x6_kernel<128, true, true, 0, false>"
IG_X6_128 = "conv_igemm_x6_kernel<128, false, true, 0, false>"
IG_X6_256 = "conv_igemm_x6_kernel<256, false, true, 0, false>"
WX6 = ["conv_wgrad_x6w_kernel<false, false>", RED]
WX6P = ["conv_wgrad_x6w_kernel<true, false>", RED]


def fallback(fwd, dgrad, wgrad):
    return dict(unfused(dgrad, wgrad), **{"conv2d concat": fwd})


# tests/test_gpu_families.py FALLBACK_SHAPES with their family settings, and the
# CONVS cases of profiles/conv_dispatch.md section 4: the forward (conv2d concat)
# is pinned too, most of these cases are about a forward kernel.
# conv_igemm_kernel<0> is ST_CONCAT, <2> ST_PARTIAL.
ROUTES.update({
    "igemm2_1ff": (("igemm_x6", 0), (2, 3, 1168, 2, 1, 64, 0, 0), fallback(
        ["conv_igemm2_kernel<1, false, false>"],
        [TRANSPOSE, "conv_igemm2_kernel<2, false, true>", COL2IM], WX6)),
    "igemm_concat": (("igemm_x6", 0), (3, 4, 10, 3, 3, 10, 1, 1), fallback(
        ["conv_igemm_kernel<0>"], [FLIP, "conv_igemm_kernel<0>"], ["conv_wgrad_kernel", RED])),
    "igemm2_1tt": (("igemm_x6", 0), (6, 7, 9, 3, 3, 64, 1, 1), fallback(
        ["conv_igemm2_kernel<1, true, true>"],
        [FLIP, "conv_igemm_kernel<2>", "reduce_pass1", "conv_splitk_reduce_kernel"], WX6P)),
    "igemm2_1ft": (("igemm_x6", 0), (1, 4, 40, 1, 3, 64, 0, 0), fallback(
        ["conv_igemm2_kernel<1, false, true>"],
        [TRANSPOSE, "conv_igemm2_kernel<2, false, true>", COL2IM], WX6)),
    "wgrad2_2t": (("wgrad_x6", 0), (7, 8, 16, 3, 3, 128, 1, 1), fallback(
        [IG_X6_128P], [FLIP, IG_X6_128P], ["conv_wgrad2_kernel<2, true>", RED])),
    "wgrad2_1t": (("wgrad_x6", 0), (4, 4, 32, 3, 3, 128, 1, 1), fallback(
        [IG_X6_128P], [FLIP, IG_X6_128P], ["conv_wgrad2_kernel<1, true>", RED])),
    "wgrad2_3f": (("wgrad_x6", 0), (11, 11, 64, 4, 3, 256, 0, 0), fallback(
        [IG_X6_256], [TRANSPOSE, IG_X6_256, COL2IM_PLANE], ["conv_wgrad2_kernel<3, false>", RED])),
    "wgrad2_2f": (("wgrad_x6", 0), (9, 10, 5, 3, 5, 96, 0, 0), fallback(
        [IG_X6_128], [TRANSPOSE, IG_X6_128, COL2IM_PLANE], ["conv_wgrad2_kernel<2, false>", RED])),
    "wgrad_frame2_P9": (("bwd_x6", 0), (4, 4, 2, 2, 2, 160, 0, 0), fallback(
        [IG_X6_256], [FLIP, "conv_direct_smallg_kernel<2>"], WF2)),
    "igemm2_2ff": (("igemm_x6", 0), (2, 3, 1168, 2, 1, 128, 0, 0), fallback(
        ["conv_igemm2_kernel<2, false, false>"],
        [TRANSPOSE, "conv_igemm2_kernel<2, false, true>", COL2IM], WX6)),
    "igemm2_1tf": (("igemm_x6", 0), (12, 12, 3, 4, 8, 64, 1, 1), fallback(
        ["conv_igemm2_kernel<1, true, false>"],
        [TRANSPOSE, "conv_fwd_slab_kernel", COL2IM_PLANE], WX6P)),
    "igemm2_2tf": (("igemm_x6", 0), (12, 12, 3, 4, 8, 128, 1, 1), fallback(
        ["conv_igemm2_kernel<2, true, false>"],
        [TRANSPOSE, "conv_igemm2_kernel<2, false, true>", COL2IM_PLANE], WX6P)),
    "fwd_frame_k40": (None, (40, 20, 4, 5, 2, 128, 0, 0), fallback(
        ["conv_fwd_frame_kernel<4>"], [FLIP, "conv_direct_smallg_kernel<4>"], WX6)),
    "wgrad_g16": (None, (6, 5, 4, 3, 3, 16, 1, 1), fallback(
        ["conv_fwd_slab_kernel"], [FLIP, "conv_direct_smallg_kernel<4>"],
        ["conv_wgrad_kernel", RED])),
    "direct_g2": (None, (3, 4, 2, 2, 2, 2, 0, 0), fallback(
        ["conv_direct_smallg_kernel<2>"], [FLIP, "conv_direct_smallg_kernel<2>"], WF1)),
    "dgrad_frame_g64": (None, (10, 6, 2, 4, 4, 64, 0, 0), fallback(
        ["conv_fwd_regs_kernel<2, 3, 0, 2, false>"], ["conv_dgrad_frame_kernel<32>"], WX6)),
    "dgrad_frame_g128": (None, (10, 6, 2, 4, 4, 128, 0, 0), fallback(
        ["conv_fwd_regs_kernel<2, 3, 0, 2, false>"], ["conv_dgrad_frame_kernel<64>"], WX6)),
})


def shape_arg(shape):
    return ",".join(str(v) for v in shape)


def parse(text):
    """[(shape, rows, mis, [(entry, [rc, ...], [kernel, ...]), ...]), ...] of a
    named log: the launches of a call are logged before its result line."""
    out, launches = [], []
    for line in text.splitlines():
        m = re.match(r"shape ((?:-?\d+ ){8})R (\d+) mis (\d)$", line)
        if m:
            out.append((tuple(int(v) for v in m.group(1).split()), int(m.group(2)),
                        int(m.group(3)), []))
            launches = []
            continue
        m = re.match(r"  K (.*) grid \d+,\d+,\d+ block \d+,\d+,\d+ lds \d+$", line)
        if m:
            launches.append(m.group(1))
            continue
        m = re.match(r" (.*) -> (-?\d+(?: -?\d+)*)$", line)
        if m:
            out[-1][3].append((m.group(1), [int(v) for v in m.group(2).split()], launches))
        launches = []  # ws / malloc / memset lines belong to no kernel list
    return out


@pytest.fixture(scope="module")
def logger(tmp_path_factory):
    """The launch logger, built as the header of conv_launch_log.cc says."""
    exe = str(tmp_path_factory.mktemp("launchlog") / "conv_launch_log")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "scripts", "conv_launch_log.cc"), "-o", exe, "-rdynamic",
                    "-ldl"], check=True)
    assert os.path.exists(kcnn.LIB_PATH), "libkcnn.so is not built"

    def run(shapes, family=None, tmp=os.path.dirname(exe)):
        env = {k: v for k, v in os.environ.items() if not k.startswith("KCNN_")}
        if family:
            env[FAMILY_ENV[family[0]]] = str(family[1])
        raw = os.path.join(tmp, "log.raw")
        with open(raw, "w") as f:
            subprocess.run([exe, kcnn.LIB_PATH] + [shape_arg(s) for s in shapes], stdout=f,
                           env=env, check=True)
        named = subprocess.run([sys.executable,
                                os.path.join(ROOT, "scripts", "conv_launch_names.py"), "--short",
                                kcnn.LIB_PATH, raw], capture_output=True, text=True, check=True)
        assert named.stderr.strip() == "unnamed handles: 0", named.stderr
        return parse(named.stdout)
    return run


def routes_of(records, shape):
    """entry -> (return code, kernels) of the first aligned, full-workspace call."""
    rows = shape[8] if len(shape) > 8 else 9
    rec = [r for r in records if r[0] == tuple(shape[:8]) and r[1] == rows and r[2] == 0]
    assert len(rec) == 1, (shape, len(rec))
    got = {}
    for entry, rcs, kernels in rec[0][3]:
        if entry in ENTRIES and entry not in got:
            got[entry] = (rcs[0], kernels)
    return got


@pytest.mark.parametrize("name", list(ROUTES))
def test_route(logger, name):
    family, shape, expect = ROUTES[name]
    got = routes_of(logger([shape], family), shape)
    for entry, kernels in expect.items():
        rc, launched = got[entry]
        assert rc == 0, f"{name} {entry}: returned {rc}"
        assert launched == kernels, f"{name} {entry}"


HIP_ERROR_LAUNCH_FAILURE = 719


def test_sweep_has_no_half_run_route(logger):
    """Over the built-in sweep (every geometry x row count x alignment, with and
    without workspace): no backward entry reports a route that stopped after its
    first filter chunk, and no successful call holds launches of two rungs that
    produce the same output (the fused backward and the frame weight gradient)."""
    records = logger([])
    assert len(records) > 700
    calls = 0
    for shape, rows, mis, entries in records:
        for entry, rcs, kernels in entries:
            if entry.split()[0] not in ("wgrad", "dgrad", "backward"):
                continue
            calls += 1
            where = f"{shape} rows {rows} mis {mis} {entry}"
            assert HIP_ERROR_LAUNCH_FAILURE not in rcs, where
            if rcs[0] != 0:
                continue
            names = {k.split("<")[0] for k in kernels}
            fused = names & {"conv_bwd_frame_kernel", "conv_bwd_dma_kernel", "conv_bwd_x6_kernel",
                             "conv_bwd_x6q_kernel"}
            assert not (fused and "conv_wgrad_frame_kernel" in names), f"{where}: {kernels}"
    assert calls > 5000
