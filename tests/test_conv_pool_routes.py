"""Which kernels the fused conv + pool entry points launch, pinned without a GPU
(test_nnet2_routes.py's counterpart for hipF_conv2d_maxpool[3d],
kcnn_conv2d_maxpool_stats and hipF_conv2d_backward_pooled[3d]).

scripts/conv_launch_log.cc loads libkcnn.so, defines hipLaunchKernel itself and
logs what an entry point launches for the operands of a case (fake device
pointers of the stated alignment).  Every case of tests/conv_pool_cases.py must
launch exactly the kernels it names, with their grid, block and dynamic LDS, so
a GPU case of test_gpu_conv_pool.py cannot go green on another instantiation
than the one it is for; every pooled-path instantiation the library holds must
have a case; and the calls an entry refuses are given here, where nothing can run.
"""
import os
import re
import subprocess
import sys

import pytest

import conv_pool_cases as T
import kcnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")


def parse(text):
    """[(return code, produced, [(kernel, grid, block, lds), ...]), ...], one a case."""
    out, launches = [], None
    for ln in text.splitlines():
        if re.match(r"case \d+ \w+$", ln):
            assert launches is None, "a case without a return code"
            launches = []
            continue
        m = re.match(r"  K (.*) grid (\d+),(\d+),(\d+) block (\d+),(\d+),(\d+) lds (\d+)$", ln)
        if m:
            v = [int(x) for x in m.groups()[1:]]
            launches.append((m.group(1), tuple(v[:3]), tuple(v[3:6]), v[6]))
            continue
        if re.match(r"  (malloc|memset) ", ln):
            continue
        m = re.match(r" rc (-?\d+)(?: produced (\d))?$", ln)
        assert m, f"unexpected line {ln!r}"
        out.append((int(m.group(1)), int(m.group(2) or 0), launches))
        launches = None
    assert launches is None
    return out


@pytest.fixture(scope="module")
def run_cases(tmp_path_factory):
    """cases -> [(return code, produced, launches)]: one logger run per family setting."""
    tmp = str(tmp_path_factory.mktemp("poollog"))
    exe = os.path.join(tmp, "conv_launch_log")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(SCRIPTS, "conv_launch_log.cc"), "-o", exe, "-rdynamic", "-ldl"],
                   check=True)
    assert os.path.exists(kcnn.LIB_PATH), "libkcnn.so is not built"

    def run(cases):
        out = [None] * len(cases)
        groups = {}
        for i, c in enumerate(cases):
            groups.setdefault(tuple(sorted(c["fam"].items())), []).append(i)
        for fam, idx in groups.items():
            env = {k: v for k, v in os.environ.items() if not k.startswith("KCNN_")}
            env.update({T.FAMILY_ENV[k]: str(v) for k, v in fam})
            raw = os.path.join(tmp, "log.raw")
            with open(raw, "w") as f:
                subprocess.run([exe, kcnn.LIB_PATH, "-"],
                               input="".join(T.line(cases[i]) + "\n" for i in idx), stdout=f,
                               env=env, text=True, check=True)
            named = subprocess.run([sys.executable, os.path.join(SCRIPTS, "conv_launch_names.py"),
                                    "--short", kcnn.LIB_PATH, raw], capture_output=True,
                                   text=True, check=True)
            assert named.stderr.strip() == "unnamed handles: 0", named.stderr
            records = parse(named.stdout)
            assert len(records) == len(idx)
            for i, r in zip(idx, records):
                out[i] = r
        return out
    return run


@pytest.fixture(scope="module")
def log(run_cases):
    """name -> (return code, produced, launches) of every case and refusal of the table."""
    cases = T.CASES + T.REFUSALS
    return {c["name"]: r for c, r in zip(cases, run_cases(cases))}


def same_launches(launched, kernels):
    """Names in order; grid, block and LDS wherever the table pins them."""
    if [k[0] for k in launched] != [k[0] for k in kernels]:
        return False
    return all(want[1] is None or got == want for got, want in zip(launched, kernels))


@pytest.mark.parametrize("case", T.CASES, ids=T.name_of)
def test_case_launches_its_kernels(log, case):
    rc, produced, launched = log[case["name"]]
    assert rc == 0, f"returned {rc}"
    assert same_launches(launched, case["kernels"]), (launched, case["kernels"])
    assert produced == case["produced"]
    if case["for_"]:
        assert case["for_"] in [k[0] for k in launched]


@pytest.mark.parametrize("case", T.REFUSALS, ids=T.name_of)
def test_refusal_launches_nothing(log, case):
    rc, produced, launched = log[case["name"]]
    assert rc == case["rc"] and rc in (T.DECLINED, T.HIP_ERROR_INVALID_VALUE)
    assert launched == [] and produced == 0


def test_refusals_cover_the_listed_reasons():
    names = {c["name"] for c in T.REFUSALS}
    assert {"fwd-P385", "fwd-P15", "fwd-window-not-dividing", "bwd-window-not-dividing", "fwd-pc3",
            "bwd-pc3", "bwd-pc2", "bwd-3x1x8", "fwd-mask-stride-short", "bwd-mask-stride-short",
            "bwd-misaligned-dp-lead1", "bwd-misaligned-mask-lead1"} <= names
    for tag in T.REFUSAL_TAGS:
        assert any(tag in c["tags"] for c in T.REFUSALS), tag


# ---- every pooled-path instantiation the dispatch can pick --------------------------------
# From the launchers' ladders, not from the log.
BOOL = ("false", "true")
EXPECTED = set()
# fwd_regs_ks: (KS, AR) f16x3 (2), bf16x6 (1), fp32 (0); fwd_regs: the pool forms
# PC (2 | 4 | 8 compiled in, -3: 3 x 1 x 4 compiled in, -1: a runtime window);
# fwd_regs_launch: the register-pooled-only form, PC 4 at AR 2 alone
FWD_KS_AR = [(1, 2), (2, 2), (1, 1), (2, 1), (4, 0), (8, 0), (12, 0), (16, 0)]
FWD_PC = (2, 4, 8, -1, -3)
EXPECTED |= {f"conv_fwd_regs_kernel<{ks}, 3, {pc}, {ar}, false>" for ks, ar in FWD_KS_AR
             for pc in FWD_PC}
EXPECTED |= {f"conv_fwd_regs_kernel<{ks}, 3, 4, 2, true>" for ks in (1, 2)}
# KCNN_X6N / KCNN_X6M / KCNN_X6P with PCM > 0, KCNN_X6QM / KCNN_X6Q
X6_WIN = [(4, 3), (4, 2), (4, 1), (8, 2), (8, 1)]       # (PCM, PH)
X6_OUT = [("true", "true"), ("false", "true"), ("true", "false")]
EXPECTED |= {f"conv_bwd_x6_kernel<{nch}, {dx}, {wg}, {pcm}, {ph}>" for nch in (1, 2, 3, 4)
             for dx, wg in X6_OUT for pcm, ph in X6_WIN}
EXPECTED |= {f"conv_bwd_x6q_kernel<{nch}, {pcm}, {ph}>" for nch in (2, 3, 4) for pcm, ph in X6_WIN}
# KCNN_BWD3_NCH / KCNN_BWD3 / KCNN_BWD3P with PCM 4 | 8
EXPECTED |= {f"conv_bwd_dma_kernel<{nch}, {dx}, {wg}, {pcm}>" for nch in (1, 2, 3, 4)
             for dx, wg in X6_OUT for pcm in (4, 8)}
# KCNN_IGP / launch_pool / launch_pair / launch_t with POOL 1..3
EXPECTED |= {f"conv_igemm_x6_kernel<{bg}, {pad}, {tab}, {pool}, {f16}>" for bg in (128, 256)
             for pad in BOOL for tab in BOOL for pool in (1, 2, 3) for f16 in BOOL}
EXPECTED |= {f"conv_igemm_fixup_kernel<{bg}, {pool}>" for bg in (128, 256) for pool in (1, 2, 3)}
# kcnn_pool_cols_complete
EXPECTED |= {"pool_colmax_kernel", "pool_count_kernel"}
EXPECTED_COUNTS = {"conv_fwd_regs_kernel": 42, "conv_bwd_x6_kernel": 60, "conv_bwd_x6q_kernel": 15,
                   "conv_bwd_dma_kernel": 24, "conv_igemm_x6_kernel": 48,
                   "conv_igemm_fixup_kernel": 6, "pool_colmax_kernel": 1, "pool_count_kernel": 1}
# No exemption: the host predicates leave every instantiation above reachable.

# the template argument that says "pooled" (0: none) per stem
POOL_ARG = {"conv_fwd_regs_kernel": 2, "conv_bwd_x6_kernel": 3, "conv_bwd_x6q_kernel": 1,
            "conv_bwd_dma_kernel": 3, "conv_igemm_x6_kernel": 3, "conv_igemm_fixup_kernel": 1}


def pooled(name):
    stem, _, args = name.partition("<")
    if stem not in POOL_ARG:
        return stem in ("pool_colmax_kernel", "pool_count_kernel")
    return args.rstrip(">").split(", ")[POOL_ARG[stem]] != "0"


def test_expected_counts():
    assert len(EXPECTED) == 197 and all(pooled(k) for k in EXPECTED)
    for stem, n in EXPECTED_COUNTS.items():
        assert sum(k.split("<")[0] == stem for k in EXPECTED) == n, stem


def named_kernels():
    return {k[0] for c in T.CASES for k in c["kernels"] if pooled(k[0])}


def test_every_reachable_instantiation_has_a_case(log):
    launched = {k[0] for c in T.CASES for k in log[c["name"]][2]}
    missing = EXPECTED - named_kernels()
    assert not missing, f"no case for {sorted(missing)}"
    assert EXPECTED - launched == set()
    assert named_kernels() <= EXPECTED, sorted(named_kernels() - EXPECTED)
    # and each is the form some case was written for, not one it passes through
    assert EXPECTED <= {c["for_"] for c in T.CASES} | {"pool_colmax_kernel", "pool_count_kernel"} \
        | {k for k in EXPECTED if k.startswith("conv_igemm_fixup_kernel")}


BWD_STEMS = ("conv_bwd_x6_kernel", "conv_bwd_x6q_kernel", "conv_bwd_dma_kernel")


def test_every_backward_form_runs_under_a_routing_mask(log):
    """All bits set hides a wrong decode and no bit hides everything, so every
    pooled backward instantiation is launched by a case whose mask is the
    forward entry's own or random window bits."""
    real = {k[0] for c in T.select(("bpool", "bpool3d")) if c["mask"] in T.REAL_MASKS
            for k in log[c["name"]][2]}
    forms = {k for k in EXPECTED if k.startswith(BWD_STEMS)}
    assert len(forms) == 99
    assert forms <= real, sorted(forms - real)
    # and for each form such a case was written for it
    assert forms <= {c["for_"] for c in T.CASES if c["mask"] in T.REAL_MASKS}


def test_bitwise_field_is_what_the_logs_say(run_cases, log):
    """`bitwise` (the GPU test compares the fused call with the unfused pair bit
    for bit where it is set) is set exactly where the logged launches of the
    fused call and of hipF_conv2d_backward / hipF_conv2d_dgrad on the same layer
    are the same arithmetic; only the default-family DMA cases are without."""
    cases = T.select(("bpool", "bpool3d"))
    unfused = [T.unfused(c) for c in cases]
    for c, u, (rc, _, launched) in zip(cases, unfused, run_cases(unfused)):
        fused = log[c["name"]][2]
        same = rc == 0 and T.arithmetic(launched) == T.arithmetic(fused)
        assert c["bitwise"] == same, (c["name"], launched, fused)
        assert rc == 0 and same_launches(launched, T.model(u)[0]), c["name"]
    assert sorted(c["name"] for c in cases if not c["bitwise"]) == [
        "bwd-default-20x20-both-1x1x4", "bwd-default-20x20-nogw-1x1x4",
        "bwd-default-40x10-both-1x1x4", "bwd-default-40x10-nogw-1x1x4"]
    assert not any(c["bitwise"] for c in T.CASES if c["entry"] not in ("bpool", "bpool3d"))


def test_expected_set_is_what_the_library_holds():
    """The pooled instantiations of these templates that libkcnn.so was built with
    are the enumeration: one added to a ladder shows up here."""
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "-t", "-C", kcnn.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    stems = {k.split("<")[0] for k in EXPECTED}
    held = set()
    for m in re.finditer(r"__device_stub__([A-Za-z0-9_]+)(<[^(]*>)?\(", out):
        name = m.group(1) + (m.group(2) or "")
        if m.group(1) in stems and pooled(name):
            held.add(name)
    assert held == EXPECTED, (sorted(held - EXPECTED), sorted(EXPECTED - held))


def test_both_sides_of_every_cut():
    tags = {t for c in T.CASES for t in c["tags"]}
    missing = [t for t in T.CUT_TAGS if t not in tags]
    assert not missing, missing


def test_cut_cases_have_the_geometry_they_are_named_for():
    """The tags are claims about a case; check them against its own fields."""
    for c in T.CASES:
        g = T.Geom(c["shape"], c["rows"])
        for t in c["tags"]:
            m = re.match(r"fwd ar (\d) Kdim (\d+)$", t)
            if m:
                assert c["fam"]["fwd_x6"] == int(m.group(1)) and g.Kdim == int(m.group(2))
            m = re.match(r"(?:fwd|x6q|dma|fwd rp) P (\d+)$", t)
            if m:
                assert g.P == int(m.group(1)), (c["name"], g.P)
            m = re.match(r"(?:fwd|bwd) G (\d+)", t)
            if m:
                assert g.G == int(m.group(1))
            m = re.match(r"(?:fwd|bwd) rows (\d+)$", t)
            if m:
                assert g.R == int(m.group(1))
            if t == "fwd rows > grid":
                assert g.R > c["kernels"][0][1][0]
            if t == "fwd rp":
                assert c["outs"] == "noY" and g.G == 128 and 353 <= g.P <= 384
            if t == "fwd padded":
                assert g.padded and c["fam"] == {}
            if t in ("fwd pitched", "bwd pitched", "ig pitched"):
                need = ("x", "w", "p", "m") + (("y",) if c["entry"] in T.FORWARDS else ("dx", "gw"))
                assert all(T.op(c, n)[2] > T.op(c, n)[1] for n in need)
            if t in ("fwd mask stride", "bwd mask stride"):
                assert T.op(c, "m")[2] > T.op(c, "m")[1]
            if t == "fwd unaligned":
                assert T.op(c, "y")[3] % 4 and T.op(c, "p")[3] % 4
            if t == "bwd misaligned dma":
                assert not (T.aligned16(*T.op(c, "p")[2:]) and T.aligned16(*T.op(c, "m")[2:]))
            if t == "default dma":
                assert c["fam"] == {}
    by = {c["name"]: c for c in T.CASES}
    # 4097 rows: two ranges, each of 256 workgroups, on the same geometry thrice
    assert len({by[n]["shape"][:5] for n in ("bwd-rows4097-x6", "bwd-rows4097-x6q",
                                             "bwd-rows4097-unpooled")}) == 1
    # the mask sources and data kinds each have backward and forward cases
    assert {c["mask"] for c in T.select(T.BACKWARDS)} == set(T.MASKS)
    assert {"randn", "ties", "special", "spread", "reject"} <= {c["data"] for c in T.CASES}
    special = {T.fwd_pc_form(c["win"]) for c in T.CASES
               if c["data"] == "special" and c["outs"] == "Y"}
    assert special == {2, 4, 8, -1, -3}
    assert any(c["data"] == "special" and "fwd rp" in c["tags"] for c in T.CASES)


# ---- the stacks of test_gpu_nnet.py: the kernel a comment names, asserted -------------------
F, X6Q, IG = "conv_fwd_regs_kernel", "conv_bwd_x6q_kernel", "conv_igemm_x6_kernel"
# name: (the forward's kernels, the pooled backward's or None where it declines)
STACK_KERNELS = {
    "G40_pc4": ([f"{F}<1, 3, 4, 2, false>"], None),          # G no multiple of 32: unfused
    "G128_P300": ([f"{F}<1, 3, 4, 2, false>"], [f"{X6Q}<4, 4, 1>", T.RED]),
    "G128_P352": ([f"{F}<2, 3, 4, 2, false>"], [f"{X6Q}<4, 4, 1>", T.RED]),
    "c5_P1_3x1x4": ([f"{F}<12, 3, -3, 0, false>"] * 2, [f"{X6Q}<4, 4, 3>", T.RED] * 2),
    "halfB_G64_pc8": ([f"{F}<1, 3, 8, 2, false>"], [f"{X6Q}<2, 8, 1>", T.RED]),
    "halfB_G96_2x1x4": ([f"{F}<1, 3, -1, 2, false>"], [f"{X6Q}<3, 4, 2>", T.RED]),
    "long_2x1x4_pad": ([f"{IG}<256, true, true, 1, false>"], None),
    "long_1x2x1": ([f"{IG}<128, false, true, 2, false>"], None),
    "long_2x1x2_G96": ([f"{IG}<128, false, true, 3, false>"], None),
}


def test_stacks_reach_the_kernels_their_comments_name(run_cases):
    from test_gpu_nnet import STACKS
    cases, want = [], []
    for name, (fwd, bwd) in STACK_KERNELS.items():
        s = STACKS[name]
        shape = s[:6] + s[8:10]
        win = (s[10], s[11], s[6]) if len(s) > 10 else (1, 1, s[6])
        chan = win[:2] == (1, 1)
        for outs in ("Y", "noY"):
            cases.append(T.make(f"{name} {outs}", "maxpool" if chan else "maxpool3d", shape, win,
                                outs, rows=37))
            want.append((0, fwd))
        if win[1] == 1:
            cases.append(T.make(f"{name} bwd", "bpool" if chan else "bpool3d", shape, win, "both",
                                rows=37))
            want.append((0, bwd) if bwd else (T.DECLINED, []))
    for c, (rc, _, launched), (want_rc, names) in zip(cases, run_cases(cases), want):
        assert rc == want_rc, c["name"]
        assert [k[0] for k in launched] == names, c["name"]
        model = T.model(c)[0]                     # and the table's model agrees, geometry included
        assert same_launches(launched, model or []), c["name"]
