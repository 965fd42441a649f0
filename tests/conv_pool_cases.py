"""The one table of direct cases of the fused conv + pool entry points: shapes,
layouts, family settings, data kinds and the kernels each case is for.

tests/test_conv_pool_routes.py runs every case through scripts/conv_launch_log.cc
on the CPU and asserts that it launches exactly `kernels`;
tests/test_gpu_conv_pool.py runs the same cases on the GPU against the oracle,
so a case that is green there ran the kernel it names.

A case: name, entry (the logger's word for the C entry point), shape (H, W, C,
kh, kw, G, pad_h, pad_w), rows, win (ph, pw, pc), outs ("Y" | "noY" for a
forward, "both" | "nodx" | "nogw" for a backward), lay {operand: (stride,
lead)} for the operands that are not dense (x, w, y, p, m, dx, gw; stride and
lead in the operand's own elements), fam {family: value} (the others at their
defaults), data (the kind of values, test_gpu_conv_pool.py), mask (a backward's
mask source), for_ (the instantiation the case was written for, from the loop
that made it), kernels [(name as conv_launch_names.py --short prints it, grid,
block, dynamic LDS bytes), ...] from the model of the launchers below, rc and
tags (what the cut and path tests look for).  A kernel whose grid is None is
pinned by name alone: the f16x3 implicit GEMM's statistics prologue, kernels
of the matrix layer with cases of their own.
"""
HIP_ERROR_INVALID_VALUE = 1
DECLINED = -1

FORWARDS = ("maxpool", "maxpool_stats", "maxpool_stats0", "maxpool3d")
BACKWARDS = ("bpool", "bpool3d", "backward", "dgrad")
FAMILY_DEFAULT = {"fwd_x6": 2, "bwd_x6": 1, "igemm_x6": 2}
FAMILY_ENV = {"fwd_x6": "KCNN_FWD_X6", "bwd_x6": "KCNN_BWD_X6", "igemm_x6": "KCNN_IGEMM_X6"}
RED = "reduce_splits_kernel"


def b(flag):
    return "true" if flag else "false"


def ceil(a, b_):
    return -(-a // b_)


def round4(n):
    return (n + 3) & ~3


def K(name, grid, block=256, lds=0):
    return (name, (grid, 1, 1) if isinstance(grid, int) else tuple(grid), (block, 1, 1), lds)


class Geom:
    def __init__(self, shape, rows):
        (self.H, self.W, self.C, self.kh, self.kw, self.G, self.pad_h, self.pad_w) = shape
        self.R = rows
        self.oh = self.H + 2 * self.pad_h - self.kh + 1
        self.ow = self.W + 2 * self.pad_w - self.kw + 1
        self.P = self.oh * self.ow
        self.Kdim = self.kh * self.kw * self.C
        self.CHW = self.C * self.H * self.W
        self.CHWp = self.C * (self.H + 2 * self.pad_h) * (self.W + 2 * self.pad_w)
        self.padded = self.pad_h > 0 or self.pad_w > 0


# ---- the launchers, modelled (cnsl-conv-frame.hip, cnsl-conv-frame-bwd.hip, cnsl-conv-x6.hip,
# cnsl-conv-igemm-x6.hip) --
FRAME_LDS_MAX = 96 * 1024
BIG_LDS_MAX = 160 * 1024


def aligned16(stride, lead):
    return stride % 4 == 0 and lead % 4 == 0


def filter_chunks(G):
    """for_filter_chunks: 128 filters at a time when G is past 128 in whole slabs."""
    if G > 128 and G % 32 == 0:
        return [min(128, G - g0) for g0 in range(0, G, 128)]
    return [G]


def fwd_regs_lds(g, G):
    if g.Kdim > 32 or G > 128 or g.P < 16 or g.P > 384 or g.CHW > 2048:
        return 0
    lds = round4(32 * g.P) * 4 + 160 * 4 + 32 * 8 + g.CHW * 4 + 8 * 4
    return lds if lds <= FRAME_LDS_MAX else 0


def fwd_arith(g, use):
    if not use or g.padded or g.G > 128:
        return 0
    if use == 2:
        return 2 if g.Kdim <= 32 else 0
    return 1 if g.Kdim <= 31 else 0


def fwd_ks(g, ar):
    if ar == 2:
        return 1 if g.Kdim <= 16 else 2
    if ar == 1:
        return 1 if g.Kdim < 16 else 2
    ksn = (g.Kdim + 1) // 2
    return 4 if ksn <= 4 else 8 if ksn <= 8 else 12 if ksn <= 12 else 16


def fwd_pc_form(win):
    ph, pw, pc = win
    if ph > 1 or pw > 1:
        return -3 if (ph, pw, pc) == (3, 1, 4) else -1
    return pc


def fwd_pool_kernels(g, win, y_stored, fam, stats_room=False):
    """kcnn_conv_fwd_frame_pool: (launches, produced) or None when it declines."""
    ph, pw, pc = win
    win3 = ph > 1 or pw > 1
    if win3:
        if pc < 1 or 32 % pc or ph * pw * pc > 16 or g.oh % ph or g.ow % pw:
            return None
    elif pc not in (2, 4, 8):
        return None
    if g.G % pc:
        return None
    chunks = filter_chunks(g.G)
    out, produced = [], 0
    for G in chunks:
        lds = fwd_regs_lds(g, G)
        if lds == 0:
            return None
        ar = fwd_arith(g, fam["fwd_x6"])
        grid = min(g.R, 256 * (2 if ar else (3 if lds * 3 <= BIG_LDS_MAX else 2)))
        rp = (not y_stored and pc == 4 and not win3 and G == 128 and ceil(g.P, 32) == 12 and
              ar == 2 and lds + 32 <= FRAME_LDS_MAX)
        form = f"conv_fwd_regs_kernel<{fwd_ks(g, ar)}, 3, {fwd_pc_form(win)}, {ar}, {b(rp)}>"
        out.append(K(form, grid, 256, lds + (32 if rp else 0)))
        npool = G // pc * g.P
        if rp and stats_room and len(chunks) == 1 and grid * 256 >= npool:
            ncq = npool // 4 if npool % 4 == 0 else npool
            out.append(K("pool_colmax_kernel", (ceil(ncq, 256), ceil(grid, 32), 1)))
            out.append(K("pool_count_kernel", min(g.R, 256)))
            produced = 1
    return out, produced


IG_IMG = {False: 2 * 3 * 384 * 64, True: 2 * 2 * 384 * 64}
IG_AUX = 384 * 8
IG_F16_PROLOGUE = ["stats_kernel", "stats_finalize_kernel", "stats_count_kernel",
                   "conv_w_presplit_kernel"]


def igemm_tab_bytes(g):
    KT = ceil(g.Kdim, 32) * 32
    tb = KT * 4 + (KT if g.padded else 0)
    return tb if IG_IMG[False] + tb <= BIG_LDS_MAX else 0


def igemm_pool_kernels(g, win, fam):
    """kcnn_conv_igemm_x6_pool behind hipF_conv2d_maxpool3d's unfused_is_igemm."""
    ph, pw, pc = win
    if (g.Kdim <= 64 and g.P >= 16) or g.G <= 8:   # in_frame_range, use_direct
        return None
    ok = (ph == 2 and pw == 1 and g.oh % 2 == 0) or (ph == 1 and pw == 2 and g.oh == 1 and
                                                      g.ow % 2 == 0)
    if not ok or pc not in (1, 2, 4) or g.G % pc:
        return None
    if not fam["igemm_x6"] or (g.padded and g.kh * g.kw > 31):
        return None
    BG = 128 if g.G <= 128 else 256
    blocks = ceil(g.G, BG) * ceil(g.R * g.P, 384 - BG)
    f16 = fam["igemm_x6"] == 3 or (fam["igemm_x6"] == 2 and
                                   2.0 * g.R * g.P * g.G * g.Kdim >= 2.0 ** 34)
    tab = igemm_tab_bytes(g)
    pool = {4: 1, 1: 2, 2: 3}[pc]
    lds = IG_IMG[f16] + tab + (IG_AUX if f16 else 0)
    main = K(f"conv_igemm_x6_kernel<{BG}, {b(g.padded)}, {b(tab > 0)}, {pool}, {b(f16)}>",
             blocks, 512, lds)
    if not f16:
        return [main]
    return ([(n, None, None, None) for n in IG_F16_PROLOGUE] + [main] +
            [K(f"conv_igemm_fixup_kernel<{BG}, {pool}>", min(blocks, 256)),
             K(f"conv_igemm_efix_kernel<{pool}>", 64)])


X6_YPL, X6_WPL, X6_PP, X6_PZ = 32 * 768, 32 * 256, 384, 388


def x6_stage_floats(P, pc, ph):
    return (((32 // pc if pc else 32) * (P // ph) * 4 + 64 + 1023) & ~1023) // 4


def x6_stage_mask_bytes(P, pc, ph):
    return (((32 // pc) * (P // ph) * (2 if ph > 1 else 1) + 32 + 255) & ~255) if pc else 0


def x6_lds(g, dx, pc, ph):
    ZZ = g.Kdim | 1
    return (3 * X6_YPL + (3 * X6_WPL if dx else 0) +
            (round4(g.P * ZZ) * 4 if dx and pc > 0 else 0) + round4(g.CHWp + 1) * 4 + X6_PP * 4 +
            x6_stage_floats(g.P, pc, ph) * 4 + x6_stage_mask_bytes(g.P, pc, ph))


def x6q_lds(g):
    return (3 * X6_YPL + 3 * X6_WPL + g.Kdim * X6_PZ * 4 + round4(g.CHWp + 1) * 8 + X6_PP * 4 +
            round4(g.CHW) * 4)


def bwd_chunk_shape_ok(g, G):
    return g.Kdim <= 31 and G % 32 == 0 and 0 < G <= 128


def x6_eligible(g, G, dx, pc, ph):
    if not bwd_chunk_shape_ok(g, G) or g.Kdim < 1 or g.P < 1 or g.P > X6_PP or g.CHW > 2048:
        return False
    if pc not in (0, 4, 8):
        return False
    if ph < 1 or ph > 3 or (ph > 1 and (pc == 0 or ph * pc > 16 or g.oh % ph)):
        return False
    return x6_lds(g, dx, pc, ph) <= BIG_LDS_MAX


def bwd_dma_lds(g, G):
    buf = ((32 * g.P * 4 + 1023) & ~1023) // 4
    sd = max(2 * buf, 8 * 1024)
    return ((G // 32) * 1024 + sd + ((g.CHWp + 4) & ~3) + ((g.P + 31) & ~31)) * 4


def bwd_kernels(g, pc, ph, dx, gw, fam, dp_aligned=True, mask_aligned=True):
    """kcnn_conv_bwd_frame for dP through a ph x 1 x pc mask (pc 0: dY itself):
    the launches, or None when it declines (then nothing is launched: only the
    first chunk may decline)."""
    if g.G > 128 and (g.G % 32 or g.G * g.P * 4 % 16):
        return None
    out = []
    chunks = filter_chunks(g.G)
    for ci, G in enumerate(chunks):
        if not bwd_chunk_shape_ok(g, G):
            return None
        nch = G // 32
        S, E = min(g.R, 256), (g.Kdim + 1) * G
        red = [K(RED, ceil(E, 64))] if gw else []
        if fam["bwd_x6"] and x6_eligible(g, G, dx, pc, ph):
            if not dp_aligned or (pc and not mask_aligned):
                return None
            nr = ceil(g.R, 4096) if gw else 1
            for c in range(nr):
                rows = g.R * (c + 1) // nr - g.R * c // nr
                Sc = min(rows, 256) if nr > 1 else S
                if dx and gw and pc and G >= 64 and x6q_lds(g) <= BIG_LDS_MAX:
                    out.append(K(f"conv_bwd_x6q_kernel<{nch}, {pc}, {ph}>", Sc, 512, x6q_lds(g)))
                else:
                    out.append(K(f"conv_bwd_x6_kernel<{nch}, {b(dx)}, {b(gw)}, {pc}, {ph}>", Sc,
                                 512, x6_lds(g, dx, pc, ph)))
            out += red
            continue
        if ph != 1 or not (16 <= g.P <= 512):
            return None
        if (pc == 0 and not dp_aligned) or pc not in (0, 4, 8):
            return None
        lds = bwd_dma_lds(g, G)
        zbytes = g.P * (g.Kdim | 1) * 4
        if dx and lds + zbytes <= BIG_LDS_MAX:
            lds += zbytes
        if g.CHW > 2048 or lds > BIG_LDS_MAX:
            return None        # the register-staged kernel takes no pooled call
        out.append(K(f"conv_bwd_dma_kernel<{nch}, {b(dx)}, {b(gw)}, {pc}>", S, 512, lds))
        out += red
    return out


# ---- the table ------------------------------------------------------------------------------
CASES = []
REFUSALS = []
OPERANDS = ("x", "w", "y", "p", "m", "dx", "gw")


def families(c):
    return dict(FAMILY_DEFAULT, **c["fam"])


def pooled_cols(c):
    g = Geom(c["shape"], c["rows"])
    ph, pw, pc = c["win"]
    return g.P * g.G // (ph * pw * pc)


def op_dims(c):
    """operand -> (rows, cols) of the matrices the entry takes."""
    g = Geom(c["shape"], c["rows"])
    return {"x": (g.R, g.CHW), "w": (g.Kdim, g.G), "y": (g.R, g.P * g.G),
            "p": (g.R, pooled_cols(c)), "m": (g.R, pooled_cols(c)), "dx": (g.R, g.CHW),
            "gw": (g.Kdim, g.G)}


def op(c, name):
    """(rows, cols, stride, lead) of an operand, as tests/_pitched.py places it."""
    rows, cols = op_dims(c)[name]
    stride, lead = c["lay"].get(name, (cols, 0))
    return rows, cols, stride, lead


def model(c):
    """(launches, produced) the launchers' model gives the case; launches None:
    the entry declines."""
    g = Geom(c["shape"], c["rows"])
    fam = families(c)
    ph, pw, pc = c["win"]
    entry = c["entry"]
    if entry in FORWARDS:
        y = c["outs"] == "Y"
        if entry == "maxpool3d":
            got = fwd_pool_kernels(g, c["win"], y, fam)
            if got is None:
                ig = igemm_pool_kernels(g, c["win"], fam)
                return ig, 0
            return got
        got = fwd_pool_kernels(g, (1, 1, pc), y, fam, entry == "maxpool_stats")
        return got if got else (None, 0)
    dx, gw = c["outs"] != "nodx", c["outs"] != "nogw"
    if entry in ("backward", "dgrad"):
        return bwd_kernels(g, 0, 1, dx, gw, fam, aligned16(*op(c, "y")[2:])), 0
    _, _, ps, pl = op(c, "p")
    _, _, ms, ml = op(c, "m")
    mbytes = 2 if entry == "bpool3d" else 1
    return bwd_kernels(g, pc, ph, dx, gw, fam, aligned16(ps, pl),
                       (ms * mbytes) % 4 == 0 and (ml * mbytes) % 4 == 0), 0


def arithmetic(kernels):
    """The arithmetic of a backward's launches, by kernel name: the two bf16x6
    kernels give the same bits, the reduction is the same everywhere."""
    out = set()
    for k_ in kernels:
        name = k_ if isinstance(k_, str) else k_[0]
        if name.startswith(("conv_bwd_x6_kernel", "conv_bwd_x6q_kernel")):
            out.add("bf16x6")
        elif name.startswith("conv_bwd_dma_kernel"):
            out.add("fp32 dma")
        elif name != RED:
            out.add(name)
    return out


def unfused(c):
    """The unfused call of a pooled backward case, as a case of its own: dense
    dY through hipF_conv2d_backward, or hipF_conv2d_dgrad when no gW is wanted."""
    assert c["entry"] in ("bpool", "bpool3d")
    return make(c["name"] + " unfused", "dgrad" if c["outs"] == "nogw" else "backward", c["shape"],
                c["win"], c["outs"], rows=c["rows"], fam=c["fam"])


def same_arithmetic_unfused(c):
    """Whether the model gives the unfused pair the fused call's arithmetic (then
    the GPU test compares the two bit for bit; test_conv_pool_routes.py asserts
    this field from the logged launches of both calls)."""
    if c["entry"] not in ("bpool", "bpool3d"):
        return False
    other = model(unfused(c))[0]
    return other is not None and arithmetic(other) == arithmetic(c["kernels"])


def make(name, entry, shape, win, outs, rows=9, fam=None, lay=None, data="randn", mask="fwd",
         for_=None, tags=(), rc=0):
    assert entry in FORWARDS + BACKWARDS and len(shape) == 8 and len(win) == 3
    assert outs in (("Y", "noY") if entry in FORWARDS else ("both", "nodx", "nogw"))
    assert (entry == "dgrad") <= (outs == "nogw") and (entry == "backward") <= (outs != "nogw")
    c = dict(name=name, entry=entry, shape=tuple(shape), rows=rows, win=tuple(win), outs=outs,
             fam=dict(fam or {}), lay=dict(lay or {}), data=data, mask=mask, for_=for_,
             tags=set(tags), rc=rc)
    assert set(c["lay"]) <= set(OPERANDS) and set(c["fam"]) <= set(FAMILY_DEFAULT)
    return c


def case(name, entry, shape, win, outs, **kw):
    c = make(name, entry, shape, win, outs, **kw)
    assert name not in {k["name"] for k in CASES + REFUSALS}, name
    kernels, produced = model(c)
    assert kernels is not None, f"{name}: the model says the entry declines"
    c["kernels"], c["produced"] = kernels, produced
    c["bitwise"] = same_arithmetic_unfused(c)
    if c["for_"]:
        assert c["for_"] in [k[0] for k in kernels], (name, c["for_"], [k[0] for k in kernels])
    CASES.append(c)
    return c


def refuse(name, entry, shape, win, outs, rc, **kw):
    c = make(name, entry, shape, win, outs, rc=rc, **kw)
    assert name not in {k["name"] for k in CASES + REFUSALS}, name
    c["kernels"], c["produced"] = [], 0
    REFUSALS.append(c)
    return c


def line(c):
    """The case as scripts/conv_launch_log.cc reads it."""
    ph, pw, pc = c["win"]
    words = [c["entry"], ",".join(str(v) for v in c["shape"] + (c["rows"],)), f"{ph}x{pw}x{pc}",
             c["outs"]]
    words += [f"{k}={s}:{ld}" for k, (s, ld) in sorted(c["lay"].items())]
    return " ".join(words)


def name_of(c):
    return c["name"]


def select(entries):
    return [c for c in CASES if c["entry"] in entries]


def win_name(win):
    return "x".join(str(v) for v in win)


def pitched(c, names, extra=4):
    """lay entries that give the named operands a pitched 16-byte-aligned stride."""
    d = op_dims(c) if isinstance(c, dict) else c
    return {n: (round4(d[n][1]) + extra, 0) for n in names}


# -- backward: every conv_bwd_x6_kernel / conv_bwd_x6q_kernel / pooled conv_bwd_dma_kernel form
# (8, 5, 1, 3, 2, G): P 24, oh 6 (divisible by 2 and 3), Kdim 6
def small(G):
    return (8, 5, 1, 3, 2, G, 0, 0)


BWD_WINDOWS = [(1, 1, 4), (1, 1, 8), (2, 1, 4), (2, 1, 8), (3, 1, 4)]
OUTS_ARGS = {"both": (True, True), "nodx": (False, True), "nogw": (True, False)}
MASKS = ("fwd", "random", "ones", "zeros")
REAL_MASKS = ("fwd", "random")    # masks under which a wrong routing or a wrong dP read shows

k = 0
for G in (32, 64, 96, 128):
    for outs, (dx, gw) in OUTS_ARGS.items():
        for win in BWD_WINDOWS:
            ph, pw, pc = win
            nch = G // 32
            entry = "bpool" if ph == 1 else "bpool3d"
            if dx and gw and G >= 64:
                form = f"conv_bwd_x6q_kernel<{nch}, {pc}, {ph}>"
            else:
                form = f"conv_bwd_x6_kernel<{nch}, {b(dx)}, {b(gw)}, {pc}, {ph}>"
            # every form under the forward's own mask or random window bits, in
            # turn (all bits and no bit are extra cases below: under those a
            # wrong decode or a wrong dP read can pass); the data kinds go round
            case(f"bwd-G{G}-{outs}-{win_name(win)}", entry, small(G), win, outs, for_=form,
                 mask=REAL_MASKS[k % 2], data="ties" if k % 3 == 2 else "randn")
            k += 1
            if ph == 1:
                case(f"bwd-G{G}-{outs}-{win_name(win)}-dma", entry, small(G), win, outs,
                     fam={"bwd_x6": 0}, mask=REAL_MASKS[(k + 1) % 2],
                     for_=f"conv_bwd_dma_kernel<{nch}, {b(dx)}, {b(gw)}, {pc}>")

# all window bits set, and none (then dX, gW and gb are exact zeros), for either
# mask width on each kernel family and each set of outputs
for nm, G, win, outs, fam in (("x6", 32, (1, 1, 4), "both", {}), ("x6-3x1x4", 96, (3, 1, 4), "nodx", {}),
                              ("x6q-2x1x8", 64, (2, 1, 8), "both", {}),
                              ("x6-2x1x4", 128, (2, 1, 4), "nogw", {}),
                              ("dma", 64, (1, 1, 8), "both", {"bwd_x6": 0}),
                              ("dma-nogw", 96, (1, 1, 4), "nogw", {"bwd_x6": 0}),
                              ("dma-nodx", 32, (1, 1, 4), "nodx", {"bwd_x6": 0})):
    for mask in ("ones", "zeros"):
        case(f"bwd-mask-{mask}-{nm}", "bpool" if win[0] == 1 else "bpool3d", small(G), win, outs,
             fam=fam, mask=mask, tags={f"bwd mask {mask}"})

# conv_bwd_x6_kernel<NCH >= 2, true, true, PCM, PH>: the pipelined kernel's LDS plan
# (x6q_lds: Kdim rows of Z and the map's split parts) is past 160 KB while the
# plain kernel's fits -- big maps under long-ish kernels, default families.
# (20, 15, 5, 3, 2, G): C*H*W 1500, Kdim 30, oh 18, P 252.
BIGMAP_X6 = (20, 15, 5, 3, 2)
for G in (64, 96, 128):
    for win in BWD_WINDOWS:
        ph, pw, pc = win
        case(f"bwd-bigmap-G{G}-{win_name(win)}", "bpool" if ph == 1 else "bpool3d",
             BIGMAP_X6 + (G, 0, 0), win, "both", rows=5,
             for_=f"conv_bwd_x6_kernel<{G // 32}, true, true, {pc}, {ph}>", tags={"x6 past x6q"})

# the default-family routes of the big maps the dispatch document names: the
# gradient's arithmetic depends on whether dX is wanted (DMA fp32 | bf16x6)
for shape, nch in (((20, 20, 5, 3, 2, 128, 0, 0), 4), ((40, 10, 5, 6, 1, 96, 0, 0), 3)):
    tag = f"{shape[0]}x{shape[1]}"
    case(f"bwd-default-{tag}-both-1x1x4", "bpool", shape, (1, 1, 4), "both", rows=5,
         for_=f"conv_bwd_dma_kernel<{nch}, true, true, 4>", tags={"default dma"})
    case(f"bwd-default-{tag}-nogw-1x1x4", "bpool", shape, (1, 1, 4), "nogw", rows=5,
         for_=f"conv_bwd_dma_kernel<{nch}, true, false, 4>", tags={"default dma"})
    case(f"bwd-default-{tag}-nodx-1x1x4", "bpool", shape, (1, 1, 4), "nodx", rows=5,
         for_=f"conv_bwd_x6_kernel<{nch}, false, true, 4, 1>", tags={"default dma"})
    case(f"bwd-default-{tag}-both-1x1x8", "bpool", shape, (1, 1, 8), "both", rows=5,
         for_=f"conv_bwd_x6_kernel<{nch}, true, true, 8, 1>", tags={"x6 past x6q"})
case("bwd-default-32x16-both-1x1x8", "bpool", (32, 16, 4, 7, 1, 128, 0, 0), (1, 1, 8), "both",
     rows=5, for_="conv_bwd_dma_kernel<4, true, true, 8>", tags={"default dma"})

# positions: x6q's B half (P > 256) and its last position; the pooled DMA
# kernel at its least and past the bf16x6 kernels' 384
P_SHAPES = {16: (5, 5, 1, 2, 2), 25: (6, 6, 1, 2, 2), 272: (17, 18, 1, 2, 2),
            352: (17, 23, 1, 2, 2), 384: (17, 25, 1, 2, 2), 385: (36, 12, 1, 2, 2),
            15: (4, 6, 1, 2, 2), 504: (43, 13, 1, 2, 2), 512: (33, 17, 1, 2, 2)}
for P, outs in ((272, "both"), (384, "both")):
    case(f"bwd-P{P}-x6q", "bpool", P_SHAPES[P] + (128, 0, 0), (1, 1, 4), outs, rows=5,
         for_="conv_bwd_x6q_kernel<4, 4, 1>", tags={f"x6q P {P}"})
case("bwd-P16-dma", "bpool", P_SHAPES[16] + (128, 0, 0), (1, 1, 4), "both", fam={"bwd_x6": 0},
     for_="conv_bwd_dma_kernel<4, true, true, 4>", tags={"dma P 16"})
for P, pc in ((385, 4), (504, 8), (512, 4)):
    case(f"bwd-P{P}-dma-pc{pc}", "bpool", P_SHAPES[P] + (128, 0, 0), (1, 1, pc), "both", rows=5,
         for_=f"conv_bwd_dma_kernel<4, true, true, {pc}>", tags={f"dma P {P}", "dma P > 384"})

# filter chunks: the second chunk adds into dX (G 256: 128 + 128, G 160: 128 + 32)
for G, second in ((256, "conv_bwd_x6q_kernel<4, 4, 1>"), (160, "conv_bwd_x6_kernel<1, true, true, 4, 1>")):
    case(f"bwd-G{G}-chunks", "bpool", small(G), (1, 1, 4), "both", for_=second,
         tags={f"bwd G {G}"})
    case(f"bwd-G{G}-chunks-3x1x4", "bpool3d", small(G), (3, 1, 4), "both", tags={f"bwd G {G}"})
    case(f"bwd-G{G}-chunks-dma", "bpool", small(G), (1, 1, 8), "both", fam={"bwd_x6": 0},
         for_=f"conv_bwd_dma_kernel<{(G - 128) // 32}, true, true, 8>", tags={f"bwd G {G}"})

# rows: one frame, more frames than the 256 workgroups, two ranges of the
# bf16x6 gradient (4097 = 2048 + 2049 frames, the second adding into the partials)
case("bwd-rows1", "bpool", small(64), (1, 1, 4), "both", rows=1, tags={"bwd rows 1"})
case("bwd-rows1-dma", "bpool", small(64), (1, 1, 4), "both", rows=1, fam={"bwd_x6": 0},
     tags={"bwd rows 1"})
case("bwd-rows300", "bpool3d", small(64), (2, 1, 4), "both", rows=300, tags={"bwd rows 300"})
case("bwd-rows300-x6", "bpool", small(32), (1, 1, 8), "both", rows=300, tags={"bwd rows 300"})
case("bwd-rows300-dma", "bpool", small(96), (1, 1, 4), "both", rows=300, fam={"bwd_x6": 0},
     tags={"bwd rows 300"})
case("bwd-rows4097-x6", "bpool", small(32), (1, 1, 4), "both", rows=4097,
     for_="conv_bwd_x6_kernel<1, true, true, 4, 1>", tags={"bwd rows 4097"})
case("bwd-rows4097-x6q", "bpool", small(64), (1, 1, 4), "both", rows=4097,
     for_="conv_bwd_x6q_kernel<2, 4, 1>", tags={"bwd rows 4097"})
case("bwd-rows4097-unpooled", "backward", small(32), (1, 1, 4), "both", rows=4097,
     for_="conv_bwd_x6_kernel<1, true, true, 0, 1>", tags={"bwd rows 4097"})
for c in CASES[-3:]:
    assert [k_[1][0] for k_ in c["kernels"]] == [256, 256, ceil(7 * c["shape"][5], 64)]

# layouts: every operand pitched; the mask with mask_stride > cols; dP or the
# mask off 16 / 4 bytes: the bf16x6 kernels decline (REFUSALS), the DMA kernel runs
for nm, entry, G, win, fam in (("x6", "bpool", 32, (1, 1, 4), {}),
                               ("x6q", "bpool3d", 64, (2, 1, 4), {}),
                               ("dma", "bpool", 64, (1, 1, 8), {"bwd_x6": 0})):
    proto = make("proto", entry, small(G), win, "both")
    case(f"bwd-pitched-{nm}", entry, small(G), win, "both", fam=fam,
         lay=pitched(proto, ("x", "w", "p", "m", "dx", "gw")), tags={"bwd pitched"})
    case(f"bwd-mask-stride-{nm}", entry, small(G), win, "both", fam=fam,
         lay={"m": (pooled_cols(proto) + 8, 0)}, tags={"bwd mask stride"})
for nm, lay in (("dp-lead1", {"p": (24 * 64 // 4 + 4, 1)}), ("dp-stride-odd", {"p": (24 * 64 // 4 + 1, 0)}),
                ("mask-lead1", {"m": (24 * 64 // 4 + 4, 1)}),
                ("mask-stride-odd", {"m": (24 * 64 // 4 + 1, 0)})):
    refuse(f"bwd-misaligned-{nm}", "bpool", small(64), (1, 1, 4), "both", DECLINED, lay=lay,
           tags={"bwd misaligned declines"})
    case(f"bwd-misaligned-{nm}-dma", "bpool", small(64), (1, 1, 4), "both", fam={"bwd_x6": 0},
         lay=lay, for_="conv_bwd_dma_kernel<2, true, true, 4>", tags={"bwd misaligned dma"})

refuse("bwd-pc2", "bpool", small(64), (1, 1, 2), "both", DECLINED)
refuse("bwd-pc3", "bpool", small(96), (1, 1, 3), "both", HIP_ERROR_INVALID_VALUE)
refuse("bwd-3x1x8", "bpool3d", small(64), (3, 1, 8), "both", DECLINED)
refuse("bwd-window-not-dividing", "bpool3d", (9, 5, 1, 3, 2, 64, 0, 0), (2, 1, 4), "both",
       HIP_ERROR_INVALID_VALUE)
refuse("bwd-mask-stride-short", "bpool", small(64), (1, 1, 4), "both", HIP_ERROR_INVALID_VALUE,
       lay={"m": (24 * 64 // 4 - 4, 0)})
refuse("bwd-3d-dma-declines", "bpool3d", small(64), (2, 1, 4), "both", DECLINED,
       fam={"bwd_x6": 0})


# -- forward: every pooled conv_fwd_regs_kernel form
def kshape(Kdim, G, pad=0):
    """oh 6, ow 4 (P 24) under a Kdim x 1 kernel over one channel."""
    return (Kdim + 5 - 2 * pad, 4, 1, Kdim, 1, G, pad, 0)


FWD_WINDOWS = {2: (1, 1, 2), 4: (1, 1, 4), 8: (1, 1, 8), -1: (2, 1, 4), -3: (3, 1, 4)}
# Kdim on both sides of every cut of fwd_regs_ks, per arithmetic (family fwd_x6)
FWD_KDIMS = {2: {16: 1, 17: 2}, 1: {15: 1, 16: 2, 31: 2},
             0: {8: 4, 9: 8, 16: 8, 17: 12, 24: 12, 25: 16, 32: 16}}
FWD_CUTS = {2: [16], 1: [15], 0: [8, 16, 24]}     # Kdim <= cut | Kdim > cut
for ar, kdims in FWD_KDIMS.items():
    for Kdim, ks in kdims.items():
        for form, win in FWD_WINDOWS.items():
            entry = "maxpool" if win[0] == 1 else "maxpool3d"
            data = "randn"
            if ar == 2 and Kdim == 17:
                data = "special"       # the data-dependent paths of the f16x3 form
            elif (Kdim + form) % 3 == 0:
                data = "ties"
            case(f"fwd-ar{ar}-K{Kdim}-{win_name(win)}", entry, kshape(Kdim, 32), win, "Y",
                 fam={"fwd_x6": ar}, data=data, tags={f"fwd ar {ar} Kdim {Kdim}"},
                 for_=f"conv_fwd_regs_kernel<{ks}, 3, {form}, {ar}, false>")
# Kdim 32 under fwd_x6 = 1 is past the bf16x6 form: the fp32 one
case("fwd-ar1-K32-falls-to-fp32", "maxpool", kshape(32, 32), (1, 1, 4), "Y", fam={"fwd_x6": 1},
     for_="conv_fwd_regs_kernel<16, 3, 4, 0, false>", tags={"fwd ar 1 Kdim 32"})
# the fp32 form under the default family: a padded map, G > 128
case("fwd-padded-fp32", "maxpool", kshape(9, 32, pad=1), (1, 1, 4), "Y",
     for_="conv_fwd_regs_kernel<8, 3, 4, 0, false>", tags={"fwd padded"})

# positions: the least, an odd count, 11 tiles, the register-pooled form's 12
# tiles (Y NULL, G 128, pc 4: KS 1 and 2) and what the same P takes with Y
# stored, the most; 385 and 15 are REFUSALS
for P in (16, 25, 352, 384):
    case(f"fwd-P{P}", "maxpool", P_SHAPES[P] + (128, 0, 0), (1, 1, 4), "Y", rows=5,
         for_="conv_fwd_regs_kernel<1, 3, 4, 2, false>", tags={f"fwd P {P}"})
RP_SHAPES = {(353, 1): (354, 1, 1, 2, 1), (353, 2): (370, 1, 1, 18, 1),
             (384, 1): (17, 25, 1, 2, 2), (384, 2): (21, 26, 1, 6, 3)}
for (P, ks), s in RP_SHAPES.items():
    case(f"fwd-rp-P{P}-KS{ks}", "maxpool", s + (128, 0, 0), (1, 1, 4), "noY", rows=5,
         data="special" if P == 353 and ks == 2 else "randn",
         for_=f"conv_fwd_regs_kernel<{ks}, 3, 4, 2, true>", tags={f"fwd rp P {P}", "fwd rp"})
    case(f"fwd-rp-P{P}-KS{ks}-Y", "maxpool", s + (128, 0, 0), (1, 1, 4), "Y", rows=5,
         for_=f"conv_fwd_regs_kernel<{ks}, 3, 4, 2, false>", tags={"fwd rp shape, Y stored"})
case("fwd-P352-noY-not-rp", "maxpool", P_SHAPES[352] + (128, 0, 0), (1, 1, 4), "noY", rows=5,
     for_="conv_fwd_regs_kernel<1, 3, 4, 2, false>", tags={"fwd 11 tiles, Y NULL"})
refuse("fwd-P385", "maxpool", P_SHAPES[385] + (128, 0, 0), (1, 1, 4), "Y", DECLINED)
refuse("fwd-P15", "maxpool", P_SHAPES[15] + (128, 0, 0), (1, 1, 4), "Y", DECLINED)

# the statistics entry: the register-pooled form with room for them (and
# without), at KS 1 with P in 353..384 (c2's layer, KS 2 and P 363, is
# test_gpu_pool_stats.py's); rows so that the grid covers the pooled columns
case("fwd-stats-P353-KS1", "maxpool_stats", RP_SHAPES[(353, 1)] + (128, 0, 0), (1, 1, 4), "noY",
     rows=48, for_="pool_colmax_kernel", data="spread", tags={"fwd stats"})
case("fwd-stats-P384-KS2-unaligned-pool", "maxpool_stats", RP_SHAPES[(384, 2)] + (128, 0, 0),
     (1, 1, 4), "noY", rows=50, lay={"p": (384 * 32 + 3, 1)}, for_="pool_count_kernel",
     data="spread", tags={"fwd stats", "fwd stats vec 0"})
case("fwd-stats-no-room", "maxpool_stats0", RP_SHAPES[(353, 1)] + (128, 0, 0), (1, 1, 4), "noY",
     rows=48, for_="conv_fwd_regs_kernel<1, 3, 4, 2, true>", tags={"fwd stats no room"})
case("fwd-stats-Y-stored", "maxpool_stats", RP_SHAPES[(353, 1)] + (128, 0, 0), (1, 1, 4), "Y",
     rows=48, for_="conv_fwd_regs_kernel<1, 3, 4, 2, false>", tags={"fwd stats not rp"})
assert [c["produced"] for c in CASES[-4:]] == [1, 1, 0, 0]

# filters: pooled rows past G (G no multiple of 32), two chunks for either mask
case("fwd-G40-pc4", "maxpool", small(40), (1, 1, 4), "Y", tags={"fwd G 40"})
case("fwd-G24-pc8", "maxpool", small(24), (1, 1, 8), "Y", tags={"fwd G 24"})
for G in (256, 160):
    case(f"fwd-G{G}-1x1x4", "maxpool", small(G), (1, 1, 4), "Y", tags={f"fwd G {G} mask 1"},
         for_="conv_fwd_regs_kernel<4, 3, 4, 0, false>")
    case(f"fwd-G{G}-3x1x4", "maxpool3d", small(G), (3, 1, 4), "Y", tags={f"fwd G {G} mask 2"},
         for_="conv_fwd_regs_kernel<4, 3, -3, 0, false>", data="ties")

# runtime windows: with a width, and pc 1, 2, 8 (pc 16 leaves no room for a
# window: ph * pw * pc <= 16, a REFUSAL)
for win in ((1, 2, 1), (2, 2, 2), (2, 1, 1), (2, 1, 2), (2, 1, 8), (1, 2, 8), (3, 2, 2)):
    case(f"fwd-window-{win_name(win)}", "maxpool3d", small(32), win, "Y",
         data="ties" if win[2] == 2 else "randn",
         for_="conv_fwd_regs_kernel<1, 3, -1, 2, false>", tags={f"fwd window {win_name(win)}"})
refuse("fwd-window-2x1x16", "maxpool3d", small(32), (2, 1, 16), "Y", DECLINED)
refuse("fwd-pc3", "maxpool", small(96), (1, 1, 3), "Y", DECLINED)
refuse("fwd-window-not-dividing", "maxpool3d", small(64), (4, 1, 4), "Y", DECLINED)
refuse("fwd-mask-stride-short", "maxpool", small(64), (1, 1, 4), "Y", HIP_ERROR_INVALID_VALUE,
       lay={"m": (24 * 64 // 4 - 1, 0)})

# rows: one, more than a backward's workgroups, more than the forward's grid
# (512 workgroups for the matrix-core forms, 768 for the fp32 one at this LDS)
case("fwd-rows1", "maxpool", small(64), (1, 1, 4), "Y", rows=1, tags={"fwd rows 1"})
case("fwd-rows300", "maxpool3d", small(64), (3, 1, 4), "Y", rows=300, tags={"fwd rows 300"})
case("fwd-rows600-past-grid", "maxpool", P_SHAPES[16] + (32, 0, 0), (1, 1, 4), "Y", rows=600,
     tags={"fwd rows > grid"})
case("fwd-rows800-past-grid-fp32", "maxpool", P_SHAPES[16] + (32, 0, 0), (1, 1, 8), "Y", rows=800,
     fam={"fwd_x6": 0}, tags={"fwd rows > grid"})
assert CASES[-2]["kernels"][0][1][0] == 512 and CASES[-1]["kernels"][0][1][0] == 768

# layouts: every operand pitched; the mask with mask_stride > cols; Y and the
# pooled output only 4-byte aligned (vec_ok 0)
for nm, entry, win in (("1x1x4", "maxpool", (1, 1, 4)), ("2x1x4", "maxpool3d", (2, 1, 4))):
    proto = make("proto", entry, small(64), win, "Y")
    case(f"fwd-pitched-{nm}", entry, small(64), win, "Y",
         lay=pitched(proto, ("x", "w", "y", "p", "m")), tags={"fwd pitched"})
    case(f"fwd-mask-stride-{nm}", entry, small(64), win, "Y",
         lay={"m": (pooled_cols(proto) + 5, 0)}, tags={"fwd mask stride"})
    case(f"fwd-unaligned-{nm}", entry, small(64), win, "Y",
         lay={"y": (24 * 64 + 1, 1), "p": (pooled_cols(proto) + 3, 1),
              "m": (pooled_cols(proto) + 1, 1), "x": (41, 1), "w": (65, 1)},
         tags={"fwd unaligned"})


# -- the implicit GEMM's pooled epilogue (kcnn_conv_igemm_x6_pool): every conv_igemm_x6_kernel
# <BG, PADDED, TAB, POOL 1..3, F16> and conv_igemm_fixup_kernel<BG, POOL>
def ig_shape(padded, tab, G):
    """oh 2, ow 2 under a long kernel; TAB false: the tap table (4 B a tap, 5
    padded, of Kdim rounded up to 32) does not fit in the 16 KB beside the images."""
    if padded:
        return (2, 2, 12 if tab else 364, 3, 3, G, 1, 1)
    return (3, 2, 40 if tab else 2049, 2, 1, G, 0, 0)


IG_POOL = {1: 4, 2: 1, 3: 2}      # POOL -> pc
for BG, G in ((128, 64), (256, 160)):
    for padded in (False, True):
        for tab in (True, False):
            for pool, pc in IG_POOL.items():
                for f16 in (False, True):
                    shape = ig_shape(padded, tab, G)
                    nm = f"ig-BG{BG}-{'pad' if padded else 'nopad'}-{'tab' if tab else 'notab'}" \
                         f"-pool{pool}-{'f16' if f16 else 'bf16'}"
                    case(nm, "maxpool3d", shape, (2, 1, pc), "Y", rows=3 if not tab else 9,
                         fam={"igemm_x6": 3 if f16 else 1},
                         data="reject" if f16 and tab else "randn",
                         for_=f"conv_igemm_x6_kernel<{BG}, {b(padded)}, {b(tab)}, {pool}, {b(f16)}>",
                         tags={f"ig BG {BG}", f"ig POOL {pool}", f"ig tab {tab}", f"ig f16 {f16}",
                               f"ig padded {padded}", "ig 2x1"})
# the 1 x 2 window (oh 1, ow even), Y NULL, G not a multiple of the tile
case("ig-1x2x4", "maxpool3d", (1, 4, 40, 1, 3, 64, 0, 0), (1, 2, 4), "Y", tags={"ig 1x2"},
     fam={"igemm_x6": 1}, for_="conv_igemm_x6_kernel<128, false, true, 1, false>")
case("ig-1x2x2-f16-noY", "maxpool3d", (1, 4, 40, 1, 3, 96, 0, 0), (1, 2, 2), "noY",
     tags={"ig 1x2"}, fam={"igemm_x6": 3}, data="reject",
     for_="conv_igemm_x6_kernel<128, false, true, 3, true>")
case("ig-pitched", "maxpool3d", ig_shape(False, True, 64), (2, 1, 4), "Y", fam={"igemm_x6": 1},
     lay={"x": (244, 0), "w": (68, 0), "y": (260, 0), "p": (36, 0), "m": (37, 1)},
     tags={"ig pitched"})
refuse("ig-frame-range-declines", "maxpool3d", (8, 5, 10, 3, 2, 64, 0, 0), (2, 1, 4), "Y",
       DECLINED)     # Kdim 60 > 32 but <= 64 with P >= 16: the frame kernels' range
refuse("ig-pc8", "maxpool3d", ig_shape(False, True, 64), (2, 1, 8), "Y", DECLINED)
refuse("ig-family-off", "maxpool3d", ig_shape(False, True, 64), (2, 1, 4), "Y", DECLINED,
       fam={"igemm_x6": 0})

# ---- both sides of every cut, by tag (test_conv_pool_routes.py asserts them present) ---------
CUT_TAGS = (
    [f"fwd ar {ar} Kdim {kd}" for ar, cuts in FWD_CUTS.items() for c_ in cuts
     for kd in (c_, c_ + 1)] +
    ["fwd ar 1 Kdim 31", "fwd ar 1 Kdim 32", "fwd padded"] +
    [f"fwd P {P}" for P in (16, 25, 352, 384)] +
    ["fwd rp P 353", "fwd rp P 384", "fwd rp shape, Y stored", "fwd 11 tiles, Y NULL",
     "fwd G 40", "fwd G 24", "fwd G 256 mask 1", "fwd G 256 mask 2", "fwd G 160 mask 1",
     "fwd G 160 mask 2", "fwd window 1x2x1", "fwd window 2x2x2", "fwd window 2x1x1",
     "fwd window 2x1x2", "fwd window 2x1x8", "fwd rows 1", "fwd rows 300", "fwd rows > grid",
     "fwd pitched", "fwd mask stride", "fwd unaligned", "fwd stats", "fwd stats vec 0",
     "fwd stats no room", "fwd stats not rp",
     "x6q P 272", "x6q P 384", "dma P 16", "dma P 385", "dma P 504", "dma P 512", "bwd G 256",
     "bwd G 160", "default dma", "x6 past x6q", "bwd rows 1", "bwd rows 300", "bwd rows 4097",
     "bwd pitched", "bwd mask stride", "bwd misaligned dma", "bwd mask ones", "bwd mask zeros"] +
    [f"ig {k_} {v}" for k_, vs in (("BG", (128, 256)), ("POOL", (1, 2, 3)),
                                   ("tab", (True, False)), ("f16", (True, False)),
                                   ("padded", (True, False))) for v in vs] +
    ["ig 2x1", "ig 1x2", "ig pitched"])
REFUSAL_TAGS = ["bwd misaligned declines"]
