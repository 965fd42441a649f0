"""The one table of direct kn_* launcher cases (src/nnet2/): shapes, layouts and
the kernel each case is for.

tests/test_nnet2_routes.py runs every case through scripts/nnet2_launch_log.cc
on the CPU and asserts that it launches exactly `kernels`; the GPU tests
(test_gpu_nnet2_kernels.py, test_gpu_timemap_kernels.py and the row-kernel
tests of test_gpu_nnet2_loss.py, test_gpu_normalize.py, test_gpu_compute_prob.py
and test_gpu_compute.py) take their shapes from here, so a case that is green
on the GPU ran the kernel it names.

A case: name, launcher, ops [(rows, cols, stride, lead), ...] (lead: floats
between an aligned address and the base; -1: NULL), args (the integers after
the operands, as nnet2_launch_log.cc reads them), kernels [(template name as
conv_launch_names.py --short prints it, grid, block, dynamic LDS bytes), ...],
and what a GPU test needs beside the shape.  REFUSALS are argument lists a
launcher must answer with hipErrorInvalidValue without launching; they never
go to a GPU.
"""
import ctypes

LAUNCHERS = ["kn_relu_prop", "kn_relu_backprop", "kn_splice_prop", "kn_splice_backprop",
             "kn_dvec_update", "kn_softmax_prop", "kn_softmax_backprop",
             "kn_comp_objf_and_deriv", "kn_softmax_xent_backprop", "kn_objf_accuracy",
             "kn_softmax_objf_accuracy", "kn_loglikes", "kn_softmax_loglikes",
             "kn_normalize_prop", "kn_normalize_backprop", "kn_timemap_epilogue",
             "kn_timemap_gather"]
HIP_ERROR_INVALID_VALUE = 1


def ceil(a, b):
    return -(-a // b)


def K(name, grid, block=256, lds=0):
    grid = tuple(grid) if isinstance(grid, (tuple, list)) else (grid,)
    return (name, grid + (1,) * (3 - len(grid)), (block, 1, 1), lds)


def elementwise_grid(rows, cols, cols_per_block):
    """hip-util.h: column blocks x rows, the rows capped at about 8k blocks."""
    cb = ceil(cols, cols_per_block)
    return (cb, min(rows, 8192 // cb + 1, 65535))


def grid_for(n):
    return max(1, min(ceil(n, 256), 256 * 32))


def b(flag):
    return "true" if flag else "false"


CASES = []
REFUSALS = []


def case(name, launcher, ops, args, kernels, **more):
    assert launcher in LAUNCHERS and all(len(o) == 4 for o in ops)
    assert name not in {c["name"] for c in CASES}, name
    CASES.append(dict(name=name, launcher=launcher, ops=[tuple(o) for o in ops], args=list(args),
                      kernels=list(kernels), **more))


def refuse(name, launcher, ops, args):
    REFUSALS.append(dict(name=name, launcher=launcher, ops=[tuple(o) for o in ops],
                         args=list(args), kernels=[]))


def line(c):
    """The case as nnet2_launch_log.cc reads it."""
    vals = [LAUNCHERS.index(c["launcher"])] + [v for o in c["ops"] for v in o] + c["args"]
    return " ".join(str(int(v)) for v in vals)


def select(launcher, gpu=True):
    return [c for c in CASES if c["launcher"] == launcher and (c.get("gpu", True) or not gpu)]


def name_of(c):
    return c["name"]


# ---- row kernels: Softmax family, objective, log-likelihoods, Normalize ------------
# Layouts, by the access width V they leave (row-regs.h lane_width: 4 when every
# base is 16-byte aligned and every stride a multiple of 4, else 2, else 1).
def layout(cols, kind):
    """(stride, lead) of one operand."""
    pitch4 = (cols + 3) // 4 * 4 + 4
    if kind == "v4":                      # a pitched 16-byte stride
        return pitch4, 0
    if kind == "v2":                      # stride = 2 mod 4
        s = cols + (2 - cols) % 4
        return (s if s > cols else s + 4), 0
    if kind == "v1s":                     # an odd stride
        return cols + 1 + cols % 2, 0
    assert kind == "v1l"                  # a base one float in
    return pitch4, 1


WIDTH = {"v4": 4, "v2": 2, "v1s": 1, "v1l": 1}
# per operand; the width is the minimum over the operands ("in4": the first alone at 4)
ROW_LAYOUTS = {"v4": ("v4", "v4", "v4"), "v2": ("v2", "v2", "v2"), "v1s": ("v1s", "v1s", "v1s"),
               "v1l": ("v1l", "v1l", "v1l"), "in4": ("v4", "v2", "v2")}

# values a lane (a thread) holds up to a column count: lane_values, wave_values, block_values
SOFTMAX_TOT = [(256, 4), (1024, 16), (4096, 64)]
NORM_WAVE_TOT = [(256, 4), (1024, 16), (2048, 32), (4096, 64)]
NORM_BLOCK_TOT = [(8192, 32), (16384, 64)]
SOFTMAX_CUTS = [256, 1024, 4096]            # cols <= cut | cols > cut
NORM_CUTS = [256, 1024, 2048, 4096, 8192, 16384]


def tot_of(cols, table):
    for limit, tot in table:
        if cols <= limit:
            return tot
    return None


def softmax_family_kernels(launcher, rows, cols, v, stats):
    tot = tot_of(cols, SOFTMAX_TOT)
    wide = tot is None
    vt = f"{v}, {tot}"
    colsum = []
    if stats:
        if wide:
            colsum.append(K("colsum_part_kernel", (ceil(cols, 256), ceil(rows, 64))))
        colsum.append(K("colsum_final_kernel", ceil(cols, 64), 1024))
    if launcher == "kn_softmax_prop":
        return [K("softmax_prop_block_kernel", rows)] if wide else \
            [K(f"softmax_prop_wave_kernel<{vt}>", ceil(rows, 4))]
    if launcher == "kn_softmax_loglikes":
        return [K("softmax_loglikes_block_kernel", rows)] if wide else \
            [K(f"softmax_loglikes_wave_kernel<{vt}>", ceil(rows, 4))]
    if launcher == "kn_softmax_backprop":
        main = K("softmax_backprop_block_kernel", rows) if wide else \
            K(f"softmax_backprop_wave_kernel<{vt}, {b(stats)}>", ceil(rows, 16))
        return [main] + colsum
    if launcher == "kn_softmax_xent_backprop":
        main = K("softmax_xent_block_kernel", rows) if wide else \
            K(f"softmax_xent_wave_kernel<{vt}, {b(stats)}>", ceil(rows, 16))
        return [main, K("objf_final_kernel", 1, 64)] + colsum
    sm = b(launcher == "kn_softmax_objf_accuracy")
    main = K(f"objf_accuracy_block_kernel<{sm}>", rows) if wide else \
        K(f"objf_accuracy_wave_kernel<{vt}, {sm}>", ceil(rows, 4))
    return [main, K("prob_final_kernel", 1, 64)]


def normalize_kernels(launcher, rows, cols, v, stats):
    which = "prop" if launcher == "kn_normalize_prop" else "backprop"
    tot = tot_of(cols, NORM_WAVE_TOT)
    if tot is not None:
        return [K(f"normalize_{which}_wave_kernel<{v}, {tot}>", ceil(rows, 4))]
    tot = tot_of(cols, NORM_BLOCK_TOT)
    if tot is not None:
        return [K(f"normalize_{which}_block_kernel<{v}, {tot}>", rows)]
    return [K(f"normalize_{which}_reread_kernel", rows)]


# launcher: (operands, takes a stats argument, the kernels)
ROW_LAUNCHERS = {
    "kn_softmax_prop": (2, False, softmax_family_kernels),
    "kn_softmax_backprop": (3, True, softmax_family_kernels),
    "kn_softmax_xent_backprop": (2, True, softmax_family_kernels),
    "kn_objf_accuracy": (1, False, softmax_family_kernels),
    "kn_softmax_objf_accuracy": (1, False, softmax_family_kernels),
    "kn_softmax_loglikes": (2, False, softmax_family_kernels),
    "kn_normalize_prop": (2, False, normalize_kernels),
    "kn_normalize_backprop": (3, False, normalize_kernels),
}
# 1 and 70 rows (70 leaves a block of two rows) at either side of every step in
# the values a lane holds; the wide forms at 5 rows
SOFTMAX_SHAPES = [(r, c) for c in (256, 257, 1024, 1025) for r in (1, 70)]
SOFTMAX_WIDE = [(5, 4096), (5, 4097)]
NORM_SHAPES = [(r, c) for c in (256, 257, 1024, 1025, 2048, 2049, 8192, 8193) for r in (1, 70)]
NORM_WIDE = [(5, 4096), (5, 4097), (3, 16384), (3, 16385)]

for _launcher, (_nops, _has_stats, _kernels) in ROW_LAUNCHERS.items():
    _norm = _launcher.startswith("kn_normalize")
    _shapes = [(s, list(ROW_LAYOUTS)) for s in (NORM_SHAPES if _norm else SOFTMAX_SHAPES)]
    _shapes += [(s, ["v4", "v2", "v1s"]) for s in (NORM_WIDE if _norm else SOFTMAX_WIDE)]
    for (_rows, _cols), _layouts in _shapes:
        for _lay in _layouts:
            if _lay == "in4" and _nops == 1:
                continue
            _kinds = ROW_LAYOUTS[_lay][:_nops]
            _v = min(WIDTH[k] for k in _kinds)
            _ops = [(_rows, _cols) + layout(_cols, k) for k in _kinds]
            for _stats in ((0, 1) if _has_stats else (None,)):
                case(f"{_launcher[3:]}-{_rows}x{_cols}-{_lay}" + ("-stats" if _stats else ""),
                     _launcher, _ops, [] if _stats is None else [_stats],
                     _kernels(_launcher, _rows, _cols, _v, bool(_stats)),
                     rows=_rows, cols=_cols, layout=_lay, v=_v, stats=bool(_stats))

# CompObjfAndDeriv and the stored log-likelihoods are element-wise: no V, no TOT
for _rows, _cols, _per_row, _lay in ((70, 257, 5, "v1s"), (1, 1025, 5, "v4"), (70, 256, 1, "v1l")):
    _num = _rows * _per_row
    case(f"comp_objf-{_rows}x{_cols}-{_lay}", "kn_comp_objf_and_deriv",
         [(_rows, _cols) + layout(_cols, _lay)] * 2, [_num],
         [K("comp_objf_kernel", ceil(_num, 256)), K("objf_final_kernel", 1, 64)],
         rows=_rows, cols=_cols, layout=_lay, per_row=_per_row)
for _rows, _cols, _lay in ((70, 257, "v1s"), (5, 1024, "v4")):
    case(f"loglikes-{_rows}x{_cols}-{_lay}", "kn_loglikes",
         [(_rows, _cols) + layout(_cols, _lay)] * 2, [],
         [K("loglikes_kernel", elementwise_grid(_rows, _cols, 256))], gpu=False)

# ---- kn_timemap_gather ------------------------------------------------------------------
# out(r, k + c positions) = map(r + u ext + dilation k, c).  tc: the channels of a
# tile, 256 halved while tc * positions > 8192; VL: 16-byte loads (channels % 4,
# tc % 4, map stride % 4, map base); VS: 16-byte stores (tc % 4, out stride % 4,
# out base).  The map holds ext = dilation (positions - 1) more rows an utterance.
def gather(name, utts, positions, channels, dilation, map_stride, out_stride, out_lead, tc, vl, vs,
           paths):
    rows, ext = sum(utts), dilation * (positions - 1)
    map_rows = rows + len(utts) * ext
    case("gather-" + name, "kn_timemap_gather",
         [(map_rows, channels, map_stride, 0), (rows, channels * positions, out_stride, out_lead)],
         [len(utts), ext, positions, dilation],
         [K(f"timemap_gather_kernel<{b(vl)}, {b(vs)}>", (min(rows, 32768), ceil(channels, tc)),
            256, 4 * (tc * positions + 4))],
         utts=utts, positions=positions, channels=channels, dilation=dilation, ext=ext, tc=tc,
         paths=paths)


gather("a", [5], 3, 8, 1, 12, 28, 0, 256, True, True, ["VL+VS"])
gather("b", [5], 3, 6, 1, 8, 20, 0, 256, False, True, ["VL off"])
gather("b2", [5], 3, 6, 1, 8, 19, 0, 256, False, False, ["VL off, VS off"])
gather("c-stride", [5], 3, 8, 1, 12, 27, 0, 256, True, False, ["VS off: stride"])
gather("c-lead", [5], 3, 8, 1, 12, 28, 1, 256, True, False, ["VS off: lead"])
gather("d", [3], 33, 132, 1, 136, 4360, 0, 128, True, True, ["tc 128", "partial last tile"])
gather("e", [3], 33, 130, 1, 132, 4292, 0, 128, False, True, ["run with a 2-float tail"])
gather("f", [2], 2049, 3, 1, 4, 6150, 0, 2, False, False, ["tc 2"])
gather("g", [2], 8192, 2, 1, 4, 16388, 0, 1, False, False, ["tc 1"])
gather("h", [3], 4, 260, 2, 264, 1044, 0, 256, True, True, ["two tiles at tc 256"])
gather("i", [32770], 2, 1, 1, 2, 3, 0, 256, False, False, ["row stride"])
gather("j", [1, 37, 5], 3, 8, 2, 12, 28, 0, 256, True, True, ["utterances with ext > 0"])

# ---- kn_timemap_epilogue ------------------------------------------------------------------
# ops: in, pooled, relu ((0, 0, 0, -1): absent).  V = 4: pool_channel 1, cols % 4,
# every stride % 4, every base 16-byte aligned.
ABSENT = (0, 0, 0, -1)


def epilogue(name, rows, cols, pool, relu, pw, pc, delta, extra, lead, v, paths, p_rows=None,
             data="random"):
    in_rows = rows + delta * (pw - 1)
    p_rows = rows if p_rows is None else p_rows
    ops = [(in_rows, cols * pc, cols * pc + extra, lead),
           (p_rows, cols, cols + extra, lead) if pool else ABSENT,
           (rows, cols, cols + extra, lead) if relu else ABSENT]
    case("epilogue-" + name, "kn_timemap_epilogue", ops, [rows, pw, pc, delta],
         [K(f"timemap_epilogue_kernel<{v}, {b(pool)}, {b(relu)}>",
            elementwise_grid(rows, cols, 256 * v))],
         rows=rows, cols=cols, pool=pool, relu=relu, pw=pw, pc=pc, delta=delta, paths=paths,
         data=data)


for _v, _extra in ((4, 4), (1, 3)):
    epilogue(f"v{_v}-pool-relu", 5, 8, True, True, 2, 1, 2, _extra, 0, _v, ["both levels"])
    epilogue(f"v{_v}-pool", 5, 8, True, False, 2, 1, 2, _extra, 0, _v, [])
    epilogue(f"v{_v}-relu", 5, 8, False, True, 1, 1, 2, _extra, 0, _v, [])
    epilogue(f"v{_v}-special", 5, 8, True, True, 3, 1, 1, _extra, 0, _v, ["special values"],
             data="special")
    epilogue(f"v{_v}-relu-special", 5, 8, False, True, 1, 1, 1, _extra, 0, _v, ["special values"],
             data="special")
epilogue("lead1", 5, 8, True, True, 2, 1, 2, 4, 1, 1, ["scalar: base"])
epilogue("pc4", 5, 8, True, False, 2, 4, 3, 4, 0, 1, ["pool_channel 4"])
epilogue("pc4-relu", 5, 8, True, True, 2, 4, 3, 4, 0, 1, ["pool_channel 4"])
epilogue("pc4-special", 5, 8, True, True, 3, 4, 1, 4, 0, 1, ["special values"], data="special")
epilogue("1028", 3, 1028, True, True, 2, 1, 1, 4, 0, 4, ["V 4, two column blocks"])
epilogue("257", 3, 257, True, True, 2, 1, 1, 3, 0, 1, ["scalar, two column blocks"])
epilogue("8200-v4", 8200, 4, True, True, 2, 1, 1, 4, 0, 4, ["row stride"])
epilogue("8200-v1", 8200, 3, False, True, 1, 1, 1, 2, 0, 1, ["row stride"])
epilogue("p-rows", 5, 8, True, True, 2, 1, 2, 4, 0, 4, ["p_dim.rows > rows"], p_rows=9)

# ---- kn_relu_prop / kn_relu_backprop ------------------------------------------------------
# the *4 kernels: cols % 4, every stride % 4, every base (and the stats workspace) aligned
RELU_SHAPES = [("3x8", 3, 8, 4, 0, True), ("3x8-stride9", 3, 8, 1, 0, False),
               ("3x8-lead1", 3, 8, 4, 1, False), ("3x7", 3, 7, 1, 0, False),
               ("8200x8", 8200, 8, 4, 0, True), ("8200x5", 8200, 5, 3, 0, False),
               ("2x1028", 2, 1028, 4, 0, True), ("2x257", 2, 257, 3, 0, False)]
for _name, _rows, _cols, _extra, _lead, _vec in RELU_SHAPES:
    _op = (_rows, _cols, _cols + _extra, _lead)
    case("relu_prop-" + _name, "kn_relu_prop", [_op] * 2, [],
         [K("relu_prop4_kernel" if _vec else "relu_prop_kernel",
            elementwise_grid(_rows, _cols, 1024 if _vec else 256))],
         rows=_rows, cols=_cols)
    case("relu_backprop-" + _name, "kn_relu_backprop", [_op] * 3, [0],
         [K("relu_backprop4_kernel" if _vec else "relu_backprop_kernel",
            (ceil(_cols, 256), ceil(_rows, 64)))],
         rows=_rows, cols=_cols, stats=False)
# with statistics: parts of 64 rows; 1 row (three waves of the *4 kernel without
# one), 65 (a part of one row), 1089 (18 parts, past the final kernel's unroll
# of 16); two column blocks
for _rows in (1, 65, 1089):
    for _cols, _extra, _vec in ((260, 4, True), (257, 3, False)):
        _op = (_rows, _cols, _cols + _extra, 0)
        case(f"relu_backprop-stats-{_rows}x{_cols}", "kn_relu_backprop", [_op] * 3, [1],
             [K("relu_backprop4_kernel" if _vec else "relu_backprop_kernel",
                (ceil(_cols, 256), ceil(_rows, 64))),
              K("relu_stats_final_kernel", ceil(_cols, 256))],
             rows=_rows, cols=_cols, stats=True)

# ---- kn_splice_prop / kn_splice_backprop ----------------------------------------------------
def splice(name, num_chunks, in_cs, out_cs, in_first, out_first, dim, const_dim, context,
           in_index, extra, paths):
    ns = len(context)
    geom = [num_chunks, in_cs, out_cs, in_first, out_first, dim, const_dim, ns,
            int(in_index is not None)] + list(context) + list(in_index or [])
    in_cols, out_cols = dim + const_dim, ns * dim + const_dim
    in_op = (num_chunks * in_cs, in_cols, in_cols + extra[0], 0)
    out_op = (num_chunks * out_cs, out_cols, out_cols + extra[1], 0)
    more = dict(num_chunks=num_chunks, in_cs=in_cs, out_cs=out_cs, in_first=in_first,
                out_first=out_first, dim=dim, const_dim=const_dim, context=list(context),
                in_index=in_index, paths=paths)
    case("splice_prop-" + name, "kn_splice_prop", [in_op, out_op], geom,
         [K("splice_prop_kernel", grid_for(out_op[0] * out_cols))], **more)
    case("splice_backprop-" + name, "kn_splice_backprop", [out_op, in_op], geom,
         [K("splice_backprop_kernel", grid_for(in_op[0] * in_cols))], **more)


splice("contiguous", 4, 7, 3, -2, 0, 5, 0, [-2, -1, 0, 1, 2], None, (3, 5), ["pitched"])
splice("const", 4, 7, 3, -2, 0, 8, 3, [-2, -1, 0, 1, 2], None, (3, 5), ["const tail"])
# block c of output row oi reads in-chunk row in_index[c * out_cs + oi]
splice("table", 3, 5, 2, 0, 0, 4, 2, [-3, 0, 4], [3, 1, 0, 4, 2, 0], (3, 5),
       ["table with a const tail", "non-monotone in_index"])
# 2,112,000 elements each way: past the 8192 blocks x 256 that one pass takes
splice("big", 1100, 5, 1, -2, 0, 384, 0, [-2, -1, 0, 1, 2], None, (4, 4), ["grid_for cap"])
assert 1100 * 5 * 384 == 2112000 > 8192 * 256 == 2097152

# ---- kn_dvec_update ------------------------------------------------------------------------------
for _n in (1, 257):
    for _x_null in (0, 1):
        case(f"dvec-{_n}" + ("-nox" if _x_null else ""), "kn_dvec_update", [], [_n, _x_null],
             [K("dvec_update_kernel", ceil(_n, 256))], n=_n, x_null=bool(_x_null))

# ---- nothing to do: return 0, launch nothing ----------------------------------------------------
case("relu_prop-0rows", "kn_relu_prop", [(0, 8, 8, 0)] * 2, [], [], gpu=False)
case("softmax_prop-0cols", "kn_softmax_prop", [(3, 0, 4, 0)] * 2, [], [], gpu=False)
case("normalize_prop-0rows", "kn_normalize_prop", [(0, 8, 8, 0)] * 2, [], [], gpu=False)
case("comp_objf-0", "kn_comp_objf_and_deriv", [(3, 8, 8, 0)] * 2, [0], [], gpu=False)
case("dvec-0", "kn_dvec_update", [], [0, 0], [], gpu=False)

# ---- refusals (hipErrorInvalidValue, nothing launched) ---------------------------------------------
M = (3, 8, 12, 0)
for _l, _n in (("kn_relu_prop", 2), ("kn_softmax_prop", 2), ("kn_softmax_loglikes", 2),
               ("kn_loglikes", 2), ("kn_normalize_prop", 2), ("kn_softmax_xent_backprop", 2),
               ("kn_comp_objf_and_deriv", 2), ("kn_relu_backprop", 3), ("kn_softmax_backprop", 3),
               ("kn_normalize_backprop", 3)):
    _tail = {"kn_relu_backprop": [0], "kn_softmax_backprop": [0], "kn_softmax_xent_backprop": [0],
             "kn_comp_objf_and_deriv": [4]}.get(_l, [])
    for _k in range(_n):  # a shape mismatch at each operand: rows, then columns
        refuse(f"{_l}: rows of operand {_k}", _l, [M if j != _k else (4, 8, 12, 0)
                                                   for j in range(_n)], _tail)
        refuse(f"{_l}: cols of operand {_k}", _l, [M if j != _k else (3, 7, 12, 0)
                                                   for j in range(_n)], _tail)
    if _l in ("kn_relu_prop", "kn_relu_backprop", "kn_comp_objf_and_deriv"):
        continue  # (their headers promise no stride check)
    for _k in range(_n):
        refuse(f"{_l}: stride < cols at operand {_k}", _l,
               [M if j != _k else (3, 8, 7, 0) for j in range(_n)], _tail)
for _l in ("kn_objf_accuracy", "kn_softmax_objf_accuracy"):
    refuse(f"{_l}: stride < cols", _l, [(3, 8, 7, 0)], [])
for _l in ("kn_relu_backprop", "kn_softmax_backprop"):
    refuse(f"{_l}: statistics without a workspace", _l, [M] * 3, [2])
refuse("kn_softmax_xent_backprop: statistics without a workspace", "kn_softmax_xent_backprop",
       [M] * 2, [2])
refuse("kn_comp_objf_and_deriv: num < 0", "kn_comp_objf_and_deriv", [M] * 2, [-1])


def _splice_refusal(name, in_op, out_op, geom):
    refuse("kn_splice_prop: " + name, "kn_splice_prop", [in_op, out_op], geom)
    refuse("kn_splice_backprop: " + name, "kn_splice_backprop", [out_op, in_op], geom)


# the good geometry: 4 chunks of 7 -> 3 rows, dim 5, context -2..2, in_first -2
_IN, _OUT = (28, 5, 8, 0), (12, 25, 28, 0)
_CTX = [-2, -1, 0, 1, 2]
_splice_refusal("no context", _IN, _OUT, [4, 7, 3, -2, 0, 5, 0, 0, 0])
_splice_refusal("65 context slots", (28, 5, 8, 0), (12, 325, 328, 0),
                [4, 7, 3, -2, 0, 5, 0, 65, 0] + [0] * 64)
_splice_refusal("input rows", (27, 5, 8, 0), _OUT, [4, 7, 3, -2, 0, 5, 0, 5, 0] + _CTX)
_splice_refusal("output rows", _IN, (13, 25, 28, 0), [4, 7, 3, -2, 0, 5, 0, 5, 0] + _CTX)
_splice_refusal("input cols", (28, 6, 8, 0), _OUT, [4, 7, 3, -2, 0, 5, 0, 5, 0] + _CTX)
_splice_refusal("output cols", _IN, (12, 26, 28, 0), [4, 7, 3, -2, 0, 5, 0, 5, 0] + _CTX)
_splice_refusal("a contiguous range that starts before the chunk", _IN, _OUT,
                [4, 7, 3, -1, 0, 5, 0, 5, 0] + _CTX)
_splice_refusal("a contiguous range that ends after the chunk", _IN, _OUT,
                [4, 7, 3, -2, 1, 5, 0, 5, 0] + _CTX)
_T_IN, _T_OUT = (15, 6, 9, 0), (6, 14, 19, 0)
_splice_refusal("in_index below the chunk", _T_IN, _T_OUT,
                [3, 5, 2, 0, 0, 4, 2, 3, 1, -3, 0, 4] + [3, 1, 0, -1, 2, 0])
_splice_refusal("in_index past the chunk", _T_IN, _T_OUT,
                [3, 5, 2, 0, 0, 4, 2, 3, 1, -3, 0, 4] + [3, 1, 0, 5, 2, 0])
_splice_refusal("a table of more than 1024 entries", (1025, 4, 4, 0), (1025, 4, 4, 0),
                [1, 1025, 1025, 0, 0, 4, 0, 1, 1, 0] + [0] * 1024)
_splice_refusal("2^31 elements", (65536, 32768, 32768, 0), (65536, 32768, 32768, 0),
                [65536, 1, 1, 0, 0, 32768, 0, 1, 0, 0])

# kn_timemap_epilogue: in 7 x 8, pooled and relu 5 x 8, rows 5, width 2, delta 2
_E = [(7, 8, 12, 0), (5, 8, 12, 0), (5, 8, 12, 0)]


def _epi_refusal(name, ops=None, args=(5, 2, 1, 2), **swap):
    ops = list(_E if ops is None else ops)
    for k, op in swap.items():
        ops[int(k[2:])] = op
    refuse("kn_timemap_epilogue: " + name, "kn_timemap_epilogue", ops, list(args))


_epi_refusal("in NULL", op0=(7, 8, 12, -1))
_epi_refusal("neither output", op1=ABSENT, op2=ABSENT)
_epi_refusal("rows 0", args=(0, 2, 1, 2))
_epi_refusal("delta 0", args=(5, 2, 1, 0))
_epi_refusal("pool_width 0", args=(5, 0, 1, 2))
_epi_refusal("pool_channel 0", args=(5, 2, 0, 2))
_epi_refusal("a width without a pool", op1=ABSENT, args=(5, 2, 1, 2))
_epi_refusal("a pool_channel without a pool", [(5, 8, 12, 0), ABSENT, (5, 4, 8, 0)],
             args=(5, 1, 2, 1))
_epi_refusal("pool_channel not dividing the columns", args=(5, 2, 3, 2))
_epi_refusal("in stride < cols", op0=(7, 8, 7, 0))
_epi_refusal("the last tap outside in", op0=(6, 8, 12, 0))
_epi_refusal("pooled rows < rows", op1=(4, 8, 12, 0))
_epi_refusal("pooled cols", op1=(5, 7, 12, 0))
_epi_refusal("pooled stride < cols", op1=(5, 8, 7, 0))
_epi_refusal("relu rows < rows", op2=(4, 8, 12, 0))
_epi_refusal("relu cols", op2=(5, 9, 12, 0))
_epi_refusal("relu stride < cols", op2=(5, 8, 7, 0))

# kn_timemap_gather: map 7 x 8, out 5 x 24, one utterance, ext 2, 3 positions, dilation 1
_G = [(7, 8, 12, 0), (5, 24, 28, 0)]


def _gather_refusal(name, args=(1, 2, 3, 1), **swap):
    ops = list(_G)
    for k, op in swap.items():
        ops[int(k[2:])] = op
    refuse("kn_timemap_gather: " + name, "kn_timemap_gather", ops, list(args))


_gather_refusal("map NULL", op0=(7, 8, 12, -1))
_gather_refusal("out NULL", op1=(5, 24, 28, -1))
_gather_refusal("no utterance", args=(0, 2, 3, 1))
_gather_refusal("ext < 0", args=(1, -1, 3, 1))
_gather_refusal("positions 0", args=(1, 2, 0, 1))
_gather_refusal("positions 8193", args=(1, 0, 8193, 1), op0=(8197, 1, 1, 0),
                op1=(5, 8193, 8193, 0))
_gather_refusal("dilation 0", args=(1, 2, 3, 0))
_gather_refusal("fewer result rows than utterances", args=(6, 0, 3, 1), op0=(20, 8, 12, 0))
_gather_refusal("out cols", op1=(5, 25, 28, 0))
_gather_refusal("map stride < cols", op0=(7, 8, 7, 0))
_gather_refusal("out stride < cols", op1=(5, 24, 23, 0))
_gather_refusal("a map too short for the last tap", op0=(6, 8, 12, 0))
_gather_refusal("a map too short for the last utterance's ext", args=(2, 2, 3, 1),
                op0=(8, 8, 12, 0))


# ---- ctypes: the launchers as the GPU tests call them ----------------------------------------------
class SpliceGeom(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("num_chunks", "in_cs", "out_cs", "in_first",
                                            "out_first", "dim", "const_dim", "num_splice")] + \
               [("context", ctypes.c_int * 64), ("table", ctypes.c_int),
                ("in_index", ctypes.c_short * 1024)]


def splice_geom(c):
    g = SpliceGeom(c["num_chunks"], c["in_cs"], c["out_cs"], c["in_first"], c["out_first"],
                   c["dim"], c["const_dim"], len(c["context"]))
    for k, v in enumerate(c["context"]):
        g.context[k] = v
    g.table = int(c["in_index"] is not None)
    for k, v in enumerate(c["in_index"] or []):
        g.in_index[k] = v
    return g


def bind(kc):
    """libkcnn.so with the argument types of the kn_* launchers set."""
    lib, D = kc.lib(), kc.MatrixDim
    P, I, Z, F64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_double
    sig = {
        "kn_relu_prop": [P, D, P, D, P],
        "kn_relu_backprop": [P, D, P, D, P, D, P, P, P, P],
        "kn_splice_prop": [P, D, P, D, SpliceGeom, P],
        "kn_splice_backprop": [P, D, P, D, SpliceGeom, P],
        "kn_dvec_update": [P, P, F64, F64, I, P],
        "kn_softmax_prop": [P, D, P, D, P],
        "kn_softmax_backprop": [P, D, P, D, P, D, P, P, P],
        "kn_comp_objf_and_deriv": [P, P, P, I, P, D, P, D, P, P, P],
        "kn_softmax_xent_backprop": [P, D, P, D, P, P, P, P, P, P, P, P],
        "kn_objf_accuracy": [P, D, P, P, P, P, P, P],
        "kn_softmax_objf_accuracy": [P, D, P, P, P, P, P, P],
        "kn_loglikes": [P, D, P, D, P, P],
        "kn_softmax_loglikes": [P, D, P, D, P, P],
        "kn_normalize_prop": [P, D, P, D, P],
        "kn_normalize_backprop": [P, D, P, D, P, D, P],
        "kn_timemap_epilogue": [P, D, P, D, P, D, I, I, I, I, P],
        "kn_timemap_gather": [P, D, P, D, P, I, I, I, I, P],
    }
    assert sorted(sig) == sorted(LAUNCHERS)
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = I
    for name, args in (("kn_relu_stats_ws", [D]), ("kn_softmax_stats_ws", [D]),
                       ("kn_objf_ws", [I]), ("kn_prob_ws", [I])):
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = Z
    for name, args in (("kn_comp_objf_blocks", [I]), ("kn_softmax_xent_blocks", [D]),
                       ("kn_prob_blocks", [D])):
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = I
    return lib
