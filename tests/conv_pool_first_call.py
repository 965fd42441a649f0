"""Worker of test_gpu_conv_pool.py::test_first_call_in_a_process: in a fresh
process, the very first call of an f16x3 implicit-GEMM form (the pooled one,
then the unfused one) must succeed.  Each form sets its dynamic-LDS attribute
on its first call only, and a refused attribute once left its error for the
launcher to return: the kernels ran, the call reported a failure, and the
caller ran the layer again on another route.  Prints one line per call."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "kaldi-cnn_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import conv_pool_cases as T  # noqa: E402
import kcnn as kc  # noqa: E402
import test_gpu_conv_pool as G  # noqa: E402
from _pitched import place  # noqa: E402
from _util import dev  # noqa: E402


def main(name):
    kc.init(0)
    c = {k["name"]: k for k in T.CASES}[name]
    g = T.Geom(c["shape"], c["rows"])
    for n, v in T.families(c).items():
        kc.set_kernel_family(n, v)
    x, Wm, bv = G.make_data(c, g)
    X, Wd, B = place(kc, T.op(c, "x"), x), place(kc, T.op(c, "w"), Wm), dev(bv)
    print("fused rc", G.run_forward(kc, c, g, X, Wd, B, True)[0])
    # the unfused entry hides a failed route behind the next one (the fp32
    # MFMAs, other bits): its first result must be its second's
    first = G.conv2d_unfused(kc, g, X, Wd, B).get()
    second = G.conv2d_unfused(kc, g, X, Wd, B).get()
    print("unfused first == second", bool((first.view("u4") == second.view("u4")).all()))


if __name__ == "__main__":
    main(sys.argv[1])
