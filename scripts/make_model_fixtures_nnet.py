"""Generate tests/golden/models/nnet_small.{bin,npz}: the Kaldi binary <Nnet>
file of one small network holding every component kind that has an encoder
(Splice, Convolution, Maxpool, RectifiedLinear, Normalize, FullyConnected,
Dropout, FullyConnected, Softmax), encoded by tests/kaldi_binary_nnet.py, plus
the fields it holds.  The GPU tests read it through Nnet::Read and require
Write to reproduce it byte for byte.

  python scripts/make_model_fixtures_nnet.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kaldi_binary_nnet as KBN  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "models")


def network():
    r = np.random.default_rng(20261020)
    f = lambda *s: r.standard_normal(s).astype(np.float32)  # noqa: E731
    # 3 frames of 8 features -> an 8 x 3 x 1 map; 3 x 1 kernels, 6 maps
    H, W, C, kh, kw, G, pc = 8, 3, 1, 3, 1, 6, 3
    oh, ow = H - kh + 1, W - kw + 1
    conv_out, pool_out = oh * ow * G, oh * ow * G // pc
    hidden, classes = 10, 7
    empty = np.zeros(0)
    return [
        ("splice", dict(input_dim=H, context=np.array([-1, 0, 1], np.int32), const_dim=0)),
        ("conv", dict(H=H, W=W, C=C, kh=kh, kw=kw, stride=1, ph=0, pw=0, G=G, oh=oh, ow=ow,
                      lr=0.02, wd=0.0005, m=0.9, linear=f(kh * kw * C, G) * 0.5, b=f(G) * 0.5,
                      prev=f(kh * kw * C, G) * 0.01)),
        ("maxpool", dict(input_dim=conv_out, H=oh, W=ow, C=G, output_dim=pool_out, ph=1, pw=1,
                         pc=pc, overlap=False, overlap2D=False)),
        ("relu", dict(dim=pool_out, value_sum=r.random(pool_out) * 5,
                      deriv_sum=r.integers(0, 9, pool_out).astype(np.float64), count=9.0)),
        ("normalize", dict(dim=pool_out, value_sum=empty, deriv_sum=empty, count=0.0)),
        ("fc", dict(lr=0.01, linear=f(hidden, pool_out) * 0.3, b=f(hidden), wd=0.0005, m=0.5,
                    prev=f(hidden, pool_out) * 0.01)),
        ("dropout", dict(dim=hidden, scale=0.0, proportion=0.5)),
        ("fc", dict(lr=0.01, linear=f(classes, hidden), b=f(classes), wd=0.0005, m=0.5,
                    prev=f(classes, hidden) * 0.01)),
        ("softmax", dict(dim=classes, value_sum=r.random(classes) * 9, deriv_sum=np.zeros(classes),
                         count=9.0)),
    ]


def main():
    os.makedirs(OUT, exist_ok=True)
    comps = network()
    path = os.path.join(OUT, "nnet_small.bin")
    with open(path, "wb") as fh:
        fh.write(KBN.encode(comps))
    np.savez(os.path.join(OUT, "nnet_small.npz"), **KBN.to_npz(comps))
    print("nnet_small", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
