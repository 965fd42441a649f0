"""Generate tests/golden/models/{dropout,softmax}.{bin,npz}: Kaldi binary
model files of DropoutComponent and SoftmaxComponent, encoded by
tests/kaldi_binary_nnet2.py from the reference's token sequences, plus the
fields they hold.  The GPU test reads them through Component::ReadNew and
requires Write to reproduce them byte for byte.

  python scripts/make_model_fixtures_nnet2.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kaldi_binary_nnet2 as KB2  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "models")


def main():
    os.makedirs(OUT, exist_ok=True)
    r = np.random.default_rng(20261019)
    fixtures = {
        "dropout": dict(dim=24, scale=0.25, proportion=0.375),
        "softmax": dict(dim=7, value_sum=r.random(7) * 10, deriv_sum=np.zeros(7), count=35.0),
    }
    for kind, p in fixtures.items():
        with open(os.path.join(OUT, f"{kind}.bin"), "wb") as fh:
            fh.write(KB2.encode(kind, p))
        np.savez(os.path.join(OUT, f"{kind}.npz"), **{k: np.asarray(v) for k, v in p.items()})
        print(kind, os.path.getsize(os.path.join(OUT, f"{kind}.bin")), "bytes")


if __name__ == "__main__":
    main()
