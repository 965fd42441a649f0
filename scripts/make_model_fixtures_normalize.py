"""Generate tests/golden/models/normalize.{bin,npz}: the Kaldi binary model
file of a NormalizeComponent (dim 12; its statistics are never updated, so
they are empty with count 0), encoded by tests/kaldi_binary_normalize.py from
the reference's token sequence, plus the fields it holds.  The GPU test reads
it through Component::ReadNew and requires Write to reproduce it byte for byte.

  python scripts/make_model_fixtures_normalize.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kaldi_binary_normalize as KBN  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "models")


def main():
    os.makedirs(OUT, exist_ok=True)
    fixtures = {
        "normalize": dict(dim=12, value_sum=np.zeros(0), deriv_sum=np.zeros(0), count=0.0),
    }
    for kind, p in fixtures.items():
        with open(os.path.join(OUT, f"{kind}.bin"), "wb") as fh:
            fh.write(KBN.encode(kind, p))
        np.savez(os.path.join(OUT, f"{kind}.npz"), **{k: np.asarray(v) for k, v in p.items()})
        print(kind, os.path.getsize(os.path.join(OUT, f"{kind}.bin")), "bytes")


if __name__ == "__main__":
    main()
