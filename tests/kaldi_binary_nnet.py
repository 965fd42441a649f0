"""Kaldi binary encoding of a whole network, the <Nnet> stream of upstream
nnet2 Nnet::Write (what nnet-init writes and nnet-am-copy / nnet-train* pass
around), on the independent component encoders of kaldi_binary.py,
kaldi_binary_nnet2.py and kaldi_binary_normalize.py:

  <Nnet> <NumComponents> int32 n <Components> n x Component </Components> </Nnet>

A network is a list of (kind, params) pairs, the kinds those of the three
component encoders.
"""
import kaldi_binary as KB
import kaldi_binary_nnet2 as KB2
import kaldi_binary_normalize as KBN
from kaldi_binary import HEADER, i32, token

ENCODERS = {**KB.ENCODERS, **KB2.ENCODERS, **KBN.ENCODERS}

TYPES = {"conv": "ConvolutionComponent", "maxpool": "MaxpoolComponent",
         "fc": "FullyConnectedComponent", "relu": "RectifiedLinearComponent",
         "splice": "SpliceComponent", "dropout": "DropoutComponent",
         "softmax": "SoftmaxComponent", "normalize": "NormalizeComponent"}


def nnet(components, num_components=None):
    """num_components: the count written (default: the true one)."""
    n = len(components) if num_components is None else num_components
    out = token("<Nnet>") + token("<NumComponents>") + i32(n) + token("<Components>")
    for kind, params in components:
        out += ENCODERS[kind](params)
    return out + token("</Components>") + token("</Nnet>")


def encode(components, num_components=None):
    return HEADER + nnet(components, num_components)


# ---- the fixture network's fields <-> one flat .npz -------------------------
def to_npz(components):
    """{'kinds': [...], '<index>.<field>': value}"""
    import numpy as np
    flat = {"kinds": np.array([k for k, _ in components])}
    for i, (_, p) in enumerate(components):
        for key, v in p.items():
            flat[f"{i}.{key}"] = np.asarray(v)
    return flat


def from_npz(z):
    kinds = [str(k) for k in z["kinds"]]
    comps = [(k, {}) for k in kinds]
    for name in z.files:
        if name == "kinds":
            continue
        i, key = name.split(".", 1)
        comps[int(i)][1][key] = z[name]
    return comps
