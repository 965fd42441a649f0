"""Kaldi binary encoding of NormalizeComponent, from the token sequence the
reference writes (nnet2/nnet-component.cc:398-412 NonlinearComponent::Write:
<Dim> <ValueSum> <DerivSum> <Count>), on the primitives of kaldi_binary.py.
"""
from kaldi_binary import HEADER, dvec, f64, i32, token


def normalize(p):
    out = token("<NormalizeComponent>") + token("<Dim>") + i32(int(p["dim"]))
    out += token("<ValueSum>") + dvec(p["value_sum"])
    out += token("<DerivSum>") + dvec(p["deriv_sum"])
    out += token("<Count>") + f64(float(p["count"]))
    return out + token("</NormalizeComponent>")


ENCODERS = {"normalize": normalize}


def encode(kind, params):
    return HEADER + ENCODERS[kind](params)
