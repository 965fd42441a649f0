"""Kaldi binary encodings of DropoutComponent and SoftmaxComponent, from the
token sequences the reference writes (nnet2/nnet-component.cc:3572-3581
Dropout -- <Dim> <DropoutScale> <DropoutProportion>: scale BEFORE proportion,
unlike upstream Kaldi; :398-412 NonlinearComponent for Softmax), on the
primitives of kaldi_binary.py.
"""
from kaldi_binary import HEADER, dvec, f32, f64, i32, token


def dropout(p):
    out = token("<DropoutComponent>") + token("<Dim>") + i32(int(p["dim"]))
    out += token("<DropoutScale>") + f32(float(p["scale"]))
    out += token("<DropoutProportion>") + f32(float(p["proportion"]))
    return out + token("</DropoutComponent>")


def softmax(p):
    out = token("<SoftmaxComponent>") + token("<Dim>") + i32(int(p["dim"]))
    out += token("<ValueSum>") + dvec(p["value_sum"])
    out += token("<DerivSum>") + dvec(p["deriv_sum"])
    out += token("<Count>") + f64(float(p["count"]))
    return out + token("</SoftmaxComponent>")


ENCODERS = {"dropout": dropout, "softmax": softmax}


def encode(kind, params):
    return HEADER + ENCODERS[kind](params)
