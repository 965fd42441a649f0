"""The launches of a pass over time maps, without a GPU: time_schedule
(capi/time-plan.h), which both ComputeShared and an OnlineComputer's time-shared
step run through NnetStack::RunTimeSchedule, as a stand-alone program under
AddressSanitizer and UBSan.  The program compares the schedules of nnet.config,
freq_conv.config, nets F and M and the shrunken 1-D net, on utterances of (1,
7, 23, 2) result frames padded and unpadded and under both routes, with tables
written out by hand, launch by launch, and checks what must hold of every
schedule (scripts/time_schedule_check.cc)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NETS = {"nnet.config": (13, 8), "freq_conv.config": (3, 3), "net F": (3, 3), "net M": (8, 5),
        "shrunken": (7, 5), "shrunken pc 4": (7, 5)}  # launches: whole utterances, a step


def test_time_schedule_program_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "time_schedule_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "kaldi-cnn_amd", "src"),
                    os.path.join(ROOT, "scripts", "time_schedule_check.cc"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), os.path.join(GOLDEN, "nnet.config"),
                        os.path.join(GOLDEN, "freq_conv.config")], capture_output=True, text=True)
    print(r.stdout[-8000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all time schedule checks passed" in r.stdout
    assert "WRONG" not in r.stdout and "REFUSED" not in r.stdout and "declined" not in r.stdout
    for net, (whole, step) in NETS.items():
        for pad in ("padded", "unpadded"):
            assert f"{net} {pad}, whole utterances: {whole} launches\n" in r.stdout
            assert f"{net} {pad}, a streaming step: {step} launches\n" in r.stdout
    # the flagship's first level under each route, as printed
    lines = [" ".join(l.split()) for l in r.stdout.splitlines()]
    assert ("conv_taps comp 1 in 0 x 113 out 1 act -1 rows 110 H 0 C 0 kh 0 taps 4 delta 1 wc 1 "
            "wd 40 relu 0 ph 0 pc 0 n 0 context 0") in lines
    assert ("conv comp 1 in 0 x 113 out -1 act 2 rows 110 H 0 C 0 kh 0 taps 4 delta 1 wc 1 "
            "wd 40 relu 1 ph 0 pc 0 n 0 context 0") in lines
    assert ("gather2d comp 3 in 3 x 73 out -1 act -1 rows 33 H 33 C 0 kh 0 taps 0 delta 1 wc 0 "
            "wd 0 relu 0 ph 0 pc 0 n 11 context 10") in lines
