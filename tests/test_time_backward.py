"""The host plan of a training step over time maps, without a GPU: the runs of
a frame list (capi/frame-index.h, frame_runs), the training plan, the rows of
the segments and the backward schedule (capi/time-plan.h: time_train_plan,
plan_train_rows, time_backward_schedule), which NnetStack::PropagateFramesShared
and its backward run, as a stand-alone program under AddressSanitizer and
UBSan (scripts/time_backward_check.cc)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_time_backward_program_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "time_backward_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "kaldi-cnn_amd", "src"),
                    os.path.join(ROOT, "scripts", "time_backward_check.cc"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), os.path.join(GOLDEN, "nnet.config"),
                        os.path.join(GOLDEN, "freq_conv.config")], capture_output=True, text=True)
    print(r.stdout[-8000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all time backward checks passed" in r.stdout
    assert "WRONG" not in r.stdout and "REFUSED" not in r.stdout
    assert ("training prefixes: shrunken 8, shrunken pc 4 8, nnet.config 14, "
            "freq_conv.config 0\n") in r.stdout
    # the hand-written list: 51 frames in 11 runs, 51 + 11 x 10 level-0 rows; 7 launches each way
    assert ("shrunken: 51 frames in 11 runs: 161 level-0 rows, 7 forward and 7 backward "
            "launches\n") in r.stdout
    assert ("nnet.config: 51 frames in 11 runs: 271 level-0 rows, 13 forward and 13 backward "
            "launches\n") in r.stdout
