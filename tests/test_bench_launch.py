"""bench.py's self-launch (no GPU): `python bench.py --gpus N` without a
launcher in the environment runs itself under torch.distributed.run with N
ranks on 127.0.0.1 and passes the child's exit status on (VERDICT r04 item 2;
the GPU run of the same path is tests/test_gpu_dp.py)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_launch_ranks_command(monkeypatch):
    import bench
    seen = {}

    class R:
        returncode = 0

    def fake_run(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return R()

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "3"])
    assert bench.launch_ranks(8) == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--master-addr=127.0.0.1" in cmd
    assert cmd[-4:] == [os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "3"][-4:]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_launch_ranks_failure_is_nonzero(monkeypatch):
    import bench

    class R:
        returncode = -9   # a rank killed by a signal

    monkeypatch.setattr(subprocess, "run", lambda cmd, env=None: R())
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    assert bench.launch_ranks(2) != 0


class _FakeComponent:
    def __init__(self, linear=None, bias=None):
        self.linear, self.bias = linear, bias

    def NumGradientParams(self):
        return 0 if self.linear is None else self.linear.numel() + self.bias.numel()

    def LinearParams(self):
        return self.linear

    def BiasParams(self):
        return self.bias


class _FakeNet:
    """The part of kcnn.Nnet that bench.dump_outputs reads, on CPU tensors."""

    def __init__(self):
        import torch
        g = torch.Generator().manual_seed(5)
        self.out = torch.randn((8, 1000), generator=g)
        # a strided view, as the library's pitched matrices are
        self.din = torch.randn((8, 48), generator=g)[:, :33]
        self.components = [_FakeComponent(torch.randn((24, 16), generator=g),
                                          torch.randn(16, generator=g)),
                           _FakeComponent(),
                           _FakeComponent(torch.randn((100, 77), generator=g),
                                          torch.randn(100, generator=g))]

    def Output(self):
        return self.out

    def InputDeriv(self, i):
        assert i == 0
        return self.din


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """Arrays within their share of the budget are written whole, larger ones
    as the same seeded sample every time; everything is float32 and the files
    together stay within the budget."""
    import numpy as np
    import bench
    net = _FakeNet()
    names = ["output", "input_deriv", "component0_linear_params", "component0_bias_params",
             "component2_linear_params", "component2_bias_params"]
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 6 * 4 * 1024)   # 1024 elements each
    w = bench.dump_outputs(net, str(tmp_path / "a"))
    bench.dump_outputs(net, str(tmp_path / "b"))
    assert sorted(w) == sorted(names)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, b)
        assert w[n][0] == a.size
        total += a.nbytes
    assert total <= 6 * 4 * 1024
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "input_deriv.npy"), net.din.numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "component0_linear_params.npy"),
                                  net.components[0].linear.numpy())
    for n, full in (("output", net.out), ("component2_linear_params", net.components[2].linear)):
        a = np.load(tmp_path / "a" / (n + ".npy"))
        assert a.shape == (1024,) and w[n] == [1024, full.numel()]
        idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(
            full.numel(), 1024, replace=False))
        np.testing.assert_array_equal(a, full.numpy().reshape(-1)[idx])


def test_steps_must_be_positive(monkeypatch):
    import pytest
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


def test_main_relaunches_without_world_size(monkeypatch):
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    calls = []
    monkeypatch.setattr(bench, "launch_ranks", lambda n: calls.append(n) or 3)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 3
    assert calls == [4]
