"""bench.py's host side without a GPU: --dump-outputs writes float32 .npy files within its budget, the same seeded rows of every
output, and every row when they fit; --steps below 1 is refused."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _outputs(BH, N, d):
    g = torch.Generator().manual_seed(3)
    o, dq, dk, dv = (torch.rand((BH, N, d), generator=g) for _ in range(4))
    return (("o", o), ("L", torch.rand((BH, N), generator=g)), ("dq", dq), ("dk", dk), ("dv", dv))


def test_dump_outputs_samples_rows_of_the_metric_shape(tmp_path):
    BH, N, d = 64, 4096, 64
    named = _outputs(BH, N, d)
    bench.dump_outputs(str(tmp_path / "a"), BH, N, d, named)
    bench.dump_outputs(str(tmp_path / "b"), BH, N, d, named)
    total = sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n, _ in named)
    assert total <= 64 * 10**6
    keep = bench.DUMP_BYTES // (4 * (4 * d + 1))
    rows = np.sort(np.random.default_rng(0).choice(BH * N, size=keep, replace=False))
    for n, t in named:
        a = np.load(tmp_path / "a" / (n + ".npy"))
        assert a.dtype == np.float32
        assert np.array_equal(a, np.load(tmp_path / "b" / (n + ".npy")))
        want = t.reshape(BH * N, -1).numpy()[rows]
        assert np.array_equal(a, want[:, 0] if t.dim() == 2 else want)


def test_dump_outputs_keeps_every_row_when_small(tmp_path):
    BH, N, d = 2, 128, 64
    named = _outputs(BH, N, d)
    bench.dump_outputs(str(tmp_path), BH, N, d, named)
    for n, t in named:
        a = np.load(tmp_path / (n + ".npy"))
        assert np.array_equal(a, t.reshape(BH * N, -1).numpy().squeeze(1) if t.dim() == 2 else t.reshape(BH * N, d).numpy())


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--config", "c4", "--dump-outputs", "x"]])
def test_parse_refuses(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit):
        bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
