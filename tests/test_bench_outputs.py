"""CPU: bench.py's command line (a plain run unless --full) and its --dump-outputs writer: float64 files, at most the size
limit in all, a matrix beyond it replaced by the same seeded sample of rows on every run.  (The GPU side of both:
tests/test_gpu_bench.py.)"""
import importlib.util
import os

import numpy as np
import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_unless_full():
    b = _bench()
    a = b.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = b.parse(["--steps", "7", "--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    assert b.DUMP_LIMIT_BYTES == 64 * 2 ** 20


def test_dump_outputs_float64_within_the_limit(tmp_path):
    b = _bench()
    g = torch.Generator().manual_seed(0)
    mu = torch.randn(64, dtype=torch.float64, generator=g)
    S = torch.randn(64, 64, dtype=torch.float64, generator=g)
    b.dump_outputs(str(tmp_path / "whole"), [("mu", mu), ("S", S)])
    assert sorted(os.listdir(tmp_path / "whole")) == ["S.npy", "mu.npy"]
    for name, t in (("mu", mu), ("S", S)):
        a = np.load(tmp_path / "whole" / f"{name}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, t.numpy())
    # room for mu and ten rows of S (each with its index): a seeded sample of ten rows, the same on every call
    limit = 64 * 8 + 10 * (64 * 8 + 8)
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), [("mu", mu), ("S", S)], limit=limit)
    assert sorted(os.listdir(tmp_path / "s1")) == ["S_sample.npy", "S_sample_rows.npy", "mu.npy"]
    rows = np.load(tmp_path / "s1" / "S_sample_rows.npy")
    sample = np.load(tmp_path / "s1" / "S_sample.npy")
    assert rows.dtype == np.float64 and sample.dtype == np.float64 and len(rows) == 10
    assert np.array_equal(rows, np.unique(rows)) and np.array_equal(sample, S.numpy()[rows.astype(int)])
    for f in os.listdir(tmp_path / "s1"):
        assert open(tmp_path / "s1" / f, "rb").read() == open(tmp_path / "s2" / f, "rb").read(), f
    assert sum(np.load(tmp_path / "s1" / f).nbytes for f in os.listdir(tmp_path / "s1")) <= limit
