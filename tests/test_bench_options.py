"""bench.py: a plain run does only what its headline needs; --full adds the extra legs and the CPU baseline."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return _bench().parse()


def test_full_is_off_by_default(monkeypatch):
    assert not _parse(monkeypatch).full
    assert not _parse(monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2").full
    assert _parse(monkeypatch, "--full").full


def test_only_needs_full(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--only", "batch128")
    assert _parse(monkeypatch, "--full", "--only", "batch128").only == "batch128"


def _run(*argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-4000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    out = _run("--gpus", "1", "--rows", "200000", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    for key in HEADLINE_KEYS:
        assert key in out, key
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert "extra" not in out and "cpu_baseline" not in out
    ids = np.load(tmp_path / "ids.npy")
    assert ids.shape == (64, 10) and list(ids[0][:3].astype(np.int64)) == out["sample_result"]["ids"]


@pytest.mark.gpu
def test_full_run_adds_the_extra_legs():
    out = _run("--gpus", "1", "--rows", "200000", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--only", "config2_10m_b1")
    assert out["full"] is True
    assert list(out["extra"]) == ["config2_10m_b1"]
    assert out["extra"]["config2_10m_b1"]["steps"] == 3 and out["extra"]["config2_10m_b1"]["ms_per_step"] > 0
