"""bench.py's command line: a plain run carries the headline only, what takes runs of its own is behind --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "roofline", "config")
BEHIND_FULL = ("cpu_baseline", "e2e_gpu", "e2e_dropin", "e2e_dropin_large", "e2e_dropin_bgzf", "other_configs")


def run_bench(*args):
    return subprocess.run([sys.executable, BENCH] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def test_full_is_an_option_and_off_by_default():
    pr = run_bench("--help")
    assert pr.returncode == 0
    text = pr.stdout.decode()
    assert "--full" in text
    for kept in ("--gpus", "--steps", "--warmup", "--dump-outputs"):
        assert kept in text
    pr = run_bench("--full", "--steps", "0")   # a flag without a value: parsed, and the run refused for its steps alone
    assert pr.returncode == 2 and "--steps must be at least 1" in pr.stderr.decode()


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone():
    pr = run_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", "65536", "--batches", "2")
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    lines = [ln for ln in pr.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    for k in BEHIND_FULL:
        assert k not in out, k


@pytest.mark.gpu
def test_full_run_adds_what_moved():
    pr = run_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", "65536", "--batches", "2", "--full", "--no-extras",
                   "--cpu-sample", "20000")
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    out = json.loads(pr.stdout.decode().splitlines()[-1])
    for k in HEADLINE:
        assert k in out, k
    assert out["cpu_baseline"]["value"] > 0
