"""bench.py's command line: a plain run measures the headline only, --full adds the side
measurements (and owns their options).  CPU only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_skips_every_side_measurement(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert (a.ess_iters, a.ball_steps, a.kernel_iters, a.no_cpu, a.fixed_step_ref) == (0, 0, 0, True, False)
    # switching a side measurement off by name stays valid without --full (the profiling scripts do)
    a = _parse(monkeypatch, "--ess-iters", "0", "--ball-steps", "0", "--kernel-iters", "0", "--no-cpu",
               "--no-fixed-step-ref", "--dump-outputs", "d")
    assert (a.ess_iters, a.ball_steps, a.kernel_iters, a.no_cpu, a.fixed_step_ref) == (0, 0, 0, True, False)
    assert a.dump_outputs == "d"


@pytest.mark.parametrize("opt", ["--ess-iters", "--ball-steps", "--kernel-iters"])
def test_side_measurement_without_full_is_an_error(monkeypatch, opt):
    with pytest.raises(SystemExit) as e:
        _parse(monkeypatch, opt, "5")
    assert e.value.code == 2


def test_full_restores_the_side_measurements(monkeypatch):
    a = _parse(monkeypatch, "--full", "--steps", "7")
    assert (a.ess_iters, a.ball_steps, a.kernel_iters, a.no_cpu, a.fixed_step_ref) == (8000, 7, 256, False, True)
    a = _parse(monkeypatch, "--full", "--ess-iters", "40", "--ball-steps", "0", "--kernel-iters", "8", "--no-cpu")
    assert (a.ess_iters, a.ball_steps, a.kernel_iters, a.no_cpu, a.fixed_step_ref) == (40, 0, 8, True, True)
