"""-m gpu: a plain `bench.py` run prints the headline line and nothing that only `--full` measures; `--full` adds those legs after
the headline (small room, tiny camera; the session and scene legs are left out with --no-extras, the PMC passes with --no-pmc)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--gaussians", "20000", "--camera", "tiny", "--steps", "6", "--warmup", "2"]
FULL_ONLY = ["render_ms", "refine_iterations_per_s", "cpu_baseline", "dropin", "extra", "roofline_opaque", "value_context"]


def _line(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(flags), capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only():
    d = _line()
    assert d["full"] is False and d["steps"] == 6 and d["warmup"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 1000.0 / d["ms_per_step"] / 61.0) / d["value"] < 0.01
    # the event-timed roofline legs are the iterations before the warm-up: still run, still reported, PMC traffic not measured
    assert d["iterations_before_timed_region"] == 2 + 2 * 33 + 2
    assert d["roofline"]["avg_launch_ms"] > 0 and d["roofline"]["traffic"] is None and "--full" in d["roofline"]["traffic_source"]
    assert d["work_per_view"]["visible_gaussians"] > 0
    for k in FULL_ONLY:
        assert k not in d, k


def test_full_run_adds_its_legs_after_the_headline():
    d = _line("--full", "--no-extras", "--no-pmc", "--refine-iters", "8")
    assert d["full"] is True and d["iterations_before_timed_region"] == 2 + 2 * 33 + 2
    assert d["render_ms"]["forward"] > 0 and d["refine_iterations_per_s"] > 0 and d["cpu_baseline"]["value"] > 0
    assert "extra" not in d and "--full" not in d["roofline"]["traffic_source"]
