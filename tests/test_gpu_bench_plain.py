"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run and `--full`.

The plain run times its steps and nothing else: its line carries the
headline fields and none of the extra measurements, and `--dump-outputs`
writes the last timed step's spectrum and IR, the same arrays on every run
with the same arguments and under `--full`.  `--full` (here without the CPU
and network legs, which tests/test_gpu_bench_ranks.py and
tests/test_tunableop.py cover) adds the latency, graph and roofline figures."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
EXTRAS = ("cpu_baseline", "network_inference", "roofline", "ir_render_ms_per_pose", "ms_per_step_graph")


def _run(capsys, *extra):
    argv = ["--gpus", "1", "--steps", "5", "--warmup", "2", "--workload", "c1_meshrir_plumbing", *extra]
    assert bench.main(argv) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_line_and_outputs(capsys, tmp_path):
    from avr_amd.workloads import WORKLOADS

    w = WORKLOADS["c1_meshrir_plumbing"]
    d = _run(capsys, "--dump-outputs", str(tmp_path / "a"))
    assert all(k in d for k in HEADLINE) and not any(k in d for k in EXTRAS)
    assert d["metric"] == bench.METRIC and d["unit"] == "ray-samples/s" and d["higher_is_better"] is True
    assert d["steps"] == 5 and d["warmup"] == 2 and d["ms_per_step"] > 0
    # value is the whole-job rate of exactly the timed steps
    assert d["value"] == pytest.approx(w.ray_samples / (d["ms_per_step"] * 1e-3), rel=1e-9)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("spectrum", "ir")}
    assert sorted(os.listdir(tmp_path / "a")) == ["ir.npy", "spectrum.npy"]
    assert a["spectrum"].dtype == a["ir"].dtype == np.float32
    assert a["spectrum"].shape == (w.batch, w.F, 2) and a["ir"].shape == (w.batch, 2 * (w.F - 1))
    assert np.isfinite(a["spectrum"]).all() and np.abs(a["spectrum"]).max() > 0
    # the IR is the spectrum's irfft (fp32 transform of at most a few hundred bins)
    ir = np.fft.irfft(a["spectrum"][..., 0].astype(np.float64) + 1j * a["spectrum"][..., 1], axis=-1)
    assert np.abs(a["ir"] - ir).max() <= 1e-5 * np.abs(ir).max()

    full = _run(capsys, "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "b"))
    assert all(k in full for k in HEADLINE + ("roofline", "ir_render_ms_per_pose", "ms_per_step_graph"))
    assert "cpu_baseline" not in full
    # same seeded inputs, same kernels: a second run writes the same arrays bit for bit
    for n in a:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / (n + ".npy"))), n
