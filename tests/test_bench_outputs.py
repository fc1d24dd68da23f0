"""bench.py's plain run and its --dump-outputs: the lean line of a run without --full, and the arrays that the last
timed step computed (CPU: the writer itself; GPU: a c2 run end to end)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stub_obe(n_settings, d, n_p):
    import torch
    g = np.random.default_rng(7)
    w = g.random(n_p)
    o = types.SimpleNamespace(_s_begin=0, _s_end=n_settings,
                              _utility_dev=torch.from_numpy(g.random(n_settings)),
                              particles=g.normal(size=(d, n_p)), particle_weights=w / w.sum())
    o._gather_settings = lambda local: local.cpu().numpy()
    return o


def test_dump_writes_float64_arrays_and_keeps_the_whole_cloud_under_the_budget(tmp_path):
    import bench
    o = _stub_obe(64, 3, 1000)
    bench.dump_outputs(o, str(tmp_path), (2.5,), 0)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"setting", "utility", "particles", "particle_weights"}
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["setting"], [2.5])
    np.testing.assert_array_equal(got["utility"], o._utility_dev.numpy())
    np.testing.assert_array_equal(got["particles"], o.particles)
    np.testing.assert_array_equal(got["particle_weights"], o.particle_weights)


def test_dump_of_a_cloud_over_the_budget_is_a_fixed_sample(tmp_path):
    import bench
    o = _stub_obe(64, 3, 5000)
    budget = 64 * 8 + 8 + 20000
    for k in (0, 1):
        bench.dump_outputs(o, str(tmp_path / str(k)), (2.5,), 0, budget_bytes=budget)
    a = {f[:-4]: np.load(tmp_path / "0" / f) for f in os.listdir(tmp_path / "0")}
    b = {f[:-4]: np.load(tmp_path / "1" / f) for f in os.listdir(tmp_path / "1")}
    assert sum(x.nbytes for x in a.values()) <= budget
    idx = a["particle_index"].astype(np.int64)
    assert 0 < idx.size < 5000 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(a["particles"], o.particles[:, idx])
    np.testing.assert_array_equal(a["particle_weights"], o.particle_weights[idx])
    for name in a:                                     # the same columns in every run
        np.testing.assert_array_equal(a[name], b[name])


def test_dump_is_written_by_rank_0_only(tmp_path):
    import bench
    bench.dump_outputs(_stub_obe(8, 2, 10), str(tmp_path / "r1"), (1.0,), 1)
    assert not (tmp_path / "r1").exists()


@pytest.mark.gpu
def test_plain_run_prints_the_lean_line_and_dumps_the_last_step(hip, tmp_path):
    """Two plain c2 runs with the same arguments: the lean line, and the same arrays from both, bit for bit."""
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    dumps = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c2", "--steps", "3", "--warmup",
                            "2", "--dump-outputs", str(tmp_path / run)], env=env, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["warmup"] == 2 and out["n_gpus"] == 1
        assert out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
        assert out["unit"] == "model-evals/s" and out["dtype"] == "f64" and out["metric"].startswith("model-evals/sec")
        for key in ("roofline", "roofline_update", "cpu_baseline", "published_workload", "other_configs", "rccl"):
            assert key not in out, key                      # measured with --full only
        dumps.append({f[:-4]: np.load(tmp_path / run / f) for f in os.listdir(tmp_path / run)})
    got = dumps[0]
    ns, n_p = bench.CONFIGS["c2"][:2]
    assert set(got) == {"setting", "utility", "particles", "particle_weights"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["utility"].shape == (ns,) and np.isfinite(got["utility"]).all()
    assert got["particles"].shape == (3, n_p) and got["particle_weights"].shape == (n_p,)
    assert abs(got["particle_weights"].sum() - 1.0) < 1e-9
    settings = bench.make_workload("c2")[0][0]
    assert got["setting"][0] == settings[int(np.argmax(got["utility"]))]     # the setting that utility chose
    assert set(dumps[1]) == set(got)
    for name in got:                                        # same arguments, same inputs: the same outputs
        np.testing.assert_array_equal(dumps[1][name], got[name], err_msg=name)
