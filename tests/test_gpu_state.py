"""copy.deepcopy, save / load and pickle of experiment objects (optbayesexpt_amd/_state.py): a copy or a restored
object continues BIT FOR BIT where the original stood — settings, cloud, weights and generator state are compared
with np.array_equal / ==, never with a tolerance.  The save / load cases are continued in a fresh child process."""
import copy
import json
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _state_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAVED = ("lorentz_full", "strict4096", "fused65536", "noise7", "sweeper", "expression", "function", "mt19937",
         "subclass")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), **extra)
    return env


def _child(args, timeout, **extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_state_cases.py")] + args, cwd=ROOT,
                       env=_env(**extra), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _same(a, b):
    assert a["picks"] == b["picks"]
    assert np.array_equal(a["particles"], b["particles"])
    assert np.array_equal(a["weights"], b["weights"])
    np.testing.assert_equal(a["rng"], b["rng"])


def _walk(x, path="state"):
    """No torch tensor, no ctypes object anywhere in a snapshot."""
    import ctypes
    assert not isinstance(x, torch.Tensor), path
    assert not isinstance(x, (ctypes._SimpleCData, ctypes.Structure, ctypes.Array)), path
    if isinstance(x, dict):
        for k, v in x.items():
            _walk(v, f"{path}[{k!r}]")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _walk(v, f"{path}[{i}]")
    elif isinstance(x, np.ndarray):
        assert x.dtype != object, path


@pytest.fixture(scope="module")
def saved(hip, tmp_path_factory):
    """Every case: 10 cycles, saved straight after the 10th pdf_update, 40 more cycles in this process; then ONE
    child process loads all of them and runs the same 40 cycles."""
    import optbayesexpt_amd as obe
    from optbayesexpt_amd import _state
    folder = str(tmp_path_factory.mktemp("state"))
    here = {}
    for case in SAVED:
        o = cases.build(case)
        cases.run(o, case, 0, cases.BEFORE)
        if case == "lorentz_full":
            assert o._sweeps.ticket is not None          # the speculative sweep of cycle 11 is in flight
        at_save = getattr(o, "constraint_calls", None)
        obe.save(o, os.path.join(folder, case + ".state"))
        with open(os.path.join(folder, case + ".state"), "rb") as f:
            _walk(pickle.load(f))
        here[case] = cases.outcome(o, *cases.run(o, case, cases.BEFORE, cases.CONTINUE))
        here[case]["snapshot"] = _state.snapshot(o)
        here[case]["user"] = dict(at_save=at_save, calls=getattr(o, "constraint_calls", None))
        del o
    _child(["continue", folder] + list(SAVED), timeout=600)
    child = {}
    for case in SAVED:
        with open(os.path.join(folder, case + ".child.pkl"), "rb") as f:
            child[case] = pickle.load(f)
    return here, child


@pytest.mark.parametrize("case", SAVED)
def test_saved_object_continues_in_a_fresh_process(saved, case):
    here, child = saved
    _same(here[case], child[case])
    _walk(here[case]["snapshot"])
    if case == "lorentz_full":
        assert any(child[case]["resampled"]), "no resample after the restore"


def test_user_subclass_keeps_its_attributes_and_hook(saved):
    here, child = saved
    got = child["subclass"]
    assert got["cls"] == "_state_cases:Constrained"
    assert got["user"]["cost_of_changing_setting"] == 2.5
    # the NumPy hook ran after every resample of the child's 40 cycles, counting on from the saved count
    saved_calls = here["subclass"]["user"]["at_save"]
    assert saved_calls > 0
    assert got["user"]["constraint_calls"] == saved_calls + sum(got["resampled"]) == here["subclass"]["user"]["calls"]


def test_deepcopy_continues_alongside_the_original(hip):
    """10 cycles, a deepcopy, then 40 more cycles on the original, the copy and an untouched twin: equal at every
    cycle (setting, weights), cloud and generator state equal at the end, with resamples in the second half."""
    case = "lorentz_full"
    o, twin = cases.build(case), cases.build(case)
    cases.run(o, case, 0, cases.BEFORE)
    cases.run(twin, case, 0, cases.BEFORE)
    c = copy.deepcopy(o)
    assert type(c) is type(o) and c._sweeps is not o._sweeps and c._ws.data_ptr() != o._ws.data_ptr()
    logs = [[], [], []]
    res = [cases.run(x, case, cases.BEFORE, cases.CONTINUE, weights_log=log) for x, log in zip((o, c, twin), logs)]
    assert res[0] == res[1] == res[2]
    for k in range(cases.CONTINUE):
        assert np.array_equal(logs[0][k], logs[1][k]) and np.array_equal(logs[0][k], logs[2][k]), k
    assert any(res[0][1][cases.CONTINUE // 2:]), "no resample in the second half"
    out = [cases.outcome(x, *r) for x, r in zip((o, c, twin), res)]
    _same(out[0], out[1])
    _same(out[0], out[2])


def test_pickle_round_trip_in_process(hip):
    case = "noise7"
    o = cases.build(case)
    cases.run(o, case, 0, 3)
    r = pickle.loads(pickle.dumps(o))
    a, b = cases.run(o, case, 3, 8), cases.run(r, case, 3, 8)
    _same(cases.outcome(o, *a), cases.outcome(r, *b))


def test_copy_is_independent(hip):
    case = "strict4096"
    o = cases.build(case)
    cases.run(o, case, 0, 5)
    w_before = np.array(o.particle_weights)
    ref = copy.deepcopy(o)
    c = copy.deepcopy(o)
    c.particle_weights[7] = 0
    c.particle_weights[100:200] = 0
    c.opt_setting()
    assert np.array_equal(o.particle_weights, w_before)
    assert o.opt_setting() == ref.opt_setting()
    assert o.last_setting_index == ref.last_setting_index
    assert c.rng is not o.rng and c.tuning_parameters is not o.tuning_parameters


def test_sharded_object_refuses_deepcopy(hip):
    import optbayesexpt_amd as obe
    g = np.random.default_rng(3)
    o = obe.OptBayesExpt(obe.models.lorentzian(), (np.linspace(1.5, 4.5, 64),), cases._lorentz_prior(g, 1024),
                         (0.1,), settings_shard=obe.SettingsShard(rank=0, world_size=2))
    with pytest.raises(TypeError, match="save"):
        copy.deepcopy(o)


def test_other_format_version_is_refused(hip, tmp_path):
    import optbayesexpt_amd as obe
    from optbayesexpt_amd import _state
    o = cases.build("strict4096")
    st = _state.snapshot(o)
    st["format"] = _state.FORMAT_VERSION + 1
    path = tmp_path / "future.state"
    with open(path, "wb") as f:
        pickle.dump(st, f)
    with pytest.raises(ValueError, match=f"{_state.FORMAT_VERSION + 1}.*{_state.FORMAT_VERSION}"):
        obe.load(str(path))


def test_copy_and_save_under_the_delivery_audit(hip, tmp_path):
    """The deepcopy and save / load scenarios in one child process with OBE_CHECK_DELIVERY=1: no armed host word
    is read, no landing zone is released with armed words."""
    report = tmp_path / "audit.jsonl"
    r = _child(["audit", str(tmp_path)], timeout=600, OBE_CHECK_DELIVERY="1", OBE_AUDIT_REPORT=str(report))
    assert "audit run ok" in r.stdout and "DeliveryError" not in r.stdout + r.stderr
    rows = [json.loads(l) for l in report.read_text().splitlines()]
    assert not any(row["pending_violations"] for row in rows), rows
    assert sum(row["reads"] for row in rows) > 100 and sum(row["armed"] for row in rows) > 20


def _shard_worker(rank, world, port, folder, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import optbayesexpt_amd as obe
        case, path = "lorentz_full", os.path.join(folder, "sharded.state")
        o = cases.build(case, settings_shard=obe.SettingsShard())
        cases.run(o, case, 0, cases.BEFORE)
        if rank == 0:
            obe.save(o, path)
        dist.barrier()
        with pytest.raises(TypeError):
            copy.deepcopy(o)
        kept = cases.outcome(o, *cases.run(o, case, cases.BEFORE, 20))
        r = obe.load(path, settings_shard=obe.SettingsShard())           # (collective, as construction)
        ret[rank] = (kept, cases.outcome(r, *cases.run(r, case, cases.BEFORE, 20)))
    finally:
        dist.destroy_process_group()


def test_sharded_object_saved_and_restored_sharded_or_not(hip, tmp_path):
    """A 2-rank (gloo, one GPU) sharded object saved after 10 cycles: the sharded original, the file restored as 2
    new shards and the file restored unsharded all continue as an unsharded run of the same experiment."""
    import torch.multiprocessing as mp
    import optbayesexpt_amd as obe
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    mp.spawn(_shard_worker, args=(2, port, str(tmp_path), ret), nprocs=2, join=True)
    case = "lorentz_full"
    twin = cases.build(case)
    cases.run(twin, case, 0, cases.BEFORE)
    want = cases.outcome(twin, *cases.run(twin, case, cases.BEFORE, 20))
    u = obe.load(str(tmp_path / "sharded.state"))
    assert u._shard is None
    _same(cases.outcome(u, *cases.run(u, case, cases.BEFORE, 20)), want)
    for rank in (0, 1):
        kept, restored = ret[rank]
        _same(kept, want)
        _same(restored, want)
