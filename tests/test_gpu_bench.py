"""bench.py as the headline is measured: a plain run times the steps and nothing else, --full adds the figures beside the
headline, and --dump-outputs writes what the last timed step computed -- the same arrays from run to run, with or without
--full, and (row shards gathered) from two ranks as from one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--rows", "300000", "--cols", "96", "--planted", "10", "--block", "16"]
OUTPUTS = ("beta", "max_h", "residual_sample")


def _bench(args, cwd=ROOT, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=600, cwd=cwd, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(got) == 1 and got[0].startswith("{"), got
    return json.loads(got[0])


def _load(d):
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in OUTPUTS)
    return {k: np.load(os.path.join(d, k + ".npy")) for k in OUTPUTS}


def test_plain_run_dumps_the_timed_outputs_and_full_adds_the_rest(tmp_path):
    d1, d2, d3 = (str(tmp_path / k) for k in ("d1", "d2", "d3"))
    j1 = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", d1] + SMALL)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j1, k
    assert j1["steps"] == 3 and j1["ms_per_step"] > 0 and j1["dtype"] == "f64"
    for k in ("graph_trial", "sparse_regime", "cpu_baseline", "timed_sweep_parity", "cfg1", "cfg3_path", "ref_shape_path"):
        assert k not in j1, k
    o1 = _load(d1)
    assert o1["beta"].shape == (96,) and o1["residual_sample"].shape == (300000,)
    assert all(v.dtype == np.float64 for v in o1.values())
    assert o1["max_h"][0] == j1["config"]["last_maxH"]
    assert abs(np.abs(o1["beta"]).sum() - j1["config"]["beta_abs_sum"]) <= 1e-12 * j1["config"]["beta_abs_sum"]
    # the same arguments: the same inputs, the same outputs
    _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", d2] + SMALL)
    o2 = _load(d2)
    for k in OUTPUTS:
        np.testing.assert_array_equal(o1[k], o2[k], err_msg=k)
    # --full: the figures beside the headline, measured after the outputs were taken
    j3 = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-live-traffic", "--dump-outputs", d3] + SMALL)
    for k in ("graph_trial", "sparse_regime", "cpu_baseline", "timed_sweep_parity", "cfg1"):
        assert k in j3 and "error" not in j3[k], (k, j3.get(k))
    assert j3["timed_sweep_parity"]["ok"]
    o3 = _load(d3)
    for k in OUTPUTS:
        np.testing.assert_array_equal(o1[k], o3[k], err_msg=k)


def test_two_ranks_dump_the_same_outputs_as_one(tmp_path):
    """Row shards on one GPU over the direct exchange: the residual sample is gathered into global row order, and a relative
    DIR names the caller's directory, not the one the ranks start in."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["CDH_P2P_SPIN_LIMIT"] = "4000000"
    common = ["--steps", "2", "--warmup", "1"] + SMALL
    ja = _bench(["--gpus", "2", "--no-rccl", "--exchange", "p2p", "--dump-outputs", "two"] + common, cwd=str(tmp_path), env=env)
    jb = _bench(["--gpus", "1", "--dump-outputs", "one"] + common, cwd=str(tmp_path), env=env)
    assert ja["n_gpus"] == 2 and ja["config"]["exchange"] == "p2p"
    oa, ob = _load(str(tmp_path / "two")), _load(str(tmp_path / "one"))
    np.testing.assert_allclose(oa["beta"], ob["beta"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(oa["max_h"], ob["max_h"], rtol=1e-9)
    np.testing.assert_allclose(oa["residual_sample"], ob["residual_sample"], rtol=0, atol=1e-8)
