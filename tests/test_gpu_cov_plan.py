"""The device pass loop behind its launch plan (csrc/cov_plan.hpp) does what it did before the plan existed: on a small
lambda path whose support crosses from 10 to 11 coordinates, every counter the library exports and beta itself, bit for
bit, equal what the commit before the plan gave (tests/golden/cov_plan_counters.json, recorded from that commit's library
on an MI355X).  With CDH_CS_UCAP=16 that crossing is where a launch starts to bring helper workgroups and the list leaves
the LDS block for the Gram table (11 + 4 / 2 > 16 - 4); without the knob the same path stays in the LDS block.
p = 96 and not 64: a full pass is the loop's only while 4 nnz <= p, and it is a pass of the helpers only when its visit list is
longer than the 16 the knob leaves in LDS -- the support has to pass 16 below p / 4.

Recording (from a child process, with CDHIP_SO naming the library to record from):
    CDHIP_SO=/path/to/libcdhip.so python tests/test_gpu_cov_plan.py OUT.json
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cov_plan_counters.json")
N, P, S = 400, 96, 22
LAMBDAS = [float(v) for v in np.exp(np.linspace(np.log(1.8), np.log(0.12), 10))]   # supports 2, 10, 12, 16, 18, 20, 21, 21, 22, 22
OPTS = dict(maxIter=2000, optTol=1e-10, randomize=False)

pytestmark = pytest.mark.gpu


def problem():
    rng = np.random.default_rng(1907)
    X = np.asfortranarray(rng.standard_normal((N, P)))
    coef = np.linspace(2.0, 0.15, S) * np.where(np.arange(S) % 2 == 0, 1.0, -1.0)
    return X, X[:, :S] @ coef + 0.5 * rng.standard_normal(N)


def measure(ucap):
    """Per solve of the path: the loop's counters (not its clocks), the table's, the cache's, the solve's own, beta and the support."""
    import coordinatedescent_jl_amd as cd
    X, Y = problem()
    old = os.environ.pop("CDH_CS_UCAP", None)
    if ucap:
        os.environ["CDH_CS_UCAP"] = str(ucap)           # read when the handle is made
    try:
        f = cd.CDLeastSquaresLoss(Y, X)
    finally:
        os.environ.pop("CDH_CS_UCAP", None)
        if old is not None:
            os.environ["CDH_CS_UCAP"] = old
    f.set_gradient_cache(3)
    f.set_onchip_solve(False)
    x, out = cd.SparseIterate(P), []
    for lam in LAMBDAS:
        cd.coordinateDescent_(x, f, cd.ProxL1(lam), cd.CDOptions(**OPTS))
        ls, st = f.device_loop_stats(), f.last_stats
        out.append({
            "loop": [ls[k] for k in ("launches", "passes", "folds", "exact_rechecks")],
            "table": [ls["table"][k] for k in ("passes", "rows_filled", "coordinates", "capacity")]
                     + [ls["forced_rounds"]["host_pass"], ls["forced_rounds"]["loop"], ls["crew"]["passes"], ls["crew"]["jobs"]],
            "cache": list(f.cache_stats().values()),
            "solve": [int(st["passes"]), int(st["full_passes"]), int(st["visits"]), int(st["converged"])],
            "support": [int(k) for k in x.nzval2ind.tolist()],
            "beta": [float(v).hex() for v in x.dense()],
        })
    f.close()
    return out


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("ucap", [16, 0], ids=["ucap16", "default"])
def test_counters_and_beta_are_the_parents(golden, ucap):
    want, got = golden["ucap%d" % ucap], measure(ucap)
    assert len(got) == len(want) == len(LAMBDAS)
    for i, (g, w) in enumerate(zip(got, want)):
        print(i, {k: g[k] for k in ("loop", "table", "cache", "solve")}, len(g["support"]))
        for key in ("loop", "table", "cache", "solve", "support"):
            assert g[key] == w[key], (ucap, i, key, g[key], w[key])
        assert g["beta"] == w["beta"], (ucap, i)                    # bit for bit
    sizes = [len(g["support"]) for g in got]
    assert min(sizes) <= 10 and max(sizes) >= 11                    # the path crosses the edge it is about
    if ucap:        # ... and went where the plan sends it: the Gram table and the helpers
        assert got[-1]["table"][0] > 0 and got[-1]["table"][6] > 0, got[-1]["table"]
    else:
        assert got[-1]["table"][0] == 0 and got[-1]["table"][6] == 0 and got[-1]["loop"][0] >= len(LAMBDAS)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    rec = {"ucap16": measure(16), "ucap0": measure(0)}
    json.dump(rec, open(sys.argv[1], "w"), indent=0)
    print("recorded", [len(s["support"]) for s in rec["ucap16"]], rec["ucap16"][-1]["table"], rec["ucap0"][-1]["loop"])
