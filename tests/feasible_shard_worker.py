"""Worker of test_gpu_feasible.py::test_loadings_and_feasible_lasso_on_two_row_shards_over_the_host_exchange (run under
torch.distributed.run, every rank on cuda:0).  Each rank holds a row shard and the only exchange is the host-staged one
(cdh_set_host_exchange -> a gloo all-reduce), as in tests/host_exchange_worker.py: cdh_loadings sums its p partial sums over
the shards through that seam, and feasibleLasso_ runs its loop on them.  Every rank also holds the whole problem on a
handle of its own, the single-handle result the shards are compared with.  Prints FEASIBLE_SHARDS_OK from rank 0."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coordinatedescent_jl_amd as cd  # noqa: E402
from coordinatedescent_jl_amd import sharded  # noqa: E402
import _feasible_oracle as FO  # noqa: E402  (the recipe)

U64 = 2.0 ** -53


def main():
    cp = sharded.ControlPlane(backend="gloo")
    assert cp.world == 2

    def shard(y, X):
        n = X.shape[0]
        row0, nl = sharded.shard_rows(n, cp.rank, cp.world)
        f = cd.CDLeastSquaresLoss(y[row0:row0 + nl], X[row0:row0 + nl], device=0, n_total=n, row_offset=row0)
        sharded.connect_host(f, cp)
        return f

    def same_on_all_ranks(v):
        every = np.frombuffer(cp.all_gather_bytes(np.ascontiguousarray(v).tobytes()), dtype=np.float64).reshape(cp.world, -1)
        return all(np.array_equal(every[0], every[q]) for q in range(1, cp.world))

    # getLoadings at r = y: rounded data, an odd row count (the shards are 2050 + 2049 rows)
    n, p = 4099, 9
    rng = np.random.default_rng(31)
    X, y = np.asfortranarray(rng.standard_normal((n, p))), rng.standard_normal(n)
    bar = 0.5 * (n + 3) * U64 + 2 * U64                 # tests/test_gpu_feasible.py: _gamma_bar
    f, f1 = shard(y, X), cd.CDLeastSquaresLoss(y, X)
    for h in (f, f1):
        cd._lib.check(h._L.cdh_initialize(h._h, h.p, 0, None, None), h._h)
    before = f.exchange_stats()["host_calls"]
    got, one = cd.getLoadings(f), cd.getLoadings(f1)
    assert f.exchange_stats()["host_calls"] == before + 1           # one all-reduce of the p sums
    t = X.astype(np.longdouble) * y.astype(np.longdouble)[:, None]
    exact = np.sqrt(np.sum(t * t, axis=0) / np.longdouble(n))
    assert np.all(np.abs(got - one) <= bar * one), (got, one)
    assert np.all(np.abs(got - exact) <= bar * exact) and np.all(np.abs(one - exact) <= bar * exact)
    assert same_on_all_ranks(got)
    cp.barrier()
    f.close()
    f1.close()

    # feasibleLasso_ on shards against the single handle
    X, y, lam0 = FO.recipe(1)
    o = cd.IterLassoOptions(initProcedure="WarmStart", optionsCD=cd.CDOptions(**FO.CD))
    f, f1 = shard(y, X), cd.CDLeastSquaresLoss(y, X)
    x, x1 = cd.SparseIterate(FO.P), cd.SparseIterate(FO.P)
    sol, sol1 = cd.feasibleLasso_(x, f, None, lam0, o), cd.feasibleLasso_(x1, f1, None, lam0, o)
    err = float(np.max(np.abs(x.dense() - x1.dense())))
    assert err <= 1e-6 and x1.nnz == 5, err
    assert sol1.penalty.lam.shape == sol.penalty.lam.shape == (FO.P,)
    assert same_on_all_ranks(x.dense()) and same_on_all_ranks(sol.penalty.lam)
    es = f.exchange_stats()
    assert es["host_calls"] > 0 and es["rccl_calls"] == 0 and es["p2p_calls"] == 0 and es["nranks"] == 2
    cp.barrier()
    f.close()
    f1.close()
    if cp.rank == 0:
        print("FEASIBLE_SHARDS_OK")
    cp.shutdown()


if __name__ == "__main__":
    main()
