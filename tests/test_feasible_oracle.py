"""The restatement of feasibleLasso! that the GPU tests compare against (tests/_feasible_oracle.py), checked on its own on
the CPU: the recipe keeps every stopping statistic clear of optTol, the loop stops on its own, and what it stops at is a
lasso solution for the loadings its last solve used."""
import numpy as np
import pytest

import _feasible_oracle as FO

CASES = [(s, i) for s in FO.SEEDS for i in FO.INITS]


@pytest.mark.parametrize("seed,init", CASES)
def test_no_statistic_of_the_recipe_lies_within_5_percent_of_opttol(seed, init):
    """The condition on the inputs the device tests rest on: a device difference of 1e-10 in the loadings cannot move a
    statistic across optTol, so the outer iteration counts must agree."""
    stats = FO.solved(seed, init).stats
    print(seed, init, stats)
    assert all(abs(s - FO.OPT_TOL) > 0.05 * FO.OPT_TOL for s in stats), stats


@pytest.mark.parametrize("seed,init", CASES)
def test_the_loop_stops_before_maxiter_with_the_planted_support(seed, init):
    sol = FO.solved(seed, init)
    assert 2 <= len(sol.stats) < 20 and sol.stats[-1] < FO.OPT_TOL
    assert all(s >= FO.OPT_TOL for s in sol.stats[:-1])
    assert sorted(sol.x.nzval2ind.tolist()) == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("seed,init", CASES)
def test_kkt_of_the_final_iterate_against_the_loadings_its_last_solve_used(seed, init):
    """-X_k'r/n + lam0 Gamma_k sign(beta_k) = 0 on the support, |X_k'r/n| <= lam0 Gamma_k off it.  The last pass moved no
    coordinate by 1e-8 or more, so a coordinate's condition is off by at most sum_j |X_k'X_j/n| 1e-8 < p 2 1e-8 < 1e-6."""
    X, y, lam0 = FO.recipe(seed)
    sol = FO.solved(seed, init)
    beta = sol.x.dense()
    np.testing.assert_allclose(sol.residuals, y - X @ beta, rtol=0, atol=1e-10)
    assert np.abs(X.T @ X / FO.N).sum(axis=1).max() < 2 * FO.P
    g = -X.T @ sol.residuals / FO.N
    on = beta != 0
    assert np.max(np.abs(g[on] + lam0 * sol.used[on] * np.sign(beta[on]))) < 1e-6
    assert np.all(np.abs(g[~on]) <= lam0 * sol.used[~on] + 1e-6)
    # ... and the returned loadings are the ones computed AFTER that solve (the reference's aliasing, :181 and :186)
    np.testing.assert_array_equal(sol.loadings, FO.get_loadings(X, sol.residuals))
    assert np.max(np.abs(sol.loadings - sol.used)) > 0


def test_maxiter_2_returns_after_two_rounds():
    sol = FO.solved(1, "Screening", maxIter=2)
    assert len(sol.stats) == 2 and sol.stats[-1] >= FO.OPT_TOL
