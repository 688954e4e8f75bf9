"""A numpy twin of cvLassoPath's host arithmetic and of cdh_path_sse, written from the definitions (not from api.py): the fold
ids of a seed, the size-weighted mean and spread of the folds' errors, the two selection rules, the rescaling that makes a
0/1-weighted loss on all rows the lasso on the training rows, and the sums of squared prediction errors in np.longdouble with
the forward error bound of the same sums taken in double."""
import numpy as np

U = 2.0 ** -53


def fold_ids(n, K, seed):
    return (np.random.default_rng(seed).permutation(n) % K).astype(np.int32)


def cv_curve(sizes, fold_mse):
    """-> (cvm, cvsd): cvm_j = sum_k (size_k / n) mse_kj, cvsd_j = sqrt(sum_k (size_k / n) (mse_kj - cvm_j)^2 / (K - 1))."""
    sizes = np.asarray(sizes, dtype=np.float64)
    fold_mse = np.asarray(fold_mse, dtype=np.float64)
    K, m = fold_mse.shape
    n = sizes.sum()
    cvm, cvsd = np.zeros(m), np.zeros(m)
    for j in range(m):
        cvm[j] = sum(sizes[k] / n * fold_mse[k, j] for k in range(K))
        cvsd[j] = np.sqrt(sum(sizes[k] / n * (fold_mse[k, j] - cvm[j]) ** 2 for k in range(K)) / (K - 1))
    return cvm, cvsd


def select(lam, cvm, cvsd):
    """-> (index_min, index_1se), 0-based: the first argmin of cvm; the largest lambda among those with
    cvm <= cvm[index_min] + cvsd[index_min], the lowest index among equal lambdas."""
    imin = 0
    for j in range(len(cvm)):
        if cvm[j] < cvm[imin]:
            imin = j
    thr = cvm[imin] + cvsd[imin]
    best = None
    for j in range(len(cvm)):
        if cvm[j] <= thr and (best is None or lam[j] > lam[best]):
            best = j
    return imin, best


def rescale(lam, n_train, n, standardize):
    """lambda of the weighted loss on all n rows whose iterates are those of the lasso at `lam` on the n_train training rows."""
    return lam * np.sqrt(n_train / n) if standardize else lam * n_train / n


def wstd(w, X):
    """_stdX!(out, w, X) (utils.jl:140-151)."""
    return np.sqrt((w[:, None] * X * X).sum(axis=0) / X.shape[0])


def path_sse(X, y, folds, k, idx1, B):
    """-> (held, train, a2_held, a2_train): the sums in np.longdouble (returned as float64), and sum_i a_i^2 with
    a_i = |y_i| + sum_t |X[i, idx1[t]] B[t, j]| over the same rows, which the forward bound multiplies."""
    L = np.longdouble
    Xs = np.asarray(X, dtype=np.float64)[:, np.asarray(idx1) - 1].astype(L)
    Bl = np.asarray(B, dtype=np.float64).astype(L)
    yl = np.asarray(y, dtype=np.float64).astype(L)
    res = yl[:, None] - Xs @ Bl
    a = np.abs(yl)[:, None] + np.abs(Xs) @ np.abs(Bl)
    held_rows = (np.asarray(folds) == k) if k >= 0 else np.zeros(len(yl), dtype=bool)
    sq, a2 = res * res, a * a
    f8 = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
    return (f8(sq[held_rows].sum(axis=0)), f8(sq[~held_rows].sum(axis=0)),
            f8(a2[held_rows].sum(axis=0)), f8(a2[~held_rows].sum(axis=0)))


def sse_bound(s, n_g, a2):
    """(2 s + n_g + 4) 2^-53 sum_i a_i^2: s FMAs per residual (relative error s u of a_i), the square doubles it and adds a
    rounding, and n_g - 1 additions in any order; the slack of 4 covers the second-order terms."""
    return (2 * s + n_g + 4) * U * np.asarray(a2)
