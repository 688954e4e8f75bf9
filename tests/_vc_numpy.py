"""The yardstick of the varying-coefficient tests: a numpy restatement of what locpolyl1 recomputes per grid point
(reference src/varying_coefficient_lasso.jl:17-21, 63-65, 550-569; src/utils.jl:140-151), and the loop of :30-79 driven
through `oracle` (its CDWeightedLSLoss and coordinateDescent!).  tests/test_vc_host.py pins it against the reference's own
Kronecker check; tests/test_gpu_varying_coefficient.py holds the device code to it."""
import numpy as np


def weights(kind, h, z, z0):
    """evaluate.(kernel, z, z0) in double on z as stored, rounded once to z's type (what cdh_vc_set_point documents)."""
    d = z.astype(np.float64) - float(z0)
    if kind == "gaussian":
        w = np.exp(-(d * d) / h) / h
    else:
        u = d / h
        w = np.where(np.abs(u) >= 1.0, 0.0, 0.75 * (1.0 - u * u) / h)
    return w.astype(z.dtype)


def peak(kind, h):
    return (1.0 if kind == "gaussian" else 0.75) / h


def expand(X, z, z0, degree):
    """_expand_X! (:550-569): v = X[i, j]; v *= (z[i] - z0) per order, all in X's type."""
    T = X.dtype.type
    n, p = X.shape
    out = np.empty((n, p * (degree + 1)), dtype=X.dtype, order="F")
    df = (z - T(z0)).astype(X.dtype)
    for j in range(p):
        v = X[:, j].copy()
        out[:, j * (degree + 1)] = v
        for l in range(1, degree + 1):
            v = (v * df).astype(X.dtype)
            out[:, j * (degree + 1) + l] = v
    return out


def wstd(w, eX):
    """_stdX!(out, w, X) (utils.jl:140-151) summed in long double."""
    wl, xl = w.astype(np.longdouble), eX.astype(np.longdouble)
    return np.sqrt(((wl[:, None] * xl * xl).sum(axis=0) / eX.shape[0]).astype(np.float64))


def oracle_locpolyl1(O, X, z, y, zgrid, degree, kind, h, lam0, **opts):
    """locpolyl1 (:30-79) with the oracle's solver on the fp64 values of the inputs as given; -> (out, stats per point)."""
    ep = X.shape[1] * (degree + 1)
    beta = O.SparseIterate(ep)
    out, stats, orders = np.zeros((ep, len(zgrid))), [], []
    y64 = y.astype(np.float64)
    for ind, z0 in enumerate(zgrid):
        w = weights(kind, h, z, z0)
        eX = expand(X, z, z0, degree)
        sx = wstd(w, eX)
        f = O.CDWeightedLSLoss(y64, eX.astype(np.float64), w.astype(np.float64))
        st = O.coordinateDescent_(beta, f, O.ProxL1(lam0, sx), O.CDOptions(warmStart=True, **opts))
        out[:, ind] = beta.dense()
        stats.append(st)
        orders.append(np.array(beta.nzval2ind))
    return out, stats, orders


def gen_data(rng, n, s, noise_cols, dtype=np.float64):
    """genData (reference benchmark/locpoly_bench.jl:156-169) plus noise columns (test/varying_coefficient_lasso.jl:129-130)."""
    X = rng.standard_normal((n, s))
    Z = rng.random(n)
    eps = 0.1 * rng.standard_normal(n)
    rb = rng.choice([2, 4, 6, 8], size=s)
    Y = (np.sin(Z[:, None] * rb[None, :]) * X).sum(axis=1) + eps
    X = np.hstack([X, rng.standard_normal((n, noise_cols))])
    return np.asfortranarray(X.astype(dtype)), Z.astype(dtype), Y.astype(dtype)
