"""The yardstick of the leave-one-out tests: lvocv_locpolyl1 (reference src/varying_coefficient_lasso.jl:82-137) restated in
numpy on top of tests/_vc_numpy.py, with the solves through `oracle`'s CDWeightedLSLoss and coordinateDescent!.  Besides the
MSE it returns, per point, what the device is held to (the sigma-iteration count, beta, the refit, the prediction) and what
makes the comparison well-posed: the margin of every sigma decision and the gap between the s-th and (s+1)-th screening score.
tests/test_vc_cv_host.py pins its pieces against closed forms; tests/test_gpu_vc_cv.py holds the device code to it."""
import numpy as np

from _vc_numpy import expand, weights, wstd

SIGMA_TOL = 1e-2        # :122
SIGMA_ITERS = 10        # :119
SCREEN = 10             # :114, min(10, ep)


def get_sigma(w, r):
    """_getSigma(w, r) (utils.jl:167-175)."""
    w, r = np.asarray(w, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return float(np.sqrt((r * r * w).sum() / w.sum()))


def screening_scores(w, eX, y):
    """|sum_i X_ij w_i y_i| (utils.jl:108-124), summed in long double."""
    wy = w.astype(np.longdouble) * y.astype(np.longdouble)
    return np.abs((eX.astype(np.longdouble) * wy[:, None]).sum(axis=0)).astype(np.float64)


def screening_set(scores, s):
    """`storage .>= nlargest(s, storage)[end]`: ties kept."""
    return scores >= np.sort(scores)[::-1][s - 1]


def find_init_residuals(w, eX, y, s):
    """_findInitResiduals!(w, X, y, s, r) (utils.jl:79-92) -> (r, S, scores): the weighted least squares fit on the screened
    columns through a QR of sqrt(w) X_S (the normal equations' solution without their squared condition number)."""
    w, eX, y = w.astype(np.float64), eX.astype(np.float64), y.astype(np.float64)
    scores = screening_scores(w, eX, y)
    S = screening_set(scores, s)
    sw = np.sqrt(w)
    b = np.linalg.lstsq(sw[:, None] * eX[:, S], sw * y, rcond=None)[0]
    return y - eX[:, S] @ b, S, scores


def groups_mask(beta, p, degree):
    """get_nonzero_coordinates!(S, beta, p, degree, true) (:479-512)."""
    return np.repeat((beta.reshape(p, degree + 1) != 0.0).any(axis=1), degree + 1)


def refit(w, eX, y, S):
    """(Xs'W Xs) \\ (Xs'W y) (:132) with the normal equations formed in long double and solved at unit diagonal ->
    (coefficients on S, the 2-norm condition number of the scaled block)."""
    wl, Xs = w.astype(np.longdouble), eX[:, S].astype(np.longdouble)
    G = (Xs.T * wl) @ Xs
    c = (Xs.T * wl) @ y.astype(np.longdouble)
    d = np.sqrt(np.diag(G))
    Gs = (G / np.outer(d, d)).astype(np.float64)
    b = np.linalg.solve(Gs, (c / d).astype(np.float64)) / d.astype(np.float64)
    return b, float(np.linalg.cond(Gs))


def oracle_lvocv(O, X, z, y, degree, kind, hArr, lam0, rows=None, **opts):
    """lvocv_locpolyl1 (:82-137) on the fp64 values of the inputs as given (weights and expansion formed in the inputs' own
    type, as the device forms them) -> (MSE, one record per point in loop order).  beta is one iterate carried across all
    points and bandwidths; an empty support predicts 0.  `rows` (default: all of them, as the reference) limits the loop to
    those observations, for timing a prefix of it."""
    n, p = X.shape
    ep = p * (degree + 1)
    s = min(SCREEN, ep)
    beta = O.SparseIterate(ep)
    y64 = y.astype(np.float64)
    MSE, points = np.zeros(len(hArr)), []
    for indH, h in enumerate(hArr):
        for i in (range(n) if rows is None else rows):
            z0 = z[i]
            w = weights(kind, h, z, z0)
            w[i] = 0
            eX = expand(X, z, z0, degree)
            sx = wstd(w, eX)
            w64, eX64 = w.astype(np.float64), eX.astype(np.float64)
            r, S0, scores = find_init_residuals(w, eX, y, s)
            srt = np.sort(scores)[::-1]
            score_gap = float((srt[s - 1] - srt[s]) / srt[0]) if ep > s else np.inf
            sigma = get_sigma(w64, r)
            f = O.CDWeightedLSLoss(y64, eX64, w64)
            sigmas, margins, solves = [sigma], [], []
            for _ in range(SIGMA_ITERS):
                solves.append(O.coordinateDescent_(beta, f, O.ProxL1(lam0 * sigma, sx), O.CDOptions(warmStart=True, **opts)))
                sigmanew = get_sigma(w64, f.r)
                sigmas.append(sigmanew)
                q = abs(sigmanew - sigma) / sigma
                margins.append(abs(q - SIGMA_TOL) / SIGMA_TOL)
                if q < SIGMA_TOL:
                    break
                sigma = sigmanew
            b = beta.dense()
            S = groups_mask(b, p, degree)
            coef, kappa, yhat = None, 1.0, 0.0
            if S.any():
                coef, kappa = refit(w, eX, y, S)
                yhat = float(eX64[i, S] @ coef)
            MSE[indH] += (yhat - y64[i]) ** 2
            points.append({"h": float(h), "row": i, "sigma_iters": len(solves), "sigmas": sigmas, "sigma": sigma,
                           "margins": margins, "score_gap": score_gap, "solves": solves, "beta": b, "S": S,
                           "order": np.array(beta.nzval2ind), "refit": coef, "kappa": kappa, "yhat": yhat,
                           "xrow": eX64[i].copy(), "screen": S0})
    return MSE, points
