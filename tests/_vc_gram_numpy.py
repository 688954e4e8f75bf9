"""The yardstick of cdh_vc_gram: the expanded design by `_vc_numpy.expand`, the kernel weights by `_vc_numpy.weights`, and
eX' diag(ω) eX, eX' diag(ω) y formed in long double (reference src/varying_coefficient_lasso.jl:572-647 computes the same
two objects loop by loop; tests/test_vc_gram_host.py pins this file to a restatement of those loops and to the Kronecker
identity of the reference's own test).  Also here: the launch arithmetic of csrc/vc_gram_types.hpp restated in Python from
the header's own constants, which tests/test_vc_gram_host.py holds to the compiled header."""
import os
import re

import numpy as np

from _vc_numpy import expand, weights

LD = np.longdouble
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coordinatedescent.jl_amd", "csrc")


def expanded(X, z, z0, degree, cols=None):
    """The expanded design of the listed base columns in long double: d = z - z0 is formed in the data's type (what the
    device does), the powers and products are exact to long double.  -> eX (n x mb (degree + 1))."""
    T = X.dtype.type
    d = (z - T(z0)).astype(X.dtype)
    Xs = X if cols is None else X[:, np.asarray(cols)]
    return expand(np.asfortranarray(Xs.astype(LD)), d.astype(LD), 0.0, degree)


def omega(kind, h, z, z0, wpow=1, e=None, leave_out=None):
    """ω_i = K(z_i, z0)^wpow e_i in long double from the kernel values rounded once to the data's type; 0 at the left-out row."""
    om = weights(kind, h, z, z0).astype(LD) ** wpow
    if e is not None:
        om = om * e.astype(LD)
    if leave_out is not None:
        om[leave_out] = 0
    return om


def gram(X, z, y, z0, degree, kind, h, wpow=1, e=None, leave_out=None, cols=None, acc=LD):
    """-> (G, c, Σω, Σ|terms of G|, Σ|terms of c|).  With a left-out row z0 is z[row] as stored.  `acc` is the type the sums
    are taken in: long double, or float64 where the caller has made every product and partial sum exactly representable."""
    if leave_out is not None:
        z0 = float(z[leave_out])
    eX = expanded(X, z, z0, degree, cols).astype(acc)
    om = omega(kind, h, z, z0, wpow, e, leave_out).astype(acc)
    yl = y.astype(acc)
    wX = om[:, None] * eX
    G, c = eX.T @ wX, wX.T @ yl
    aG, ac = np.abs(eX).T @ np.abs(wX), np.abs(wX).T @ np.abs(yl)
    return G, c, om.sum(), aG, ac


# ---- csrc/vc_gram_types.hpp, restated from its own constants -----------------------------------------------------------------
def constants():
    txt = open(os.path.join(CSRC, "vc_gram_types.hpp")).read()
    out = {}
    for name in ("kVgMaxCols", "kVgMaxDegree", "kVgRows", "kVgTile", "kVgThreads", "kVgMaxBlocks"):
        out[name] = int(re.search(r"constexpr int %s = (\d+);" % name, txt).group(1))
    out["kVgPartialDoubles"] = 1 << int(re.search(r"kVgPartialDoubles = \(int64_t\)1 << (\d+);", txt).group(1))
    return out


K = constants()


def nrec(Q, mb):
    return (2 * Q + 1) * (mb * (mb + 1) // 2) + (Q + 1) * mb + 1


def launch(n, Q, mb):
    """What a cdh_vc_gram call over n rows runs: chunks of rows, workgroups G, tile pairs, slices S, and the chain length L."""
    R, TL = K["kVgRows"], K["kVgTile"]
    groups = -(-(mb + 2) // TL)
    pairs = groups * (groups + 1) // 2
    S = min(K["kVgThreads"] // pairs, R)
    chunks = -(-n // R)
    fit = K["kVgPartialDoubles"] // nrec(Q, mb)
    G = max(1, min(chunks, K["kVgMaxBlocks"], fit))
    L = -(-chunks // G) * -(-R // S) + S + -(-G // 4) + 2
    return {"chunks": chunks, "G": G, "groups": groups, "pairs": pairs, "S": S, "L": L,
            "wraps": chunks > G, "capped_by_blocks": G == K["kVgMaxBlocks"] and chunks > G,
            "capped_by_buffer": G == fit and chunks > G, "ragged": n % R != 0}
