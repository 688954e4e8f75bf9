"""The case tables of the GLM steps and solves where weights clamp and exp saturates: what tests/test_glm_extremes_host.py pins
on the CPU and tests/test_gpu_glm_extremes.py runs on the device.  Nothing in here needs a GPU.

eta is INJECTED, not fitted: with p = 2, column 1 of X holding the wanted values and the iterate (1.0, 0), initialize! leaves
r = 0 - eta 1 and y = 0 in the handle, so the kernel's eta = y - r is the table's value bit for bit (every GPU case asserts
it).  For the Poisson family the same eta is placed three ways: through X (offset 0), through the offset (X beta = 0), and by
cancellation (X beta = +800, o = fl(-800 + c): the kernel's 800 + o is then the c the table lists, after that one rounding).

A table is cycled over the rows of a shape from a start chosen so that row n - 1 and the first row of the second tile hold
saturated entries; a shape shorter than the table runs from several starts that cover it between them."""
import numpy as np

import _glm_plan as GP

U = 2.0 ** -53
TINY = 2.0 ** -1074                          # the spacing of the subnormal range
WMIN = 2.0 ** -17                            # a power of two: e / WMIN and -mu / WMIN are exact, so r gives the device's exp back

# (n, grid cap, the branch of the plan the shape is named for)
SHAPES = [(33, GP.MAX_GRID, "one short tile"), (GP.ROWS + 1, GP.MAX_GRID, "two workgroups"), (2 * GP.ROWS + 1, 2, "second stride")]


def reaches(n, cap, branch):
    pl = GP.plan(n, cap)
    want = {"one short tile": pl["tiles"] == 1 and pl["grid"] == 1 and pl["ld"] - n == 31 and n % GP.VEC == 1,
            "two workgroups": pl["grid"] == 2 and pl["strides"] == 1,
            "second stride": pl["grid"] == cap and pl["strides"] == 2 and pl["tiles"] == cap + 1}[branch]
    assert want, (n, cap, branch, pl)
    return pl


# ---- the binomial table ----------------------------------------------------------------------------------------------------------
def clamp_boundary(wmin=WMIN):
    """The eta > 0 at which e / (1 + e)^2 == wmin, e = exp(-eta): e = (1 - 2 wmin - sqrt(1 - 4 wmin)) / (2 wmin), written
    without the cancellation as 2 wmin / (1 - 2 wmin + sqrt(1 - 4 wmin))."""
    e = 2.0 * wmin / (1.0 - 2.0 * wmin + np.sqrt(1.0 - 4.0 * wmin))
    return float(-np.log(e))


B_EDGE = clamp_boundary()
# two values on either side of the boundary: the twin's w_raw is off wmin by about 1e-3 and 1e-7 relative there, the
# device's by at most 64 ulp = 7e-15 more
B_NEAR = (B_EDGE - 1e-3, B_EDGE - 1e-7, B_EDGE + 1e-7, B_EDGE + 1e-3)
B_ETAS = (0.0, 1e-300,                       # centre and tiny predictor
          36.0, 36.7, 37.5,                  # on either side of where 1 + e rounds to 1 (e = 2^-53 at 36.7368)
          40.0) + B_NEAR + (                 # p rounds to 1 exactly; the clamp boundary (here, so that no 33 rows are all tame)
          708.0, 708.4, 709.0,               # e leaves the normal range (2^-1022 = exp(-708.3964))
          740.0, 744.44, 745.0, 745.13,      # subnormal e
          746.0, 800.0)                      # e == 0
B_LABELS = (0.0, 1.0, 0.25)
B_SAT = 36.0                                 # |eta| from here on counts as saturated


def binomial_table():
    """-> (eta, label), one row per entry: every eta with both signs (0 once) and every label."""
    eta, lab = [], []
    for a in B_ETAS:
        for s in ((1.0,) if a == 0.0 else (1.0, -1.0)):
            for l in B_LABELS:
                eta.append(s * a)
                lab.append(l)
    return np.array(eta), np.array(lab)


# ---- the Poisson table -----------------------------------------------------------------------------------------------------------
# (tame and saturated values alternate, and eta_max and its successor go in the middle, so that no 33 rows are all tame)
P_ETAS = (0.0, 300.0, 1.25, -300.0, -1.25, 700.0, -20.0, -700.0, 745.0, -745.0, -746.0, -800.0)
P_COUNTS = (0.0, 1.0, 3.0, 1e300)            # (count = 1 at eta = 0 is the row with dev == 0 and r == 0 exactly)
P_ETA_MAX = (50.0, 700.0)
PLACES = ("X", "offset", "cancel")
CANCEL = 800.0
P_SAT = 300.0


def poisson_table(eta_max):
    """-> (eta, count, place, eta_lin, offset), one row per entry, the three placements of a (eta, count) pair adjacent.  eta is
    what the kernel's eta_lin + offset comes to: the listed value, or for "cancel" fl(800 + fl(-800 + listed))."""
    etas = P_ETAS[:8] + (eta_max, float(np.nextafter(eta_max, np.inf))) + P_ETAS[8:]
    eta, cnt, place, lin, off = [], [], [], [], []
    for c in etas:
        for y in P_COUNTS:
            for pl in range(len(PLACES)):
                l, o = ((c, 0.0), (0.0, c), (CANCEL, -CANCEL + c))[pl]
                eta.append(l + o)
                cnt.append(y)
                place.append(pl)
                lin.append(l)
                off.append(o)
    return np.array(eta), np.array(cnt), np.array(place), np.array(lin), np.array(off)


# ---- a table over the rows of a shape -------------------------------------------------------------------------------------------
def starts(sat, n):
    """The starts from which a table of len(sat) entries is cycled over n rows, entry (start + i) % T in row i: row n - 1, and
    row GP.ROWS where there is one, hold saturated entries, and the starts cover the table between them."""
    T = len(sat)

    def ok(s):
        return sat[(s + n - 1) % T] and (n <= GP.ROWS or sat[(s + GP.ROWS) % T])

    out, covered = [], 0                     # entries [0, covered) are covered
    while covered < T:
        s = covered
        while not ok(s % T):                 # back up: the overlap only repeats entries
            s -= 1
            assert s > covered - n, "no admissible start"
        if s % T not in out:
            out.append(s % T)
        covered = s + n
    return out


def entries(T, n, start):
    return (start + np.arange(n)) % T


def cases(T_sat):
    """-> [(n, cap, branch, start)] over SHAPES for a table whose saturated entries are T_sat."""
    return [(n, cap, branch, s) for n, cap, branch in SHAPES for s in starts(T_sat, n)]


def case_id(c):
    return "n%d-cap%d-from%d" % (c[0], c[1], c[3])


B_TABLE = binomial_table()
B_CASES = cases(np.abs(B_TABLE[0]) >= B_SAT)
P_TABLES = {em: poisson_table(em) for em in P_ETA_MAX}
P_CASES = {em: cases(np.abs(P_TABLES[em][0]) >= P_SAT) for em in P_ETA_MAX}


def design(eta_lin, seed):
    """X (n x 2, Fortran order): column 1 the wanted X beta, column 2 small normals; the iterate is (1.0, 0)."""
    n = len(eta_lin)
    X = np.empty((n, 2), order="F")
    X[:, 0] = eta_lin
    X[:, 1] = 1e-3 * np.random.default_rng(seed).standard_normal(n)
    return X


def third(n):
    """A third of the rows, moving through the residues so that it meets every label and placement of a cycled table: row
    3 a + b is in it when (a + b) % 3 == 1."""
    i = np.arange(n)
    return (i + i // 3) % 3 == 1


# ---- the hard data of the solves -------------------------------------------------------------------------------------------------
N_SOLVE, P_SOLVE = 300, 10


def separable_data():
    """Linearly separable labels: default_rng(11), X standard normal, y = [X_0 + 0.5 X_1 > 0]."""
    rng = np.random.default_rng(11)
    X = np.asfortranarray(rng.standard_normal((N_SOLVE, P_SOLVE)))
    y = (X[:, 0] + 0.5 * X[:, 1] > 0.0).astype(np.float64)
    return X, y


def exposure_data():
    """Counts with tiny and large exposures: default_rng(21), X, beta* = (0.5, -0.4, 0.3, 0, ...), o = log U(0.5, 2) with
    o[::5] -= 16 and o[1::10] += 4, y ~ Poisson(exp(0.3 + X beta* + o)); drawn in the order X, exposures, counts."""
    rng = np.random.default_rng(21)
    X = np.asfortranarray(rng.standard_normal((N_SOLVE, P_SOLVE)))
    bstar = np.zeros(P_SOLVE)
    bstar[:3] = (0.5, -0.4, 0.3)
    o = np.log(rng.uniform(0.5, 2.0, N_SOLVE))
    o[::5] -= 16.0
    o[1::10] += 4.0
    y = rng.poisson(np.exp(0.3 + X @ bstar + o)).astype(np.float64)
    return X, y, o


# name -> (family, lambda / lambda_max, intercept fitted?, IRLS settings beyond the defaults)
SOLVES = {"separable-0.01": ("binomial", 0.01, False, {}),
          "separable-0.002": ("binomial", 0.002, False, {}),
          "exposures": ("poisson", 0.1, False, {}),
          "exposures-b": ("poisson", 0.1, True, {}),
          "capped": ("poisson", 0.1, False, dict(etaMax=4.0, maxIter=3, optTol=0.0)),
          "capped-b": ("poisson", 0.1, True, dict(etaMax=4.0, maxIter=3, optTol=0.0))}
INNER_TOL, IRLS_TOL, SOLVE_WMIN = 1e-12, 1e-10, 1e-5
_TWIN = {}


def twin_solve(name, randomize=False):
    """The twin's answer for a solve, computed once: dict(X, y, o, lam, icpt, irls (the IRLSOptions fields), beta, b0, rounds,
    converged, rise, monotone, clamped, capped (at the final beta), eta (the linear predictor there, without the offset)).
    monotone restates the front end's rule -- F rose between two rounds by more than 1e-10 max(1, F before) -- as
    rise <= 1e-10: tests/test_glm_extremes_host.py holds every rise to be below 1e-12 or far above 1e-10 max(1, |F|)."""
    key = (name, randomize)
    if key in _TWIN:
        return _TWIN[key]
    import oracle as O
    import _logistic_numpy as LG
    import _poisson_numpy as PN
    family, frac, icpt, extra = SOLVES[name]
    irls = dict(maxIter=25, optTol=IRLS_TOL, wmin=SOLVE_WMIN, etaMax=50.0)
    irls.update(extra)
    opts = O.CDOptions(maxIter=100000, optTol=INNER_TOL, randomize=randomize)
    if family == "binomial":
        X, y = separable_data()
        o = None
        lam = frac * LG.lambda_max(X, y)
        b, b0, rounds, conv, rise = LG.logistic_lasso(X, y, lam, None, opts, irls["maxIter"], irls["optTol"], irls["wmin"])
        eta = X @ b
        clamped, capped = int(LG.rows(y, eta, irls["wmin"])[4].sum()), 0
    else:
        X, y, o = exposure_data()
        lam = frac * PN.lambda_max(X, y, o, intercept=icpt)
        b, b0, rounds, conv, rise = PN.poisson_lasso(X, y, o, lam, None, opts, irls["maxIter"], irls["optTol"], irls["wmin"],
                                                     irls["etaMax"], intercept=icpt)
        eta = (PN.with_ones(X) @ np.r_[b, b0]) if icpt else X @ b
        rows = PN.rows(y, eta, o, irls["wmin"], irls["etaMax"])
        clamped, capped = int(rows[5].sum()), int(rows[6].sum())
    _TWIN[key] = dict(X=X, y=y, o=o, lam=lam, icpt=icpt, irls=irls, beta=b, b0=b0, rounds=rounds, converged=conv, rise=rise,
                      monotone=bool(rise <= 1e-10), clamped=clamped, capped=capped, eta=eta, family=family)
    return _TWIN[key]
