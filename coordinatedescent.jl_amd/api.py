"""Host-side mirror of CoordinateDescent.jl's interface for the hot path, over the
C-ABI of the HIP library (include/cdhip.h).

The reference is Julia and no Julia toolchain exists in this image, so this mirror
is Python (julia/CoordinateDescentHIP.jl holds the thin ccall binding a Julia
maintainer would add).  Names, argument meaning and error behaviour follow the
reference: `coordinateDescent!` is `coordinateDescent_`, and so on (a trailing
underscore stands for Julia's `!`).  Coordinates are 1-based, as in the reference.
All arithmetic of the path runs in the HIP library; nothing here computes on the
CPU beyond the O(p) bookkeeping the reference also does on the host.

Reference files mirrored (relative to the reference's src/):
  utils.jl:7-39                      CDOptions, IterLassoOptions
  cd_differentiable_function.jl      the loss operators and the 4-function plugin API
  coordinate_descent.jl              coordinateDescent!, _findLambdaMax
  atom_iterator.jl                   OrderedIterator, RandomIterator
  lasso.jl                           lasso, sqrtLasso, scaledLasso!, feasibleLasso!, LassoPath, refitLassoPath
  varying_coefficient_lasso.jl       the smoothing kernels, locpolyl1, lvocv_locpolyl1, get_nonzero_coordinates
  ProximalBase 0.3.0 (not vendored)  ProxL1, SparseIterate (contract: SURVEY.md App. B)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import (ArgumentError, DimensionMismatch, DomainError, HipError,  # noqa: F401
                   CDH_F32, CDH_F64, CDH_LS, CDH_SQRT, CDH_WLS, CDH_SWEEP_BLOCK, CDH_SWEEP_COORD,
                   CDH_VC_EPANECHNIKOV, CDH_VC_GAUSSIAN,
                   cdh_options, cdh_stats, check)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# --------------------------------------------------------------------------------------
# Options (src/utils.jl:7-39)
# --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class CDOptions:
    """CDOptions(;maxIter=2000, optTol=1e-7, randomize=true, warmStart=true, numSteps=50)
    (src/utils.jl:7-20).  `seed` seeds the documented substitute for Julia's global RNG
    used by RandomIterator (src/atom_iterator.jl:60)."""
    maxIter: int = 2000
    optTol: float = 1e-7
    randomize: bool = True
    warmStart: bool = True
    numSteps: int = 50
    seed: int = 0

    def _c(self):
        return cdh_options(int(self.maxIter), float(self.optTol), int(bool(self.randomize)),
                           int(bool(self.warmStart)), int(self.numSteps), int(self.seed))


@dataclass(frozen=True)
class IterLassoOptions:
    """IterLassoOptions (src/utils.jl:24-39); initProcedure in {"Screening","InitStd","WarmStart"}."""
    maxIter: int = 20
    optTol: float = 1e-2
    initProcedure: str = "Screening"
    sinit: int = 5
    sigmainit: float = 1.0
    optionsCD: CDOptions = field(default_factory=CDOptions)


# --------------------------------------------------------------------------------------
# ProximalBase: ProxL1, SparseIterate
# --------------------------------------------------------------------------------------
class ProxL1:
    """ProxL1(λ0) / ProxL1(λ0, λ::AbstractArray): fields lambda0 and lam (None = unweighted)."""

    def __init__(self, lambda0, lam=None):
        self.lambda0 = float(lambda0)
        self.lam = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64).copy()


class SparseIterate:
    """SparseIterate(p): dense-indexable iterate with an insertion-ordered support
    (nzval2ind[1:nnz]); zeros written to stored coordinates keep their slot until
    dropzeros_ (test/atom_iterator.jl:13-28)."""

    def __init__(self, p, values=None):
        if isinstance(p, np.ndarray):
            values, p = p, p.shape[0]
        self.p = int(p)
        self._val = np.zeros(self.p)
        self._slot2ind = np.zeros(self.p, dtype=np.int64)
        self._ind2slot = np.zeros(self.p, dtype=np.int64)
        self._nnz = 0
        self._version = 0
        if values is not None:
            for k, v in enumerate(np.asarray(values, dtype=np.float64)):
                if v != 0.0:
                    self[k + 1] = v

    # -- AbstractArray surface ---------------------------------------------------------
    def __len__(self):
        return self.p

    def __getitem__(self, k1):
        s = self._ind2slot[k1 - 1]
        return float(self._val[s - 1]) if s else 0.0

    def __setitem__(self, k1, v):
        k = int(k1) - 1
        if not 0 <= k < self.p:
            raise IndexError(k1)
        v = float(v)
        s = self._ind2slot[k]
        self._version += 1
        if s:
            self._val[s - 1] = v
        elif v != 0.0:
            self._val[self._nnz] = v
            self._slot2ind[self._nnz] = k
            self._nnz += 1
            self._ind2slot[k] = self._nnz

    @property
    def nnz(self):
        return self._nnz

    @property
    def nzval2ind(self):
        """1-based support in insertion order."""
        return self._slot2ind[: self._nnz] + 1

    @property
    def nzval(self):
        return self._val[: self._nnz].copy()

    def dense(self):
        out = np.zeros(self.p)
        out[self._slot2ind[: self._nnz]] = self._val[: self._nnz]
        return out

    __array__ = lambda self, dtype=None, copy=None: self.dense()  # noqa: E731  Vector(x)

    def __eq__(self, other):
        return isinstance(other, SparseIterate) and self.p == other.p and \
            np.array_equal(self.dense(), other.dense())

    def fill_(self, v=0.0):
        """fill!(x, 0) empties the iterate."""
        if v != 0.0:
            raise ArgumentError("only fill!(x, 0) is used on this path")
        self._ind2slot[self._slot2ind[: self._nnz]] = 0
        self._nnz = 0
        self._version += 1

    def dropzeros_(self):
        """dropzeros!(x): swap-with-last compaction (order unpinned by the reference's tests)."""
        i = 0
        while i < self._nnz:
            if self._val[i] == 0.0:
                self._ind2slot[self._slot2ind[i]] = 0
                last = self._nnz - 1
                if i != last:
                    self._val[i] = self._val[last]
                    self._slot2ind[i] = self._slot2ind[last]
                    self._ind2slot[self._slot2ind[i]] = i + 1
                self._nnz -= 1
            else:
                i += 1
        self._version += 1

    def copy(self):
        y = SparseIterate(self.p)
        y._val[:] = self._val
        y._slot2ind[:] = self._slot2ind
        y._ind2slot[:] = self._ind2slot
        y._nnz = self._nnz
        return y

    # -- sync with a device handle -------------------------------------------------------
    def _load(self, idx1, val):
        self._ind2slot[:] = 0
        n = len(idx1)
        self._slot2ind[:n] = np.asarray(idx1, dtype=np.int64) - 1
        self._val[:n] = val
        self._ind2slot[self._slot2ind[:n]] = np.arange(1, n + 1)
        self._nnz = n
        self._version += 1


def numCoordinates(obj):
    """numCoordinates(f) / ProximalBase.numCoordinates(x)."""
    return obj.p


# --------------------------------------------------------------------------------------
# Loss operators = the plugin API (src/cd_differentiable_function.jl)
# --------------------------------------------------------------------------------------
class CoordinateDifferentiableFunction:
    """abstract type CoordinateDifferentiableFunction (src/cd_differentiable_function.jl:1)."""


class _HipLoss(CoordinateDifferentiableFunction):
    """A loss whose X, y, r live in HBM behind one cdh_handle."""
    _kind = CDH_LS

    def __init__(self, y, X, w=None, *, device=0, n_total=None, row_offset=0):
        X = np.asarray(X)
        y = np.asarray(y)
        if X.dtype not in (np.float64, np.float32) or y.dtype != X.dtype or X.ndim != 2:
            raise TypeError("MethodError: y::AbstractVector{T}, X::AbstractMatrix{T}, T<:AbstractFloat")
        if y.shape[0] != X.shape[0]:  # cd_differentiable_function.jl:53,212
            raise DimensionMismatch("length(y) != size(X, 1)")
        if w is not None and np.asarray(w).shape[0] != X.shape[0]:  # :129
            raise DimensionMismatch("length(w) != size(X, 1)")
        n, p = X.shape
        self._create(X.dtype, n, p, device, n_total, row_offset)
        step = max(1, (64 << 20) // max(1, n * X.itemsize))
        for j0 in range(0, p, step):
            blk = np.asfortranarray(X[:, j0:j0 + step])
            check(self._L.cdh_set_X_cols(self._h, j0, blk.shape[1], _vp(blk), n), self._h)
        yy = np.ascontiguousarray(y)
        check(self._L.cdh_set_y(self._h, _vp(yy)), self._h)
        if w is not None:
            ww = np.ascontiguousarray(w, dtype=X.dtype)
            check(self._L.cdh_set_obs_weights(self._h, _vp(ww)), self._h)

    def _create(self, dtype, n, p, device, n_total, row_offset):
        self._L = _lib.lib()
        self.dtype = np.dtype(dtype)
        self.n, self.p = int(n), int(p)
        self.n_total = int(n if n_total is None else n_total)
        self.row_offset = int(row_offset)
        h = C.c_void_p()
        st = self._L.cdh_create(C.byref(h), CDH_F64 if self.dtype == np.float64 else CDH_F32,
                                self._kind, self.n, self.n_total, self.row_offset, self.p, int(device))
        check(st, None)
        self._h = h
        self._synced = None  # (id(x), version) of the iterate the handle currently mirrors
        self._penalty = None
        self.last_stats = None

    @classmethod
    def generate(cls, n, p, *, seed=123, s=0, noise=1.0, dtype=np.float64, device=0, n_total=None,
                 row_offset=0):
        """Synthetic Gaussian problem generated on the device (benchmark/cd_bench.jl:8-14
        shapes); returns (loss, planted beta*)."""
        self = cls.__new__(cls)
        self._create(dtype, n, p, device, n_total, row_offset)
        bstar = np.zeros(max(int(s), 1))
        check(self._L.cdh_generate(self._h, int(seed), int(s), float(noise), _vp(bstar)), self._h)
        return self, bstar[: int(s)]

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.cdh_destroy(self._h)
                self._h = None
        except Exception:
            pass

    close = __del__

    # -- data views ------------------------------------------------------------------------
    @property
    def r(self):
        """f.r: the residual vector (copied from HBM)."""
        out = np.zeros(self.n, dtype=self.dtype)
        check(self._L.cdh_get_residual(self._h, _vp(out)), self._h)
        return out

    @property
    def y(self):
        out = np.zeros(self.n, dtype=self.dtype)
        check(self._L.cdh_get_y(self._h, _vp(out)), self._h)
        return out

    @property
    def w(self):
        """f.w: the observation weights of a weighted loss (copied from HBM)."""
        out = np.zeros(self.n, dtype=self.dtype)
        check(self._L.cdh_get_obs_weights(self._h, _vp(out)), self._h)
        return out

    def X_cols(self, j0, ncols):
        """Columns [j0, j0+ncols) (0-based bulk helper) copied back from HBM."""
        out = np.zeros((self.n, ncols), dtype=self.dtype, order="F")
        check(self._L.cdh_get_X_cols(self._h, int(j0), int(ncols), _vp(out), self.n), self._h)
        return out

    # -- execution control -----------------------------------------------------------------
    def set_sweep_mode(self, mode, block=32):
        mode = {"coord": CDH_SWEEP_COORD, "block": CDH_SWEEP_BLOCK}.get(mode, mode)
        check(self._L.cdh_set_sweep_mode(self._h, int(mode), int(block)), self._h)

    def set_screening(self, on=True):
        """0 / False: never; 1 / True: full passes of the solves (default); 2: cdPass_ as well."""
        check(self._L.cdh_set_screening(self._h, int(on)), self._h)

    def set_gradient_cache(self, mode=1):
        """0 off, 1 rent-or-buy (default), 2 from the first full pass, 3 = 2 without the tall-problem guard."""
        check(self._L.cdh_set_gradient_cache(self._h, int(mode)), self._h)

    def set_onchip_solve(self, on=True):
        """One-launch solves of problems that fit on chip (cdh_set_onchip_solve; on by default)."""
        check(self._L.cdh_set_onchip_solve(self._h, int(bool(on))), self._h)

    def onchip_stats(self):
        out = (C.c_int64 * 2)()
        check(self._L.cdh_onchip_stats(self._h, out), self._h)
        return {"solves": int(out[0]), "gram_matrices": int(out[1])}

    def onchip_last(self):
        """Of the last one-launch solve: visit steps, kernel time in microseconds, the clock (GHz) the chip held."""
        out = (C.c_int64 * 3)()
        check(self._L.cdh_onchip_last(self._h, out), self._h)
        return {"steps": int(out[0]), "kernel_us": out[2] / 100.0, "clock_GHz": (out[1] / out[2] * 0.1) if out[2] else 0.0}

    def gradient_cache_mode(self):
        out = C.c_int32()
        check(self._L.cdh_get_gradient_cache(self._h, C.byref(out)), self._h)
        return out.value

    def cache_drift(self, rereference_now=False):
        """max_k |g_carried - X_k'r| / thr_k at the gradient cache's re-references (cdh_cache_drift); with
        rereference_now the carried gradient is taken afresh from X first (one dots-only pass) and measured."""
        out = (C.c_double * 3)()
        check(self._L.cdh_cache_drift(self._h, int(bool(rereference_now)), out), self._h)
        return {"last": out[0], "max": out[1], "measured": int(out[2])}

    def cache_stats(self):
        out = (C.c_int64 * 10)()
        check(self._L.cdh_cache_stats(self._h, out), self._h)
        return dict(zip(("passes", "settled_visits", "exact_visits", "reference_passes", "gram_batches", "gram_columns",
                         "covariance_visits", "residual_catchups", "rollbacks", "device_passes"), [int(v) for v in out]))

    def cache_gram_column(self, k):
        """(X'X_k as the gradient cache holds it, the relative error its entries are declared to carry); k 1-based."""
        out, eps = np.zeros(self.p), C.c_double()
        check(self._L.cdh_cache_gram_column(self._h, int(k), _vp(out), C.byref(eps)), self._h)
        return out, eps.value

    def set_device_loop(self, on=True, helpers=None):
        """The pass loop of a cache-served solve on the device (cdh_set_device_loop; on by default).  helpers: 0 keeps the
        loop to one workgroup (large visit lists then run from its Gram table only), n > 2 sets the number of helper
        workgroups a launch that expects large visit lists brings (default 31)."""
        v = int(bool(on))
        if on and helpers is not None:
            v = 2 if int(helpers) == 0 else max(3, int(helpers))
        check(self._L.cdh_set_device_loop(self._h, v), self._h)

    def device_loop_stats(self):
        out = (C.c_int64 * 12)()
        check(self._L.cdh_device_loop_stats(self._h, out), self._h)
        d = dict(zip(("launches", "passes", "folds", "exact_rechecks"), [int(x) for x in out[:4]]))
        d["phase_us"] = dict(zip(("list", "scan", "exact_g", "visits", "recheck", "accept", "bookkeeping", "dropzeros_rest"),
                                 [int(x) / 100.0 for x in out[4:]]))
        t = (C.c_int64 * 8)()
        check(self._L.cdh_device_loop_table(self._h, t), self._h)
        d["table"] = dict(zip(("passes", "rows_filled", "coordinates", "capacity"), [int(x) for x in t[:4]]))
        d["forced_rounds"] = {"host_pass": int(t[4]), "loop": int(t[5])}
        d["crew"] = {"passes": int(t[6]), "jobs": int(t[7])}
        return d

    def set_use_graph(self, on=True):
        check(self._L.cdh_set_use_graph(self._h, int(bool(on))), self._h)

    def comm_init(self, unique_id: bytes, rank: int, nranks: int):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(self._L.cdh_comm_init(self._h, buf, int(rank), int(nranks)), self._h)

    def comm_drop(self):
        """Give the RCCL communicator up so that another exchange can be installed (cdh_comm_drop)."""
        check(self._L.cdh_comm_drop(self._h), self._h)

    def p2p_local_handle(self) -> bytes:
        buf = C.create_string_buffer(64)
        check(self._L.cdh_p2p_local_handle(self._h, buf), self._h)
        return buf.raw

    def p2p_connect(self, handles: bytes, rank: int, nranks: int):
        if len(handles) != 64 * int(nranks):
            raise ArgumentError("p2p_connect needs 64 bytes per rank")
        buf = C.create_string_buffer(bytes(handles), len(handles))
        check(self._L.cdh_p2p_connect(self._h, buf, int(rank), int(nranks)), self._h)

    def p2p_enable(self, on=True):
        check(self._L.cdh_p2p_enable(self._h, int(bool(on))), self._h)

    def set_host_exchange(self, fn, rank, nranks):
        """Bring-your-own transport: `fn(array_of_doubles)` must sum the array in place over all ranks
        (cdh_set_host_exchange).  The ctypes trampoline is kept alive on the loss."""
        if fn is None:
            check(self._L.cdh_set_host_exchange(self._h, _lib.HOST_ALLREDUCE_FN(0), None, 0, 1), self._h)
            self._host_cb = None
            return

        def tramp(_user, ptr, count):
            try:
                fn(np.ctypeslib.as_array(ptr, shape=(count,)))
                return 0
            except Exception:      # nothing may unwind into the library
                return 1
        cb = _lib.HOST_ALLREDUCE_FN(tramp)
        check(self._L.cdh_set_host_exchange(self._h, cb, None, int(rank), int(nranks)), self._h)
        self._host_cb = cb

    def exchange_stats(self):
        """All-reduces issued through each exchange so far, and the rank count the active one reports."""
        a, b, c, n = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        check(self._L.cdh_exchange_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)), self._h)
        return {"rccl_calls": a.value, "p2p_calls": b.value, "host_calls": c.value, "nranks": n.value}

    def exchange_probe(self, values):
        """All-reduce (sum) up to 4096 doubles through the active exchange; returns the sums."""
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        check(self._L.cdh_exchange_probe(self._h, v.ctypes.data_as(C.c_void_p), v.size), self._h)
        return v

    def exchange_latency(self, count, iters=200):
        """Average microseconds per all-reduce of `count` doubles through the active exchange (collective)."""
        out = C.c_double()
        check(self._L.cdh_exchange_latency(self._h, int(count), int(iters), C.byref(out)), self._h)
        return out.value

    def profile_begin(self):
        check(self._L.cdh_profile_begin(self._h), self._h)

    def profile_end(self):
        ms, nl, by = C.c_double(), C.c_int64(), C.c_double()
        check(self._L.cdh_profile_end(self._h, C.byref(ms), C.byref(nl), C.byref(by)), self._h)
        return ms.value, nl.value, by.value

    # -- cross-validation folds (cdh_set_folds, cdh_set_fold_weights, cdh_path_sse) ---------
    def set_folds(self, folds, K):
        """Keep the 0-based fold id of every row on the device (folds=None: drop them); returns the fold sizes."""
        if folds is None:
            check(self._L.cdh_set_folds(self._h, None, 0, None), self._h)
            return None
        ids = np.ascontiguousarray(folds, dtype=np.int32)
        if ids.shape != (self.n,):
            raise ArgumentError("folds must hold one id per row")
        count = np.zeros(max(int(K), 1), dtype=np.int64)
        check(self._L.cdh_set_folds(self._h, _vp(ids), int(K), _vp(count)), self._h)
        return count

    def set_fold_weights(self, k):
        """f.w = (fold != k) written on the device (k = -1: all ones); the handle is left as an upload of those weights
        would leave it."""
        check(self._L.cdh_set_fold_weights(self._h, int(k)), self._h)
        self._synced = None

    def path_sse(self, k, idx1, B, held=True, train=True):
        """Σ_i (y_i - Σ_t X[i, idx1[t]] B[t, j])² for every column j of B (len(idx1) x m) over the rows of fold k and over
        the other rows, in one pass over the listed columns (k = -1: every row is a training row).  Returns
        (held, train); an output that was not asked for is None.  Read-only on the handle."""
        idx1 = np.ascontiguousarray(idx1, dtype=np.int64)
        B = np.asfortranarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != idx1.shape[0]:
            raise DimensionMismatch("B must have one row per listed coordinate")
        s, m = B.shape
        oh = np.zeros(m) if held else None
        ot = np.zeros(m) if train else None
        check(self._L.cdh_path_sse(self._h, int(k), s, _vp(idx1), m, _vp(B), max(s, 1), _vp(oh), _vp(ot)), self._h)
        return oh, ot

    # -- sync helpers ----------------------------------------------------------------------
    def _set_penalty(self, g):
        if not isinstance(g, ProxL1):
            raise TypeError("MethodError: descendCoordinate! is defined for g::ProxL1 only")
        n_om = 0 if g.lam is None else g.lam.shape[0]
        check(self._L.cdh_set_penalty(self._h, g.lambda0, _vp(g.lam), n_om), self._h)

    def _push(self, x, rebuild):
        idx = np.ascontiguousarray(x.nzval2ind, dtype=np.int64)
        val = np.ascontiguousarray(x._val[: x.nnz], dtype=np.float64)
        fn = self._L.cdh_initialize if rebuild else self._L.cdh_set_iterate
        check(fn(self._h, len(x), x.nnz, _vp(idx), _vp(val)), self._h)
        self._synced = (id(x), x._version)

    def _ensure_synced(self, x):
        if self._synced != (id(x), x._version):
            self._push(x, rebuild=False)

    def _pull(self, x):
        if getattr(self, "_pull_idx", None) is None:      # (two p-sized host buffers, kept: a path pulls once per lambda)
            self._pull_idx, self._pull_beta = np.zeros(max(self.p, 1), dtype=np.int64), np.zeros(self.p)
        idx, beta = self._pull_idx, self._pull_beta
        nnz = C.c_int64()
        check(self._L.cdh_get_support(self._h, _vp(idx), C.byref(nnz)), self._h)
        check(self._L.cdh_get_beta(self._h, _vp(beta)), self._h)
        sup = idx[: nnz.value]
        x._load(sup, beta[sup - 1])
        self._synced = (id(x), x._version)


class CDLeastSquaresLoss(_HipLoss):
    """CDLeastSquaresLoss(y, X): |y - Xβ|²/(2n) (src/cd_differentiable_function.jl:43-111)."""
    _kind = CDH_LS


class CDSqrtLassoLoss(_HipLoss):
    """CDSqrtLassoLoss(y, X): |y - Xβ|₂ (src/cd_differentiable_function.jl:202-291)."""
    _kind = CDH_SQRT


class CDWeightedLSLoss(_HipLoss):
    """CDWeightedLSLoss(y, X, w): Σ w_i (y_i - X_iβ)²/(2n) (src/cd_differentiable_function.jl:118-194)."""
    _kind = CDH_WLS

    def __init__(self, y, X, w, **kw):
        super().__init__(y, X, w, **kw)


class _GLMLoss(CDWeightedLSLoss):
    """What CDLogisticLoss and CDPoissonLoss share: the upload of X in column chunks, the observations kept in a buffer of
    the handle's own beside the working response, and the objective read off a read-only step.  A family adds
    _set_observations (its export), irls_step with its own arguments, and _irls: that step as the IRLS loop calls it."""
    _objective_step = {}                 # the arguments of objective's read-only irls_step
    _has_weights = False                 # observation weights are set on the handle (cdh_glm_set_weights)

    def __init__(self, y, X, offset=None, *, weights=None, device=0):
        X = np.asarray(X)
        obs = np.ascontiguousarray(y, dtype=np.float64)
        off = None if offset is None else np.ascontiguousarray(offset, dtype=np.float64)
        if X.dtype != np.float64 or X.ndim != 2:
            raise TypeError("MethodError: %s takes X::AbstractMatrix{Float64}" % type(self).__name__)
        if obs.ndim != 1 or obs.shape[0] != X.shape[0]:
            raise DimensionMismatch("length(y) != size(X, 1)")
        if off is not None and off.shape != obs.shape:
            raise DimensionMismatch("length(offset) != size(X, 1)")
        n, p = X.shape
        v = _strata_weights(None, weights, n)[1]
        self._create(X.dtype, n, p, device, None, 0)
        step = max(1, (64 << 20) // max(1, n * X.itemsize))
        for j0 in range(0, p, step):
            blk = np.asfortranarray(X[:, j0:j0 + step])
            check(self._L.cdh_set_X_cols(self._h, j0, blk.shape[1], _vp(blk), n), self._h)
        self._set_observations(obs, off)
        if v is not None:
            check(self._L.cdh_glm_set_weights(self._h, _vp(v)), self._h)
            self._has_weights = True

    def _get_weights(self):
        """The observation weights the handle holds (normalised to sum to n); ones when none were given."""
        out = np.zeros(self.n)
        check(self._L.cdh_glm_get_weights(self._h, _vp(out)), self._h)
        return out

    def _prior(self):
        """The observation weights of a loss made with them, None otherwise (no call is made then)."""
        return self._get_weights() if self._has_weights else None

    def _observations(self):
        out = np.zeros(self.n)
        check(self._L.cdh_glm_get_labels(self._h, _vp(out)), self._h)
        return out

    def objective(self, g=None):
        """F(β) = (the family's nll) + λ0 Σ ω_j |β_j| at the handle's iterate, read-only (apply=0)."""
        val = self.irls_step(apply=False, **self._objective_step)["nll"]
        if g is not None:
            beta = np.zeros(self.p)
            check(self._L.cdh_get_beta(self._h, _vp(beta)), self._h)
            val += g.lambda0 * float(np.sum(np.abs(beta) * (1.0 if g.lam is None else g.lam)))
        return val


class CDLogisticLoss(_GLMLoss):
    """CDLogisticLoss(y, X; weights=None): (1/n) Σ [log(1 + e^η_i) - y_i η_i], η = Xβ, labels y_i in [0, 1]; no reference counterpart.
    Minimised by IRLS: a round is the weighted lasso of CDWeightedLSLoss (src/cd_differentiable_function.jl:118-194) on the
    working response z and weights w, which the handle's y and w hold from one irls_step to the next; the labels live in a
    buffer of their own (cdh_glm_set_labels).  fp64 only, one device.

    weights (glmnet's weights =): v_i finite and > 0 -- case or survey weights, class re-balancing, the trials of a
    proportion label -- normalised HERE to sum to n (v n / Σv; the library stores what it is given), so that unit weights
    leave F as it was: F = (1/n) Σ v_i [log(1 + e^η_i) - y_i η_i].  A row's step is the unweighted one and its stored working
    weight v_i w_i (cdh_glm_set_weights): an integer weight reproduces a replicated row.  The penalty scales of the paths
    stay the reference's _stdX!, the root mean square over the rows present: they are NOT weighted by v."""
    _objective_step = {"wmin": 0.25}     # (the sum of nll does not depend on wmin)

    def __init__(self, y, X, *, weights=None, device=0):
        super().__init__(y, X, weights=weights, device=device)

    def _set_observations(self, labels, _):
        check(self._L.cdh_glm_set_labels(self._h, 0, _vp(labels)), self._h)

    labels = property(_GLMLoss._observations)
    weights = property(_GLMLoss._get_weights)

    def irls_step(self, apply=True, wmin=1e-5, fold=None):
        """One IRLS step at the iterate the handle holds (cdh_glm_irls).  apply=True turns the handle's y, w and r into the
        working response, the working weights (clamped below at wmin) and their residual; apply=False only reads.  Returns
        {"nll": (1/n) Σ nll_i, "sum_w": Σ w_i, "clamped": rows whose weight was clamped}.

        fold=k (cdh_glm_irls_fold, after set_folds): the rows of fold k are held out -- w = 0, z = η, r = 0 -- and the three
        sums run over the other rows; the dict gains "held_nll" = Σ nll_i and "held_miss" = Σ y_i [η_i <= 0] + (1 - y_i) [η_i > 0]
        over the held-out rows (sums, not means).  "nll" stays (1/n) Σ over the training rows: the handle's objective.

        On a loss with weights every sum but "clamped" is weighted by v: "nll" = (1/n) Σ v_i nll_i, "sum_w" = Σ v_i w_i,
        "held_nll" = Σ v_i nll_i and "held_miss" = Σ v_i miss_i."""
        po = C.POINTER(C.c_double)
        if fold is None:
            out = np.zeros(3)
            check(self._L.cdh_glm_irls(self._h, 1 if apply else 0, float(wmin), out.ctypes.data_as(po)), self._h)
            return {"nll": float(out[0]) / self.n, "sum_w": float(out[1]), "clamped": int(out[2])}
        out = np.zeros(5)
        check(self._L.cdh_glm_irls_fold(self._h, int(fold), 1 if apply else 0, float(wmin), out.ctypes.data_as(po)), self._h)
        return {"nll": float(out[0]) / self.n, "sum_w": float(out[1]), "clamped": int(out[2]),
                "held_nll": float(out[3]), "held_miss": float(out[4])}

    def _irls(self, apply, irls, fold):
        return self.irls_step(apply, irls.wmin, fold)


class CDPoissonLoss(_GLMLoss):
    """CDPoissonLoss(y, X, offset=None; weights=None): (1/n) Σ [μ_i - y_i η_i], η = Xβ + o, μ = e^η, counts y_i >= 0 and offsets o_i (log
    exposure); no reference counterpart.  Minimised by IRLS like CDLogisticLoss (a sibling, not a subclass of it): a round is
    the weighted lasso of CDWeightedLSLoss (src/cd_differentiable_function.jl:118-194) on the working response and weights
    the handle's y and w hold from one irls_step to the next.  The counts and the offset live in buffers of their own
    (cdh_glm_set_counts), and the stored working response leaves the offset out: f.y - f.r is Xβ.  fp64 only, one device.

    weights (glmnet's weights =): v_i finite and > 0 (frequency or survey weights), normalised HERE to sum to n (v n / Σv; the
    library stores what it is given): F = (1/n) Σ v_i [μ_i - y_i η_i].  A row's step is the unweighted one and its stored
    working weight v_i w_i (cdh_glm_set_weights).  The penalty scales of the paths are NOT weighted by v."""

    def __init__(self, y, X, offset=None, *, weights=None, device=0):
        super().__init__(y, X, offset, weights=weights, device=device)

    def _set_observations(self, counts, off):
        check(self._L.cdh_glm_set_counts(self._h, _vp(counts), _vp(off)), self._h)

    counts = property(_GLMLoss._observations)
    weights = property(_GLMLoss._get_weights)

    @property
    def offset(self):
        """The offsets (zeros when none was given)."""
        out = np.zeros(self.n)
        check(self._L.cdh_glm_get_offset(self._h, _vp(out)), self._h)
        return out

    def irls_step(self, apply=True, wmin=1e-5, eta_max=50.0, fold=None):
        """One IRLS step at the iterate the handle holds (cdh_glm_poisson_irls).  apply=True turns the handle's y, w and r into
        the working response (without the offset), the working weights (μ clamped below at wmin, η capped above at eta_max)
        and their residual; apply=False only reads.  Returns {"nll": (1/n) Σ [μ_i - y_i η_i], "sum_w": Σ w_i, "clamped": rows
        whose weight was clamped, "capped": rows whose η was capped, "deviance": Σ dev_i}, the sums over the training rows
        ("capped" over all rows).

        fold=k (after set_folds): the rows of fold k are held out -- w = 0, z = Xβ, r = 0 -- and the dict gains
        "held_deviance" = Σ dev_i over them (a sum, not a mean).

        On a loss with weights "nll", "sum_w", "deviance" and "held_deviance" are weighted by v ((1/n) Σ v_i nll_i, Σ v_i w_i,
        Σ v_i dev_i); "clamped" and "capped" stay row counts."""
        out = np.zeros(6)
        k = -1 if fold is None else int(fold)
        if k < 0 and fold is not None:
            raise ArgumentError("fold must be a fold id")
        check(self._L.cdh_glm_poisson_irls(self._h, k, 1 if apply else 0, float(wmin), float(eta_max),
                                           out.ctypes.data_as(C.POINTER(C.c_double))), self._h)
        res = {"nll": float(out[0]) / self.n, "sum_w": float(out[1]), "clamped": int(out[2]), "capped": int(out[3]),
               "deviance": float(out[5])}
        if fold is not None:
            res["held_deviance"] = float(out[4])
        return res

    def _irls(self, apply, irls, fold):
        return self.irls_step(apply, irls.wmin, irls.etaMax, fold)


def _survival3(y, n=None):
    """y = [time, status] (n x 2, glmnet's Surv matrix) or [start, stop, status] (n x 3, Surv(start, stop, status)) ->
    (start or None, time, status) as contiguous float64 vectors, time the stop time; refused on the host the way
    cdh_glm_set_survival and cdh_glm_set_survival_interval would refuse them.  One refusal is worded for this layer: a
    three-column y whose first column is not below its second is not an interval matrix at all -- what a [time, status, ...]
    matrix with a column too many looks like -- so it is a DimensionMismatch, as every other y that is not a Surv matrix is;
    the message names the row and the two values."""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 2 or y.shape[1] not in (2, 3):
        raise DimensionMismatch("y must be n x 2: [time, status], or n x 3: [start, stop, status]")
    if n is not None and y.shape[0] != n:
        raise DimensionMismatch("size(y, 1) != size(X, 1)")
    start = np.ascontiguousarray(y[:, 0]) if y.shape[1] == 3 else None
    time, status = np.ascontiguousarray(y[:, -2]), np.ascontiguousarray(y[:, -1])
    if not np.all(np.isfinite(time)):
        raise ArgumentError("time[%d] is not finite" % int(np.nonzero(~np.isfinite(time))[0][0]))
    bad = (status != 0.0) & (status != 1.0)
    if np.any(bad):
        raise ArgumentError("status[%d] is neither 0 (censored) nor 1 (event)" % int(np.nonzero(bad)[0][0]))
    if not np.any(status == 1.0):
        raise ArgumentError("no row is an event: the partial likelihood is constant")
    if start is not None:
        if not np.all(np.isfinite(start)):
            raise ArgumentError("start[%d] is not finite" % int(np.nonzero(~np.isfinite(start))[0][0]))
        bad = ~(start < time)
        if np.any(bad):
            i = int(np.nonzero(bad)[0][0])
            raise DimensionMismatch("y is n x 3 but not [start, stop, status]: start[%d] = %g is not below stop[%d] = %g"
                                    % (i, start[i], i, time[i]))
    return start, time, status


def _survival(y, n=None):
    """_survival3 without the start times: (time, status)."""
    return _survival3(y, n)[1:]


def _strata_weights(strata, weights, n):
    """strata -> contiguous int32 ids or None, weights -> float64 normalised to sum to n (v n / Σv) or None; refused on the
    host: a wrong length, ids that are not integers or do not fit int32, a weight that is not finite or not > 0."""
    if strata is not None:
        a = np.asarray(strata)
        if a.ndim != 1 or a.shape[0] != n:
            raise DimensionMismatch("length(strata) != size(X, 1)")
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.number) or np.iscomplexobj(a):
            raise ArgumentError("strata must be integers")
        if not np.issubdtype(a.dtype, np.integer):
            bad = ~(np.isfinite(a) & (a == np.floor(np.where(np.isfinite(a), a, 0.0))))
            if np.any(bad):
                raise ArgumentError("strata[%d] is not an integer" % int(np.nonzero(bad)[0][0]))
        bad = (a < -2 ** 31) | (a > 2 ** 31 - 1)
        if np.any(bad):
            raise ArgumentError("strata[%d] does not fit int32" % int(np.nonzero(bad)[0][0]))
        strata = np.ascontiguousarray(a, dtype=np.int32)
    if weights is not None:
        v = np.ascontiguousarray(weights, dtype=np.float64)
        if v.ndim != 1 or v.shape[0] != n:
            raise DimensionMismatch("length(weights) != size(X, 1)")
        bad = ~(np.isfinite(v) & (v > 0.0))
        if np.any(bad):
            raise ArgumentError("weights[%d] is not finite and > 0" % int(np.nonzero(bad)[0][0]))
        weights = v * n / v.sum()
    return strata, weights


_COX_TIES = ("breslow", "efron")             # cdh_glm_set_cox_ties' 0 and 1


def _cox_ties(ties, X=None, y=None):
    """What the Cox front ends refuse of their ties keyword before the device: an unknown rule, and Efron together with
    start-stop times (a matrix with a three-column y, or a loss made with them).  -> ties."""
    if not isinstance(ties, str) or ties not in _COX_TIES:
        raise ArgumentError('ties must be "breslow" or "efron", not %r' % (ties,))
    interval = getattr(X, "_interval", False) if isinstance(X, CoordinateDifferentiableFunction) else \
        (y is not None and np.ndim(y) == 2 and np.shape(y)[1] == 3)
    if ties == "efron" and interval:
        raise ArgumentError("Efron ties are not offered with start-stop times (y n x 3)")
    return ties


class CDCoxLoss(_GLMLoss):
    """CDCoxLoss(y, X, offset=None; strata=None, weights=None): -(1/n) Σ δ_i (η_i - log S_i), η = Xβ + o, S_i = Σ_{t_j >= t_i} e^η_j -- the negative log
    partial likelihood of the Cox model with Breslow ties (glmnet's family = "cox"); y is n x 2, [time, status], status 1 an
    event and 0 censored; no reference counterpart.  Minimised by IRLS like its siblings CDLogisticLoss and CDPoissonLoss: a
    round is the weighted lasso of CDWeightedLSLoss (src/cd_differentiable_function.jl:118-194) on the working response and
    weights the handle's y and w hold from one irls_step to the next.  The step is not elementwise: the risk-set sums are
    scans in time order, run on the device through the order cdh_glm_set_survival keeps; the rows stay in the caller's order.
    There is no intercept (it cancels).

    Ties: Breslow unless set_ties("efron") is called -- Efron's rule, survival::coxph's default, for right-censored data (not
    yet with start-stop times).  Among the training rows of a tie group with d events, D = Σ v e and m = (Σ v δ) / d over them,
    the l-th event's denominator is S - (l/d) D: F = -(1/n) Σ_g [Σ_events v δ η - m Σ_l log(S - (l/d) D)], and A_i, B_i sum
    m c / den and m c² / den² with c = 1 - l/d inside an event's own group and 1 elsewhere.  The weights follow coxph's
    convention (every event of a group enters with the group's mean event weight).  The group sums are scans that restart at
    the groups' bounds, on the device: constant work per row whatever the groups' sizes.

    Start-stop times (glmnet's Surv(start, stop, status)): y is n x 3, [start, stop, status], and row i is at risk at t iff
    start_i < t <= stop_i -- time-varying covariates (a subject is several rows), delayed entry, recurrent events.  A row
    whose start equals an event time is not at risk at it; one whose stop equals it is.  S(t) is then a DIFFERENCE, the sum
    over stop_j >= t less the sum over start_j >= t (a second order by (stratum, start), a second scan), and A_i = P(stop_i) -
    P(start_i) with P(u) = Σ_{event times t <= u} δ / S(t), B likewise.  The subtraction is inherent -- glmnet and
    survival::coxph subtract too: the error of S is relative to the two sums of the row's stratum, about n U (T + T2), not to
    S, and that of A and B to P(stop) + P(start); an event whose computed S is not > 0 is skipped, a working weight driven
    negative is clamped at wmin.  The handle then always runs the segmented, weighted arithmetic.  The library does not know
    subjects: in cross-validation the rows of one subject should share a fold -- pass folds=.

    strata (glmnet's stratifySurv): integer ids that fit int32; S_i, A_i and B_i then run over the rows of row i's stratum
    only, by scans that restart at every stratum's boundary.  weights (glmnet's weights =): v_i > 0, normalised HERE to sum to
    n (v n / Σv; the library stores what it is given), so that unit weights leave F as it was:
    F = -(1/n) Σ v_i δ_i (η_i - log S_i) with S_i = Σ v_j e^η_j; the working weight is v e A - (v e)² B, so an integer weight
    reproduces a replicated row's gradient and nll, not its diagonal.  The penalty scales of the paths stay the reference's
    _stdX!, the root mean square over the rows present: they are NOT weighted by v.  fp64 only, one device."""

    def __init__(self, y, X, offset=None, *, strata=None, weights=None, device=0):
        self._start, self._time, status = _survival3(y, np.shape(X)[0] if np.ndim(X) == 2 else None)
        if offset is not None and not np.all(np.isfinite(np.asarray(offset, dtype=np.float64))):
            raise ArgumentError("the offset is not finite")
        self._strata, self._weights = _strata_weights(strata, weights, len(status))
        self._weighted = self._weights is not None
        self._interval = self._start is not None
        self._n_events = int(np.count_nonzero(status))           # baseline_hazard's capacity, without a download
        super().__init__(status, X, offset, device=device)
        del self._start, self._time, self._strata, self._weights

    def _set_observations(self, status, off):
        if self._start is not None:
            check(self._L.cdh_glm_set_survival_interval(self._h, _vp(self._start), _vp(self._time), _vp(status), _vp(off),
                                                        _vp(self._strata), _vp(self._weights)), self._h)
        elif self._strata is None and self._weights is None:
            check(self._L.cdh_glm_set_survival(self._h, _vp(self._time), _vp(status), _vp(off)), self._h)
        else:
            check(self._L.cdh_glm_set_survival_strata(self._h, _vp(self._time), _vp(status), _vp(off), _vp(self._strata),
                                                      _vp(self._weights)), self._h)

    def set_ties(self, ties):
        """The tie rule of the step's sums (cdh_glm_set_cox_ties): "breslow" (the default) or "efron", survival::coxph's default.
        Efron is refused on a loss with start-stop times.  The handle's y, w and r are not touched: the next irls_step runs
        under the new rule."""
        _cox_ties(ties)
        if ties == "efron" and getattr(self, "_interval", False):
            raise ArgumentError("Efron ties are not offered with start-stop times (y n x 3)")
        check(self._L.cdh_glm_set_cox_ties(self._h, _COX_TIES.index(ties)), self._h)

    @property
    def ties(self):
        """The tie rule the handle holds: "breslow" or "efron"."""
        if getattr(self, "_h", None) is None:
            return "breslow"
        out = C.c_int32()
        check(self._L.cdh_glm_get_cox_ties(self._h, C.byref(out)), self._h)
        return _COX_TIES[out.value]

    @property
    def strata(self):
        """The stratum ids (int32), in the caller's row order; zeros when none were given."""
        out = np.zeros(self.n, dtype=np.int32)
        check(self._L.cdh_glm_get_survival_strata(self._h, _vp(out), None), self._h)
        return out

    @property
    def weights(self):
        """The observation weights the handle holds (normalised to sum to n), in the caller's row order; ones when none
        were given."""
        out = np.zeros(self.n)
        check(self._L.cdh_glm_get_survival_strata(self._h, None, _vp(out)), self._h)
        return out

    def _get_survival(self, which):
        out = np.zeros(self.n)
        args = (_vp(out), None) if which == 0 else (None, _vp(out))
        check(self._L.cdh_glm_get_survival(self._h, *args), self._h)
        return out

    @property
    def start(self):
        """The start times, in the caller's row order; None when y had two columns (every row at risk from -inf)."""
        if not getattr(self, "_interval", False):
            return None
        out = np.zeros(self.n)
        check(self._L.cdh_glm_get_survival_start(self._h, _vp(out)), self._h)
        return out

    time = property(lambda self: self._get_survival(0), doc="The times (the stop times of start-stop data), in the caller's row order.")
    status = property(lambda self: self._get_survival(1), doc="The statuses: 1 an event, 0 censored.")
    offset = CDPoissonLoss.offset

    def _step(self, apply, wmin, eta_max, k):
        out = np.zeros(5)
        check(self._L.cdh_glm_cox_irls(self._h, int(k), 1 if apply else 0, float(wmin), float(eta_max),
                                       out.ctypes.data_as(C.POINTER(C.c_double))), self._h)
        return out

    def _events(self, v):
        """Σ v δ as the record reports it: an int on an unweighted loss, the float itself on a weighted one."""
        return float(v) if getattr(self, "_weighted", False) else int(v)

    def _record(self, out, n):
        return {"nll": float(out[0]) / n, "sum_w": float(out[1]), "clamped": int(out[2]), "capped": int(out[3]),
                "events": self._events(out[4])}

    def irls_step(self, apply=True, wmin=1e-5, eta_max=50.0, fold=None):
        """One IRLS step at the iterate the handle holds (cdh_glm_cox_irls).  apply=True turns the handle's y, w and r into the
        working response (without the offset), the working weights (e A - e² B, clamped below at wmin; η capped above at
        eta_max) and their residual; apply=False only reads.  Returns {"nll": (1/n) Σ δ_i (log S_i - η_i), "sum_w": Σ w_i,
        "clamped": rows whose weight was clamped (the rows before the first event always are), "capped": rows whose η was
        capped, "events": Σ δ_i}, the sums over the training rows ("capped" over all rows).  With strata and weights S, A and B
        are those of the row's stratum, e and δ are v e and v δ, and "events" is the float Σ v_i δ_i.

        fold=k (after set_folds): the rows of fold k are held out -- they leave the risk sets and the event sums, and get
        w = 0, z = Xβ, r = 0."""
        k = -1 if fold is None else int(fold)
        if k < 0 and fold is not None:
            raise ArgumentError("fold must be a fold id")
        return self._record(self._step(apply, wmin, eta_max, k), self.n)

    def _irls(self, apply, irls, fold):
        """The step as the IRLS loop calls it.  Read-only with a fold it runs twice, with fold k held out and with nobody held
        out, and adds "held_deviance" = -2 (ℓ_all - ℓ_train), glmnet's grouped partial-likelihood deviance of the held-out
        rows (a sum), and "held_events", the events among them."""
        if fold is None or apply:
            return self.irls_step(apply, irls.wmin, irls.etaMax, fold)
        train = self._step(False, irls.wmin, irls.etaMax, int(fold))
        every = self._step(False, irls.wmin, irls.etaMax, -1)
        res = self._record(train, self.n)
        res["held_deviance"] = 2.0 * (float(every[0]) - float(train[0]))
        res["held_events"] = self._events(every[4]) - self._events(train[4])
        return res

    def residuals(self, type="martingale", eta_max=50.0):
        """The residuals of the model at the iterate the handle holds (cdh_glm_cox_residuals), an n-vector in the caller's row
        order; no row is held out.  type: "martingale" -- M_i = δ_i - e^η_i A_i, survival's residuals(coxph, "martingale"),
        unweighted (v_i M_i is the gradient's term); "deviance" -- sign(M_i) sqrt(-2 (M_i + δ_i log(e^η_i A_i))),
        residuals(coxph, "deviance"); "cumhaz" -- A_i itself, the baseline cumulative hazard accrued over the row's time at
        risk: H0 at the row's time (less H0 at its start with start-stop times) -- the A of the handle's own step, read where the
        baseline table reads it, so that it equals baseline_hazard()'s step function at the row's time with ==.
        The baseline is uncentred (x = 0, offset 0).  η is capped at eta_max as in irls_step; y, w, r and β are not touched."""
        if type not in _COX_RESIDUALS:
            raise ArgumentError('type must be "martingale", "deviance" or "cumhaz", not %r' % (type,))
        out = np.zeros(self.n)
        ptrs = [_vp(out) if t == type else None for t in _COX_RESIDUALS]
        check(self._L.cdh_glm_cox_residuals(self._h, float(eta_max), *ptrs), self._h)
        return out

    def baseline_hazard(self, eta_max=50.0):
        """The cumulative baseline hazard of the model at the iterate the handle holds (cdh_glm_cox_baseline; R's basehaz(fit,
        centered = FALSE) and glmnet's survfit.coxnet at x = 0): a CoxBaseline with one entry per (stratum, event time), in
        (stratum id, time) ascending order.  Breslow's estimate, or Efron's on a loss set to Efron ties; uncentred (x = 0,
        offset 0).  The tie groups are compacted on the device; `hazard` is the per-stratum first difference of `cumhaz`,
        taken here.  y, w, r and β are not touched."""
        cap = getattr(self, "_n_events", None)                   # a table row holds at least one event: one call suffices
        if cap is None:                                          # (a loss whose survival data did not come through __init__)
            cap = int(np.count_nonzero(self.status))
        stratum = np.zeros(cap, dtype=np.int32)
        cols = [np.zeros(cap) for _ in range(5)]
        count = C.c_int64()
        check(self._L.cdh_glm_cox_baseline(self._h, float(eta_max), cap, _vp(stratum), *[_vp(c) for c in cols], C.byref(count)),
              self._h)
        m = count.value
        stratum = stratum[:m].copy()
        time, n_event, risk_sum, cumhaz, cumvar = (c[:m].copy() for c in cols)
        head = np.r_[True, stratum[1:] != stratum[:-1]] if m else np.zeros(0, dtype=bool)
        hazard = np.where(head, cumhaz, cumhaz - np.r_[0.0, cumhaz[:-1]]) if m else np.zeros(0)
        return CoxBaseline(stratum, time, n_event, risk_sum, hazard, cumhaz, cumvar)

    def concordance(self, fold=None):
        """Harrell's concordance index of the model at the iterate the handle holds (cdh_glm_cox_concordance; R's
        survival::concordance, glmnet's Cindex): a CoxConcordance.  fold=None: over all rows; fold=k (after set_folds): over the
        rows of fold k alone, the held-out rows.  Rows i != j of one stratum are comparable, i the earlier, iff i is an event
        and t_j > t_i, or t_j == t_i and j is censored; the pair is concordant if η_i > η_j, discordant if η_i < η_j, tied if
        they are equal, and counts v_i v_j.  η = Xβ + offset is NOT capped.  The counts come from a merge sort of η on the
        device; without weights they are exact.  The tie rule does not enter; not offered with start-stop times.  y, w, r and β
        are not touched.  A NaN among the η of the rows that take part is refused."""
        k = -1 if fold is None else int(fold)
        if k < 0 and fold is not None:
            raise ArgumentError("fold must be a fold id")
        out = np.zeros(4)
        check(self._L.cdh_glm_cox_concordance(self._h, k, out.ctypes.data_as(C.POINTER(C.c_double))), self._h)
        if out[3] > 0:
            raise ArgumentError("eta is NaN in %d of the rows that take part: the concordance index is undefined" % int(out[3]))
        c, d, t = float(out[0]), float(out[1]), float(out[2])
        comparable = c + d + t
        return CoxConcordance(c, d, t, comparable, (c + t / 2.0) / comparable if comparable > 0 else float("nan"))

    def _score_columns(self, columns):
        """The 1-based columns of a score call: the given ones, or the support of the handle's β."""
        if columns is None:
            idx = np.zeros(max(self.p, 1), dtype=np.int64)
            nnz = C.c_int64()
            check(self._L.cdh_get_support(self._h, _vp(idx), C.byref(nnz)), self._h)
            cols = idx[: nnz.value].copy()
            if len(cols) == 0:
                raise ArgumentError("the support of β is empty: name the columns")
        else:
            cols = np.atleast_1d(np.asarray(columns))
            if cols.ndim != 1 or len(cols) == 0 or not np.issubdtype(cols.dtype, np.integer):
                raise ArgumentError("columns must be a non-empty vector of 1-based column indices")
            cols = np.ascontiguousarray(cols, dtype=np.int64)
        if len(cols) > COX_SCORE_MAX_COLS:
            raise ArgumentError("%d columns: score residuals and the information matrix are offered for at most %d columns"
                                % (len(cols), COX_SCORE_MAX_COLS))
        if cols.min() < 1 or cols.max() > self.p:
            raise ArgumentError("a column index lies outside 1 .. p")
        return cols

    def _score(self, columns, eta_max, schoenfeld=False, score=False, info=False, centre=None):
        """cdh_glm_cox_score -> (columns, schoenfeld n x m or None, score n x m or None, info m x m or None, the centres used)."""
        cols = self._score_columns(columns)
        m = len(cols)
        mu = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
        if mu is not None and mu.shape != (m,):
            raise DimensionMismatch("centre must hold one value per column")
        used = np.zeros(m)
        sch = np.zeros((self.n, m), order="F") if schoenfeld else None
        L = np.zeros((self.n, m), order="F") if score else None
        I = np.zeros((m, m)) if info else None
        check(self._L.cdh_glm_cox_score(self._h, float(eta_max), m, _vp(cols), _vp(mu), _vp(used), _vp(sch), _vp(L), _vp(I)), self._h)
        return cols, sch, L, I, used

    def score_residuals(self, columns=None, weighted=False, eta_max=50.0):
        """The score residuals of the model at the iterate the handle holds (cdh_glm_cox_score; R's residuals(coxph, "score")),
        n x m in the caller's row order, for the 1-based `columns` (None: the support of the handle's β; at most 64), Breslow
        ties: L_ic = δ_i (x_ic - x̄_c(t_i)) - e^η_i Σ_{event times t <= t_i} h(t) (x_ic - x̄_c(t)), x̄_c(t) the risk-set mean
        Σ v e^η x_c / S.  weighted=True multiplies row i by v_i; the column sums of the weighted form are the gradient
        X_c'(vδ - v e^η A).  Not offered with Efron ties or start-stop times yet.  y, w, r and β are not touched."""
        _, _, L, _, _ = self._score(columns, eta_max, score=True)
        return L * self.weights[:, None] if weighted else L

    def schoenfeld_residuals(self, columns=None, eta_max=50.0):
        """The Schoenfeld residuals x_ic - x̄_c(t_i) of the events (cdh_glm_cox_score; R's residuals(coxph, "schoenfeld")): a
        CoxSchoenfeld with the event rows in (stratum, time) ascending order, ties in the handle's order, which is the
        caller's.  An event whose risk-set sum is not > 0 has a zero row.  What a proportional-hazards check needs."""
        cols, sch, _, _, _ = self._score(columns, eta_max, schoenfeld=True)
        status, time, strata = self.status, self.time, self.strata
        rows = np.nonzero(status != 0)[0]
        rows = rows[np.lexsort((time[rows], strata[rows]))]       # stable: ties keep the caller's order
        return CoxSchoenfeld(rows, strata[rows], time[rows], np.ascontiguousarray(sch[rows]), cols)

    def information(self, columns=None, eta_max=50.0):
        """The information matrix of the model at the iterate the handle holds (cdh_glm_cox_score), m x m: the Hessian of the
        un-normalised negative log partial likelihood in β_columns, Σ_events vδ [Σ_risk v e^η x̃x̃'/S - x̄x̄'], formed on the
        device from centred columns; symmetric.  Its inverse is coxph's var."""
        return self._score(columns, eta_max, info=True)[3]


COX_SCORE_MAX_COLS = 64     # include/cdhip.h: cdh_glm_cox_score's cap; kCoxScoreMaxCols in csrc/cox_plan.hpp


@dataclass
class CoxSchoenfeld:
    """The Schoenfeld residuals of a Cox model (CDCoxLoss.schoenfeld_residuals): `rows` -- the event rows' indices in (stratum,
    time) ascending order; `stratum` and `time` of those rows; `resid` -- n_events x m, x_ic - x̄_c(t_i); `columns` -- the
    1-based columns."""
    rows: np.ndarray
    stratum: np.ndarray
    time: np.ndarray
    resid: np.ndarray
    columns: np.ndarray


@dataclass
class CoxInference:
    """Standard errors of a fitted Cox model (coxInference): `columns` (1-based), `beta` on them, `var` = I⁻¹, `se`, `z` =
    beta / se; with robust=True also `dfbeta` = diag(v) L I⁻¹ (n x m; R's residuals(type = "dfbeta", weighted = TRUE)),
    `robust_var` = D'D with D = dfbeta summed over the cluster ids, and `robust_se` -- else None."""
    columns: np.ndarray
    beta: np.ndarray
    var: np.ndarray
    se: np.ndarray
    z: np.ndarray
    dfbeta: np.ndarray = None
    robust_var: np.ndarray = None
    robust_se: np.ndarray = None


_COX_RESIDUALS = ("cumhaz", "martingale", "deviance")      # cdh_glm_cox_residuals' three outputs, in its order


@dataclass
class CoxBaseline:
    """The cumulative baseline hazard of a Cox model (CDCoxLoss.baseline_hazard; R's basehaz, uncentred), one entry per tie
    group -- one stratum, one time -- that holds an event, in (stratum, time) ascending order: the stratum id, the time, n_event
    (Σ v δ over the group), risk_sum (Σ v e^η over the rows at risk), hazard (the increment of cumhaz inside the stratum),
    cumhaz (H0 of the stratum at that time, the group included) and cumvar (the same sum of hazard / risk_sum)."""
    stratum: np.ndarray
    time: np.ndarray
    n_event: np.ndarray
    risk_sum: np.ndarray
    hazard: np.ndarray
    cumhaz: np.ndarray
    cumvar: np.ndarray


@dataclass
class CoxConcordance:
    """Harrell's concordance index (CDCoxLoss.concordance): the weighted numbers of concordant, discordant and tied pairs,
    comparable = their sum, and C = (concordant + tied / 2) / comparable -- nan when nothing is comparable."""
    concordant: float
    discordant: float
    tied: float
    comparable: float
    C: float


# --------------------------------------------------------------------------------------
# Smoothing kernels (src/varying_coefficient_lasso.jl:3-21)
# --------------------------------------------------------------------------------------
class SmoothingKernel:
    """abstract type SmoothingKernel{T} (src/varying_coefficient_lasso.jl:3); field h, the bandwidth."""
    _kind = None

    def __init__(self, h):
        self.h = float(h)

    def __repr__(self):
        return f"{type(self).__name__}({self.h!r})"


class GaussianKernel(SmoothingKernel):
    """GaussianKernel(h) (:6-8)."""
    _kind = CDH_VC_GAUSSIAN


class EpanechnikovKernel(SmoothingKernel):
    """EpanechnikovKernel(h) (:10-12)."""
    _kind = CDH_VC_EPANECHNIKOV


def createKernel(kernelType, h):
    """createKernel(::Type{K}, h) (:14-15)."""
    if not (isinstance(kernelType, type) and issubclass(kernelType, SmoothingKernel) and kernelType._kind is not None):
        raise TypeError("MethodError: createKernel(::Type{<:SmoothingKernel}, h)")
    return kernelType(h)


def evaluate(k, x, y):
    """evaluate(k, x, y) (:17-21), on the host and as the reference writes it -- not the textbook forms: the Gaussian is
    exp(-(x-y)^2 / h) / h, the Epanechnikov 0.75 (1 - u^2) / h with u = (x-y) / h, zero from |u| = 1 on.  Broadcasts."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if isinstance(k, GaussianKernel):
        out = np.exp(-(x - y) ** 2 / k.h) / k.h
    elif isinstance(k, EpanechnikovKernel):
        u = (x - y) / k.h
        out = np.where(np.abs(u) >= 1.0, 0.0, 0.75 * (1.0 - u * u) / k.h)
    else:
        raise TypeError("MethodError: evaluate(k::SmoothingKernel, x, y)")
    return float(out) if out.ndim == 0 else out


def get_nonzero_coordinates(beta, p, degree, expanded):
    """get_nonzero_coordinates(β, p, degree, expanded) (:479-512): which of the p groups of degree + 1 consecutive
    coefficients hold a non-zero -- as a mask over the p (degree + 1) coefficients (expanded) or over the p groups."""
    b = beta.dense() if isinstance(beta, SparseIterate) else np.asarray(beta, dtype=np.float64)
    if b.shape[0] != p * (degree + 1):
        raise DimensionMismatch("length(β) != p * (degree + 1)")
    groups = (b.reshape(p, degree + 1) != 0.0).any(axis=1)
    return np.repeat(groups, degree + 1) if expanded else groups


class CDVaryingCoefficientLoss(CDWeightedLSLoss):
    """The CDWeightedLSLoss(y, expandX, w) that locpolyl1 keeps rewriting (src/varying_coefficient_lasso.jl:50-65), with the
    base design X (n x p) and z resident in HBM: `set_point` regenerates the kernel weights, the expanded design
    X[i,:] ⊗ [1, (z_i - z0), ..., (z_i - z0)^degree] and its weighted column scales on the device for a new z0
    (cdh_vc_set_data / cdh_vc_set_point).  numCoordinates is p (degree + 1); base column j is expanded column j (degree + 1)."""

    def __init__(self, y, X, z, degree, *, device=0):
        X, y, z = np.asarray(X), np.asarray(y), np.asarray(z)
        if X.dtype not in (np.float64, np.float32) or y.dtype != X.dtype or z.dtype != X.dtype or X.ndim != 2:
            raise TypeError("MethodError: X::Matrix{T}, z::Vector{T}, y::Vector{T}, T<:AbstractFloat")
        if y.shape[0] != X.shape[0]:
            raise DimensionMismatch("length(y) != size(X, 1)")
        if z.shape[0] != X.shape[0]:
            raise DimensionMismatch("length(z) != size(X, 1)")
        degree = int(degree)
        if not 0 <= degree <= 3:
            raise ArgumentError("the polynomial degree must be 0 .. 3")
        n, pb = X.shape
        self.p_base, self.degree = int(pb), degree
        self._create(X.dtype, n, pb * (degree + 1), device, None, 0)
        Xf, zz = np.asfortranarray(X), np.ascontiguousarray(z)
        check(self._L.cdh_vc_set_data(self._h, pb, degree, _vp(Xf), n, _vp(zz)), self._h)
        check(self._L.cdh_set_y(self._h, _vp(np.ascontiguousarray(y))), self._h)
        self.point_stats = []

    def set_point(self, kernel, z0):
        """w .= evaluate.(kernel, z, z0); _expand_X!(expandX, X, z, z0, degree); _stdX!(stdX, w, expandX) (:63-65) on the
        device; returns stdX.  The iterate the handle holds is kept (the next solve warm-starts from it)."""
        if not isinstance(kernel, SmoothingKernel) or kernel._kind is None:
            raise TypeError("MethodError: kernel::SmoothingKernel")
        out = np.zeros(self.p)
        check(self._L.cdh_vc_set_point(self._h, kernel._kind, kernel.h, float(z0), _vp(out)), self._h)
        return out

    def set_point_leave_out(self, kernel, row):
        """The point of lvocv_locpolyl1 for observation `row` (0-based, as X_cols counts columns): z0 = z[row] as stored,
        w .= evaluate.(kernel, z, z0); w[row] = 0; _expand_X!; _stdX! (:109-113), and the screening scores |Σ_i X_ij w_i y_i| of
        _findLargestCorrelations(w, X, y, s) (src/utils.jl:108-124) from the same pass over the design; returns
        (stdX, scores).  The iterate the handle holds is kept."""
        if not isinstance(kernel, SmoothingKernel) or kernel._kind is None:
            raise TypeError("MethodError: kernel::SmoothingKernel")
        std, scores = np.zeros(self.p), np.zeros(self.p)
        check(self._L.cdh_vc_set_point_loo(self._h, kernel._kind, kernel.h, int(row), _vp(std), _vp(scores)), self._h)
        return std, scores

    def _gram_columns_and_e(self, base_cols, e):
        """What expanded_gram and expanded_gram_batch share: -> (the listed base columns 1-based, their number mb,
        ep = mb (degree + 1), e as an n-vector of the design's type or None)."""
        cols = np.arange(self.p_base) if base_cols is None else np.atleast_1d(np.asarray(base_cols))
        if cols.dtype == bool:
            cols = np.nonzero(cols)[0]
        idx1 = np.ascontiguousarray(cols.astype(np.int64) + 1)
        mb = idx1.shape[0]
        ep = mb * (self.degree + 1)
        ee = None
        if e is not None:
            ee = np.ascontiguousarray(np.asarray(e), dtype=self.dtype)
            if ee.shape != (self.n,):
                raise DimensionMismatch("length(e) != size(X, 1)")
        return idx1, mb, ep, ee

    def expanded_gram(self, kernel, z0=0.0, *, leave_out=None, wpow=1, e=None, base_cols=None, rhs=True):
        """_expand_Xt_w_X! / _expand_Xt_w_Y! (src/varying_coefficient_lasso.jl:572-647) of the listed base columns around z0,
        straight from the resident base design (cdh_vc_gram): -> (G, c, Σω), G the ep x ep weighted Gram matrix of the expanded
        design, ep = len(base_cols) (degree + 1), c its right-hand side (None with rhs=False), ω_i = K(z_i, z0)^wpow · e_i.
        `leave_out` (a 0-based row) moves z0 to the stored z[row] (the z0 given is then ignored) and gives that row weight zero; `base_cols` are 0-based base
        columns (default: all; at most 64), `e` an optional n-vector.  A read-only query: the handle's weights, expanded
        columns, residual, cache and iterate stay as they are."""
        _check_kernel(kernel)
        idx1, mb, ep, ee = self._gram_columns_and_e(base_cols, e)
        G = np.zeros((ep, ep), order="F")
        c = np.zeros(ep) if rhs else None
        sw = C.c_double()
        check(self._L.cdh_vc_gram(self._h, kernel._kind, kernel.h, 0.0 if leave_out is not None else float(z0),
                                  -1 if leave_out is None else int(leave_out),
                                  int(wpow), _vp(ee), mb, _vp(idx1), _vp(G), _vp(c), C.byref(sw)), self._h)
        return G, c, sw.value

    def expanded_gram_batch(self, kernel, h, z0=None, *, leave_out=None, wpow=1, e=None, base_cols=None, rhs=True):
        """expanded_gram around m points in one call (cdh_vc_gram_batch): -> (G[m, ep, ep], c[m, ep] or None, Σω[m]), point t
        bit-identical to expanded_gram(kernelType(h[t]), z0[t], leave_out=leave_out[t], ...).  `kernel` is a kernel type
        (GaussianKernel, EpanechnikovKernel), a kernel (its type is taken; the bandwidths are `h`) or a cdh_vc_kernel code;
        `h`, `z0` and `leave_out` are scalars or length-m vectors, broadcast against each other; an entry of `leave_out`
        is a 0-based row or -1 for none.  `wpow`, `e` and `base_cols` are shared by the points.  At most
        CDH_VC_GRAM_MAX_POINTS points per call.  A read-only query, as expanded_gram."""
        kind = _kernel_kind(kernel)
        args = [np.asarray(h, dtype=np.float64)]
        if z0 is not None:
            args.append(np.asarray(z0, dtype=np.float64))
        if leave_out is not None:
            lo = np.asarray(leave_out)
            if lo.dtype.kind not in "iu":
                raise TypeError("MethodError: leave_out::Vector{Int64}")
            args.append(lo.astype(np.int64))
        if any(a.ndim > 1 for a in args):
            raise TypeError("MethodError: h, z0 and leave_out are scalars or vectors")
        try:
            shape = np.broadcast_shapes(*[a.shape for a in args])
        except ValueError:
            raise DimensionMismatch("h, z0 and leave_out do not broadcast to one length") from None
        m = int(shape[0]) if shape else 1
        if not 1 <= m <= _lib.CDH_VC_GRAM_MAX_POINTS:
            raise ArgumentError(f"cdh_vc_gram_batch: need 1 <= m <= {_lib.CDH_VC_GRAM_MAX_POINTS} points")
        full = [np.ascontiguousarray(np.broadcast_to(a, (m,))) for a in args]
        hh = full[0]
        zz = full[1] if z0 is not None else None
        ll = full[-1] if leave_out is not None else None
        idx1, mb, ep, ee = self._gram_columns_and_e(base_cols, e)
        G = np.zeros((m, ep, ep))
        c = np.zeros((m, ep)) if rhs else None
        sw = np.zeros(m)
        check(self._L.cdh_vc_gram_batch(self._h, kind, m, _vp(hh), _vp(zz), _vp(ll), int(wpow), _vp(ee), mb, _vp(idx1),
                                        _vp(G), _vp(c), _vp(sw)), self._h)
        return G.transpose(0, 2, 1), c, sw          # a block is column-major: G[t] is what expanded_gram returns


class CDQuadraticLoss(CoordinateDifferentiableFunction):
    """CDQuadraticLoss(A, b): x'Ax/2 + x'b (src/cd_differentiable_function.jl:299-348), behind one cdh_quad handle.

    A p-vector `b` is the reference's single problem; a p x m `b` is a batch of m problems that share A (problem j has
    b[:, j]) and are solved by coordinateDescent_ in one launch.  fp64 only (the reference's Ax is Float64 whatever T is).
    The generic functions take `problem=j` (0-based) to address one problem of a batch."""

    def __init__(self, A, b, *, device=0, max_batch=None):
        A, b = np.asarray(A), np.asarray(b)
        if A.dtype != np.float64 or b.dtype != np.float64:
            raise TypeError("MethodError: CDQuadraticLoss is Float64 only (A::Matrix{Float64}, b::Vector{Float64})")
        if A.ndim != 2 or A.shape[0] != A.shape[1]:          # :306 issymmetric(A)
            raise ArgumentError("A must be square")
        if b.ndim not in (1, 2) or b.shape[0] != A.shape[0] or (b.ndim == 2 and b.shape[1] < 1):
            raise ArgumentError("length(b) != size(A, 1)")
        if not np.array_equal(A, A.T):
            raise ArgumentError("A must be symmetric")
        self.p = int(A.shape[0])
        self.batched = b.ndim == 2
        self.m = int(b.shape[1]) if self.batched else 1
        self.max_batch = self.m if max_batch is None else int(max_batch)
        if self.m > self.max_batch:
            raise ArgumentError(f"m = {self.m} problems exceed the handle's max_batch = {self.max_batch}")
        if self.p > _lib.CDH_QUAD_MAX_P:
            raise ArgumentError(f"p = {self.p} exceeds CDH_QUAD_MAX_P = {_lib.CDH_QUAD_MAX_P}, the largest problem whose state fits "
                                "160 KiB of LDS")
        self._L = _lib.lib()
        self._h = None
        h = C.c_void_p()
        check(self._L.cdh_quad_create(C.byref(h), self.p, self.max_batch, int(device)), None)
        self._h = h
        Af = np.asfortranarray(A)
        self._q(self._L.cdh_quad_set_A(self._h, _vp(Af), self.p))
        self.last_stats = None
        self._load_b(b)

    def _load_b(self, b):
        self.b = np.array(b.reshape(self.p, self.m), dtype=np.float64, order="F", copy=True)   # column j = problem j, ldb = p
        self._q(self._L.cdh_quad_set_b(self._h, self.m, _vp(self.b), self.p))
        self._synced = [None] * self.m       # (id(x), version) of the iterate the handle mirrors, per problem
        self._zero = [True] * self.m         # the handle's iterate is still the zero a new b leaves: an empty x needs no upload
        self._lam0 = np.zeros(self.m)
        self._omega = None                   # None, a p-vector shared by all problems, or p x m (column-major)
        self._pen_sent = False

    def set_b(self, b):
        """Another b (p-vector, or p x m with m <= max_batch) on the same A: as a new loss, every iterate zero and Ax = 0."""
        b = np.asarray(b)
        if b.dtype != np.float64:
            raise TypeError("MethodError: CDQuadraticLoss is Float64 only")
        if b.ndim not in (1, 2) or b.shape[0] != self.p or (b.ndim == 2 and b.shape[1] < 1):
            raise ArgumentError("length(b) != size(A, 1)")
        m = int(b.shape[1]) if b.ndim == 2 else 1
        if m > self.max_batch:
            raise ArgumentError(f"m = {m} problems exceed the handle's max_batch = {self.max_batch}")
        self.batched, self.m = b.ndim == 2, m
        self._load_b(b)

    def _q(self, status):
        check(status, None)                  # (a quad handle reports through cdh_last_error(NULL))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.cdh_quad_destroy(self._h)
                self._h = None
        except Exception:
            pass

    close = __del__

    # -- penalty -----------------------------------------------------------------------------
    def _send_penalty(self):
        om = self._omega
        ldo = 0 if om is None or om.ndim == 1 else self.p
        self._q(self._L.cdh_quad_set_penalty(self._h, _vp(self._lam0), _vp(om), ldo))
        self._pen_sent = True

    def _set_penalty(self, g, problem=0):
        """ProxL1 of ONE problem; the others keep theirs."""
        if not isinstance(g, ProxL1):
            raise TypeError("MethodError: descendCoordinate! is defined for g::ProxL1 only")
        j, om = int(problem), self._omega
        col = None if om is None else (om if om.ndim == 1 else om[:, j])
        same = self._pen_sent and self._lam0[j] == g.lambda0 and \
            ((g.lam is None and col is None) or (g.lam is not None and col is not None and np.array_equal(g.lam, col)))
        if same:
            return
        self._lam0[j] = g.lambda0
        if self.m == 1:
            self._omega = None if g.lam is None else g.lam.copy()
        elif not (g.lam is None and om is None):
            if om is None or om.ndim == 1:
                self._omega = np.asfortranarray(np.tile((np.ones(self.p) if om is None else om)[:, None], (1, self.m)))
            self._omega[:, j] = 1.0 if g.lam is None else g.lam
        self._send_penalty()

    def _set_penalties(self, gs):
        """One ProxL1 per problem, or one for all."""
        shared = isinstance(gs, ProxL1)
        glist = [gs] * self.m if shared else list(gs)
        if len(glist) != self.m or not all(isinstance(g, ProxL1) for g in glist):
            raise ArgumentError("need one ProxL1, or one per problem")
        self._lam0 = np.array([g.lambda0 for g in glist], dtype=np.float64)
        if all(g.lam is None for g in glist):
            self._omega = None
        elif shared or self.m == 1:
            self._omega = glist[0].lam.copy()
        else:
            self._omega = np.asfortranarray(np.stack([np.ones(self.p) if g.lam is None else g.lam for g in glist], axis=1))
        self._send_penalty()

    # -- iterates ------------------------------------------------------------------------------
    def _problem(self, problem):
        j = int(problem)
        if not 0 <= j < self.m:
            raise ArgumentError(f"problem {j} outside 0 .. {self.m - 1}")
        return j

    def _push(self, x, j):
        idx = np.ascontiguousarray(x.nzval2ind, dtype=np.int64)
        val = np.ascontiguousarray(x._val[: x.nnz], dtype=np.float64)
        self._q(self._L.cdh_quad_set_iterate(self._h, j, x.nnz, _vp(idx), _vp(val)))
        self._synced[j] = (id(x), x._version)
        self._zero[j] = x.nnz == 0

    def _ensure_synced(self, x, j):
        if numCoordinates(x) != self.p:
            raise DimensionMismatch("numCoordinates(x) != numCoordinates(f)")
        if self._synced[j] != (id(x), x._version):
            if x.nnz == 0 and self._zero[j]:
                self._synced[j] = (id(x), x._version)
            else:
                self._push(x, j)

    def _pull(self, x, j):
        if getattr(self, "_pull_idx", None) is None:
            self._pull_idx, self._pull_val = np.zeros(self.p, dtype=np.int64), np.zeros(self.p)
        nnz = C.c_int64()
        self._q(self._L.cdh_quad_get_iterate(self._h, j, C.byref(nnz), _vp(self._pull_idx), _vp(self._pull_val)))
        x._load(self._pull_idx[: nnz.value], self._pull_val[: nnz.value])
        self._synced[j] = (id(x), x._version)
        self._zero[j] = nnz.value == 0

    def _gradient_vector(self, j):
        """Ax + b of problem j as the handle holds it (p doubles)."""
        out = np.zeros(self.p)
        self._q(self._L.cdh_quad_get_gradient(self._h, j, _vp(out)))
        return out

    def _omega_of(self, j):
        om = self._omega
        return None if om is None else (om if om.ndim == 1 else om[:, j])

    # -- the driver ----------------------------------------------------------------------------
    def _coordinate_descent(self, x, g, options):
        xs = list(x) if self.batched else [x]
        if self.batched and (isinstance(x, SparseIterate) or len(xs) != self.m):
            raise ArgumentError("a batch takes a list of one SparseIterate per problem")
        gl = [g] * self.m if isinstance(g, ProxL1) else list(g)
        if len(gl) != self.m:
            raise ArgumentError("need one ProxL1, or one per problem")
        for xj, gj in zip(xs, gl):
            _check_dims(xj, self, gj)
        self._set_penalties(g if isinstance(g, ProxL1) else gl)
        if options.warmStart:
            for j, xj in enumerate(xs):
                self._ensure_synced(xj, j)
        o, st = options._c(), (cdh_stats * self.m)()
        self._q(self._L.cdh_quad_coordinate_descent(self._h, C.byref(o), st))
        stats = [_stats(s) for s in st]
        self.last_stats = stats if self.batched else stats[0]
        for j, xj in enumerate(xs):
            self._pull(xj, j)
        return x


def initialize_(f, x, problem=0):
    """initialize!(f, x): r = y - Xβ (src/cd_differentiable_function.jl:59-72); CDQuadraticLoss: Ax (:311-320)."""
    if isinstance(f, CDQuadraticLoss):
        j = f._problem(problem)
        f._ensure_synced(x, j)
        f._q(f._L.cdh_quad_initialize(f._h))
        return
    f._push(x, rebuild=True)


def gradient(f, x, k, problem=0):
    """gradient(f, x, k) (src/cd_differentiable_function.jl:75-76, 234-235; CDQuadraticLoss: Ax[k] + b[k], :321-322)."""
    if isinstance(f, CDQuadraticLoss):
        j = f._problem(problem)
        f._ensure_synced(x, j)
        return float(f._gradient_vector(j)[int(k) - 1])
    f._ensure_synced(x)
    out = C.c_double()
    check(f._L.cdh_gradient(f._h, int(k), C.byref(out)), f._h)
    return out.value


def descendCoordinate_(f, g, x, k, problem=0):
    """descendCoordinate!(f, g, x, k) -> h (src/cd_differentiable_function.jl:83-111, 242-291; CDQuadraticLoss: :324-348)."""
    if isinstance(f, CDQuadraticLoss):
        j = f._problem(problem)
        f._set_penalty(g, j)
        f._ensure_synced(x, j)
        out = C.c_double()
        f._q(f._L.cdh_quad_descend(f._h, j, int(k), C.byref(out)))
        f._pull(x, j)
        return out.value
    f._set_penalty(g)
    f._ensure_synced(x)
    out = C.c_double()
    check(f._L.cdh_descend(f._h, int(k), C.byref(out)), f._h)
    f._pull(x)
    return out.value


# --------------------------------------------------------------------------------------
# Coordinate schedulers (src/atom_iterator.jl) -- host objects; the library has its own
# copy of the same logic for whole solves.
# --------------------------------------------------------------------------------------
class OrderedIterator:
    def __init__(self, iterate):
        self.iterate, self.fullPass = iterate, True

    def __iter__(self):
        if self.fullPass:
            return iter(range(1, numCoordinates(self.iterate) + 1))
        return iter(self.iterate.nzval2ind.tolist())

    def __len__(self):
        return numCoordinates(self.iterate) if self.fullPass else self.iterate.nnz


class RandomIterator:
    """Fisher-Yates with the documented splitmix64 substitute for Julia's global RNG."""

    def __init__(self, iterate, seed=0):
        self.iterate, self.fullPass = iterate, True
        self.order = list(range(1, numCoordinates(iterate) + 1))
        self._state = int(seed) & 0xFFFFFFFFFFFFFFFF

    def _next(self):
        m = 0xFFFFFFFFFFFFFFFF
        self._state = (self._state + 0x9E3779B97F4A7C15) & m
        z = self._state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)

    def __iter__(self):
        L = len(self)
        if self.fullPass:
            return iter(self.order[:L])
        sup = self.iterate.nzval2ind
        return iter([int(sup[o - 1]) for o in self.order[:L]])

    def __len__(self):
        return numCoordinates(self.iterate) if self.fullPass else self.iterate.nnz


def reset_(it, fullPass):
    """reset!(it, fullPass) (src/atom_iterator.jl:34-37, 53-64)."""
    it.fullPass = bool(fullPass)
    if isinstance(it, RandomIterator):
        L = len(it)
        for i in range(L):
            it.order[i] = i + 1
        for i in range(L - 1):
            j = i + it._next() % (L - i)
            it.order[i], it.order[j] = it.order[j], it.order[i]
    return it


# --------------------------------------------------------------------------------------
# Driver (src/coordinate_descent.jl)
# --------------------------------------------------------------------------------------
def _check_dims(x, f, g):
    if numCoordinates(x) != numCoordinates(f):  # :13
        raise DimensionMismatch("numCoordinates(x) != numCoordinates(f)")
    if g.lam is not None and g.lam.shape[0] != numCoordinates(f):  # :14-16
        raise DimensionMismatch("length(g.λ) != numCoordinates(f)")


def _stats(st):
    return {"passes": st.passes, "full_passes": st.full_passes, "visits": st.visits,
            "converged": bool(st.converged), "domain_error": bool(st.domain_error),
            "maxH": st.maxH, "lambda_max": st.lambda_max}


def coordinateDescent_(x, f, g, options=None):
    """coordinateDescent!(x, f, g::ProxL1, options=CDOptions()) (src/coordinate_descent.jl:7-39).
    Returns x; pass/convergence statistics are left in f.last_stats."""
    options = options or CDOptions()
    if isinstance(f, CDQuadraticLoss):       # a single problem, or a batch: lists of iterates and penalties, one launch
        return f._coordinate_descent(x, g, options)
    _check_dims(x, f, g)
    f._set_penalty(g)
    f._ensure_synced(x)
    o, st = options._c(), cdh_stats()
    status = f._L.cdh_coordinate_descent(f._h, C.byref(o), C.byref(st))
    check(status, f._h)
    f.last_stats = _stats(st)
    f._pull(x)
    if st.domain_error:
        raise DomainError("sqrt-lasso update took sqrt of a negative (λ² ≥ ‖X_k‖² ?)")
    return x


def cdPass_(x, f, g, visit, problem=0):
    """_cdPass!(x, f, g, it) (src/coordinate_descent.jl:94-110) over an explicit 1-based
    visit list; returns maxH."""
    if isinstance(visit, np.ndarray) and visit.dtype == np.int64 and visit.flags.c_contiguous:
        idx = visit                      # a prepared list crosses as is (sweep loops reuse one)
    else:
        idx = np.ascontiguousarray(list(visit), dtype=np.int64)
    out = C.c_double()
    if isinstance(f, CDQuadraticLoss):
        j = f._problem(problem)
        f._set_penalty(g, j)
        f._ensure_synced(x, j)
        f._q(f._L.cdh_quad_pass(f._h, j, idx.shape[0], _vp(idx), C.byref(out)))
        f._pull(x, j)
        return out.value
    f._set_penalty(g)
    f._ensure_synced(x)
    check(f._L.cdh_pass(f._h, idx.shape[0], _vp(idx), C.byref(out)), f._h)
    f._pull(x)
    return out.value


def findLambdaMax(x, f, g, problem=0):
    """_findLambdaMax(x, f, g) (src/coordinate_descent.jl:118-149)."""
    if isinstance(f, CDQuadraticLoss):       # max_k |gradient(f, x, k)| / omega_k, on the host from the handle's Ax + b
        j = f._problem(problem)
        f._ensure_synced(x, j)
        t = np.abs(f._gradient_vector(j))
        if g.lam is not None:
            t = t / g.lam
        return float(t.max())
    f._set_penalty(g)
    f._ensure_synced(x)
    out = C.c_double()
    check(f._L.cdh_lambda_max(f._h, C.byref(out)), f._h)
    return out.value


def stdX(f, weighted=False):
    """_stdX!(out, X) (src/utils.jl:127-138) for the X resident behind loss f; weighted: _stdX!(out, w, X) (:140-151)
    with the observation weights of a CDWeightedLSLoss."""
    out = np.zeros(f.p)
    check((f._L.cdh_col_wrms if weighted else f._L.cdh_col_rms)(f._h, _vp(out)), f._h)
    return out


def getLoadings(f):
    """_getLoadings!(out, X, e) (src/utils.jl:153-164) at e = f.r: Γ_j = sqrt(Σ_i (X_ij r_i)² / n) for the X resident behind
    loss f, one pass over X on the device (cdh_loadings).  Read-only on the handle."""
    out = np.zeros(f.p)
    check(f._L.cdh_loadings(f._h, _vp(out)), f._h)
    return out


def objective(f, g=None, problem=0):
    """f(β) + λ0 Σ ω|β| at the handle's current state (src/coordinate_descent.jl:1-3)."""
    if isinstance(f, CDQuadraticLoss):       # x'Ax/2 + x'b = sum_k x_k (g_k + b_k) / 2 with g = Ax + b as the handle holds it
        j = f._problem(problem)
        x = SparseIterate(f.p)
        f._pull(x, j)
        f._synced[j] = None
        k, grad = x._slot2ind[: x.nnz], f._gradient_vector(j)
        val = float(np.sum(x._val[: x.nnz] * (grad[k] + f.b[k, j]) * 0.5))
        if g is not None:
            om = np.ones(x.nnz) if g.lam is None else g.lam[k]
            val += g.lambda0 * float(np.sum(np.abs(x._val[: x.nnz]) * om))
        return val
    if isinstance(f, CDLogisticLoss):        # F itself, not the weighted least squares of the round the handle is in
        return f.objective(g)
    if g is not None:
        f._set_penalty(g)
    out = C.c_double()
    check(f._L.cdh_objective(f._h, C.byref(out)), f._h)
    return out.value


# --------------------------------------------------------------------------------------
# Front-ends (src/lasso.jl)
# --------------------------------------------------------------------------------------
@dataclass
class LassoSolution:
    """LassoSolution (src/lasso.jl:7-17)."""
    x: SparseIterate
    residuals: np.ndarray
    penalty: ProxL1
    sigma: float


def _std_resid(f):
    """std(f.r) as Statistics.std computes it: the mean, then the centred sum of squares (two passes on the device),
    Bessel-corrected (cdh_resid_std)."""
    out = C.c_double()
    check(f._L.cdh_resid_std(f._h, C.byref(out), None), f._h)
    return float(out.value)


def solve_screening_ols(G, c, xt_r_of, refinements=2):
    """Xs \\ y (src/utils.jl:70; a QR in the reference) from the Gram block G = Xs'Xs and c = Xs'y: the minimum-norm solution
    of the normal equations through the symmetric eigendecomposition of G (directions whose eigenvalue is below 1e-13 of the
    largest are left out, as a rank-revealing QR leaves them out), then refined against the normal equations' own residual
    Xs'(y - Xs b), which `xt_r_of(b)` evaluates on the device -- so that near-collinear screening columns do not cost the
    squared condition number in the fitted values."""
    w, V = np.linalg.eigh(G)
    keep = w > 1e-13 * max(w[-1], 0.0)
    Vk = V[:, keep]
    pinv = (Vk / w[keep]) @ Vk.T
    b = pinv @ c
    for _ in range(refinements):
        b = b + pinv @ xt_r_of(b)
    return b


def _as_loss(cls, X, y):
    return X if isinstance(X, _HipLoss) else cls(y, X)


def lasso(X, y, lam, omega=None, options=None):
    """lasso(X, y, λ[, ω], options) (src/lasso.jl:26-53).  X may also be an existing
    CDLeastSquaresLoss (data already resident in HBM); y is then ignored."""
    f = _as_loss(CDLeastSquaresLoss, X, y)
    x = SparseIterate(f.p)
    g = ProxL1(lam, omega)
    coordinateDescent_(x, f, g, options)
    return LassoSolution(x, f.r, g, _std_resid(f))


def sqrtLasso(X, y, lam, omega=None, options=None, standardizeX=True):
    """sqrtLasso (src/lasso.jl:62-98).  standardizeX=True uses ω = _stdX!(X), the behaviour
    the reference intends (its branch is dead on Julia >= 1.0)."""
    f = _as_loss(CDSqrtLassoLoss, X, y)
    x = SparseIterate(f.p)
    if omega is None and standardizeX:
        omega = stdX(f)
    g = ProxL1(lam, omega)
    coordinateDescent_(x, f, g, options)
    return LassoSolution(x, f.r, g, _std_resid(f))


def _ols_on_columns(f, idx1):
    """X[:, S] \\ y for the 1-based column list idx1 of a handle that stands at β = 0 (r = y), with nothing n-sized on the
    host: cdh_gram gives (X_S'X_S, X_S'y), the host solves the |S| x |S| system and refines it against X_S'(y - X_S b),
    which initialize! and one pass over the |S| columns evaluate on the device.  The handle is left at the last refinement's
    iterate; the caller sets what it wants and drops f._synced."""
    L, m = f._L, idx1.shape[0]
    G, c = np.zeros((m, m)), np.zeros(m)
    check(L.cdh_gram(f._h, m, _vp(idx1), _vp(G), _vp(c), None), f._h)

    def normal_residual(b):                  # Xs'(y - Xs b): initialize! forms the residual, one pass over the s columns dots it
        check(L.cdh_initialize(f._h, f.p, m, _vp(idx1), _vp(np.ascontiguousarray(b))), f._h)
        out = np.zeros(m)
        check(L.cdh_xt_r_cols(f._h, m, _vp(idx1), _vp(out)), f._h)
        return out

    return solve_screening_ols(G, c, normal_residual)      # Xs \ y


def _find_init_residuals(f, s):
    """_findInitResiduals! (src/utils.jl:65-77, 96-106): leaves r = y - X_S (X_S \\ y) on the device, S the s columns most
    correlated with y.  Everything n-sized stays in HBM: the screening scores X'y and the s x s normal equations
    (X_S'X_S, X_S'y) come from one pass each over the columns involved, the host solves the s x s system, and the residual
    y - X_S b is formed by initialize! on the device (s is 5 by default)."""
    L = f._L
    check(L.cdh_initialize(f._h, f.p, 0, None, None), f._h)  # beta = 0, r = y: X'r == X'y
    f._synced = None
    out = np.zeros(f.p)
    check(L.cdh_xt_r(f._h, _vp(out)), f._h)
    xty = np.abs(out)
    thr = np.sort(xty)[::-1][s - 1]
    S = np.nonzero(xty >= thr)[0]            # `storage .>= nlargest(s, storage)[end]`: ties kept
    if len(S) > 4096:
        raise ArgumentError("screening set larger than 4096 columns")
    idx1 = np.ascontiguousarray(S + 1, dtype=np.int64)
    coef = _ols_on_columns(f, idx1)
    check(L.cdh_initialize(f._h, f.p, len(S), _vp(idx1), _vp(np.ascontiguousarray(coef))), f._h)
    f._synced = None


def _find_init_sigma(f, s):
    """_findInitSigma! (src/utils.jl:60-64): std of the OLS residuals on the s columns most correlated with y."""
    _find_init_residuals(f, s)
    return _std_resid(f)                     # std(y - Xs * (Xs \ y))


def scaledLasso_(x, X, y, lam, omega, options=None):
    """scaledLasso!(x, X, y, λ, ω, options) (src/lasso.jl:107-144)."""
    o = options or IterLassoOptions()
    f = _as_loss(CDLeastSquaresLoss, X, y)
    n = f.n_total
    if o.initProcedure == "Screening":
        sigma = _find_init_sigma(f, o.sinit)
    elif o.initProcedure == "InitStd":
        sigma = o.sigmainit
    elif o.initProcedure == "WarmStart":
        initialize_(f, x)
        sigma = _std_resid(f)
    else:
        raise ArgumentError("Incorrect initialization Symbol")  # :128
    g = ProxL1(lam * sigma, omega)
    for _ in range(o.maxIter):
        coordinateDescent_(x, f, g, o.optionsCD)
        s, ss = C.c_double(), C.c_double()
        check(f._L.cdh_resid_moments(f._h, C.byref(s), C.byref(ss)), f._h)
        sigmanew = float(np.sqrt(ss.value / n))  # :134
        if abs(sigmanew - sigma) / sigma < o.optTol:
            break
        sigma = sigmanew
        g = ProxL1(lam * sigma, omega)
    return LassoSolution(x, f.r, g, _std_resid(f))


def feasibleLasso_(x, X, y, lam0, options=None):
    """feasibleLasso!(x, X, y, λ0, options) (src/lasso.jl:154-194): the lasso with the heteroscedasticity-robust penalty
    loadings Γ_j = sqrt(Σ_i (X_ij r_i)² / n), re-estimated from the residual after every solve until
    max|Γold - Γ| / max Γ < optTol.  X may also be an existing CDLeastSquaresLoss; y is then ignored.

    This is the behaviour the reference intends: its own function cannot run on Julia >= 1.0, because `Array{T}(p)`
    (:164-165) is no longer a constructor (as in sqrtLasso) and `LassoSolution(x, f.r, g, std(f.r))`
    (:193) names an outer constructor the struct does not have (:7-17 define `LassoSolution{T, S}(...)` only).

    One quirk is kept: `g = ProxL1(λ0, Γ)` (:181) aliases Γ, which `_getLoadings!` (:186) overwrites in place, so the
    penalty of the returned LassoSolution carries the loadings computed AFTER the last solve, not the ones it used.

    The loadings are one pass over X on the device per round (cdh_loadings); only the p-vector comes to the host, where the
    stopping statistic is taken.  Nothing n-sized leaves HBM inside the loop."""
    o = options or IterLassoOptions()
    f = _as_loss(CDLeastSquaresLoss, X, y)
    if o.initProcedure == "Screening":
        _find_init_residuals(f, o.sinit)                     # :169
    elif o.initProcedure == "InitStd":
        coordinateDescent_(x, f, ProxL1(lam0 * o.sigmainit, stdX(f)), o.optionsCD)   # :171-173
    elif o.initProcedure == "WarmStart":
        initialize_(f, x)                                    # :175
    else:
        raise ArgumentError("Incorrect initialization Symbol")  # :177
    gamma = getLoadings(f)                                   # :179
    for _ in range(o.maxIter):
        gamma_old = gamma
        coordinateDescent_(x, f, ProxL1(lam0, gamma), o.optionsCD)
        gamma = getLoadings(f)                               # :186
        if np.max(np.abs(gamma_old - gamma)) / np.max(gamma) < o.optTol:   # :188
            break
    return LassoSolution(x, f.r, ProxL1(lam0, gamma), _std_resid(f))


@dataclass
class LassoPathResult:
    """LassoPath{T} (src/lasso.jl:201-204)."""
    lambdapath: list
    betapath: list


def refitLassoPath(path, X, Y):
    """refitLassoPath(path, X, Y) (src/lasso.jl:208-225): for every distinct support S along the path, the least-squares
    coefficients X[:, S] \\ Y.  Returns a dict from the sorted 1-based support (a tuple) to a float64 array; a support already
    seen is skipped, and the empty support maps to an empty array.  X may also be an existing CDLeastSquaresLoss; Y is then
    ignored.

    Per support the handle is initialised at β = 0 (r = y), cdh_gram gives (X_S'X_S, X_S'y), and the host solves the
    |S| x |S| system with the refinement _findInitResiduals! uses -- nothing n-sized on the host.  cdh_gram takes up to 4096
    columns: a larger support raises ArgumentError.  The handle is left at β = 0 with r = y (an iterate synced to it before
    the call is pushed again by its next use)."""
    f = _as_loss(CDLeastSquaresLoss, X, Y)
    out = {}
    for beta in path.betapath:
        S = tuple(int(k) + 1 for k in np.nonzero(beta.dense())[0])   # findall(!iszero, β)
        if S in out:
            continue
        if len(S) > 4096:
            raise ArgumentError("support larger than 4096 columns")
        check(f._L.cdh_initialize(f._h, f.p, 0, None, None), f._h)
        f._synced = None
        out[S] = _ols_on_columns(f, np.array(S, dtype=np.int64)) if S else np.zeros(0)
    check(f._L.cdh_initialize(f._h, f.p, 0, None, None), f._h)
    f._synced = None
    return out


def LassoPath(X, Y, lambdapath, options=None, max_hat_s=np.inf, standardizeX=True, reuse_residual=True):
    """LassoPath(X, Y, λpath, options; max_hat_s, standardizeX) (src/lasso.jl:229-260):
    one x and one f shared by all λ (warm starts), βpath[i] = copy(x)."""
    f = _as_loss(CDLeastSquaresLoss, X, Y)
    sx = stdX(f) if standardizeX else np.ones(f.p)
    return _solve_path(f, lambdapath, sx, options, max_hat_s, reuse_residual)


def _solve_path(f, lambdapath, sx, options, max_hat_s, reuse_residual):
    """The loop of LassoPath (src/lasso.jl:250-257) on whatever loss f is by now, with the penalty scales sx: a fresh x
    warm-started along λ.  LassoPath and the folds of cvLassoPath run it."""
    x = SparseIterate(f.p)
    lambdapath = list(lambdapath)
    betapath = []
    # x and f are shared by all lambdas; after the first solve the carried residual already
    # equals y - X x, so later warm starts skip the redundant initialize! (rounding-level effect)
    check(f._L.cdh_set_reuse_residual(f._h, 1 if reuse_residual else 0), f._h)
    # a path is many solves on one X: the gradient cache need not wait for evidence of that (1 -> 2 for the
    # duration of the path).  Whatever else the caller -- or CDH_GRADIENT_CACHE -- set on this loss stays: 0 is off.
    mode_before = f.gradient_cache_mode()
    if mode_before == 1:
        check(f._L.cdh_set_gradient_cache(f._h, 2), f._h)
    try:
        for i, lam in enumerate(lambdapath):
            coordinateDescent_(x, f, ProxL1(lam, sx), options)
            betapath.append(x.copy())
            if x.nnz > max_hat_s:
                lambdapath = lambdapath[: i + 1]
                break
    finally:
        check(f._L.cdh_set_reuse_residual(f._h, 0), f._h)
        if mode_before == 1:
            check(f._L.cdh_set_gradient_cache(f._h, 1), f._h)
    return LassoPathResult(lambdapath, betapath)


@dataclass
class CVLassoPathResult:
    """What cvLassoPath returns.  fold_mse[k, j] is the mean squared prediction error of λ_j on the rows of fold k by the
    path fitted without them, train_mse[k, j] the same on the rows it was fitted on; cvm and cvsd weight the folds by their
    sizes; the two indices are 0-based positions in lambdapath."""
    lambdapath: np.ndarray
    fold_sizes: np.ndarray
    fold_mse: np.ndarray
    train_mse: np.ndarray
    cvm: np.ndarray
    cvsd: np.ndarray
    index_min: int
    lambda_min: float
    index_1se: int
    lambda_1se: float
    path: LassoPathResult = None
    fold_paths: list = None


def _cv_fold_ids(n, K, folds, seed):
    """The 0-based fold of every row, checked on the host: a caller's array, or default_rng(seed).permutation(n) % K."""
    K = int(K)
    if K < 2 or K > 255 or K > n:
        raise ArgumentError("need 2 <= K <= 255 folds, and K <= n")
    if folds is None:
        ids = np.random.default_rng(seed).permutation(n) % K
    else:
        ids = np.asarray(folds)
        if ids.shape != (n,):
            raise ArgumentError("folds must hold one id per row")
        if not np.issubdtype(ids.dtype, np.integer):
            if not np.all(ids == np.floor(ids)):
                raise ArgumentError("fold ids must be integers")
        if ids.min() < 0 or ids.max() >= K:
            raise ArgumentError("fold ids must lie in 0 .. K - 1")
    ids = ids.astype(np.int32)
    sizes = np.bincount(ids, minlength=K)
    if np.any(sizes == 0):
        raise ArgumentError("fold %d is empty" % int(np.nonzero(sizes == 0)[0][0]))
    return ids, sizes


def _cv_select(lam, sizes, fold_mse):
    """cvm, cvsd and the two selection rules from the folds' errors."""
    n, K = sizes.sum(), len(sizes)
    wt = sizes / n
    cvm = wt @ fold_mse
    cvsd = np.sqrt(wt @ (fold_mse - cvm) ** 2 / (K - 1))
    imin = int(np.argmin(cvm))
    ok = np.nonzero(cvm <= cvm[imin] + cvsd[imin])[0]
    i1se = int(ok[np.argmax(lam[ok])])           # the largest λ within one standard error; argmax takes the lowest index of a tie
    return cvm, cvsd, imin, i1se


def cvLassoPath(X, Y, lambdapath, K=10, folds=None, options=None, standardizeX=True, seed=0, full_path=True,
                keep_fold_paths=False):
    """K-fold cross-validation of LassoPath(X, Y, λpath, options; standardizeX) (src/lasso.jl:229-260) on the device; no
    reference counterpart.  X may also be an existing CDLeastSquaresLoss (Y is then ignored); the design is uploaded once.

    A fold is a 0/1 observation weight: LassoPath on the n_k training rows of fold k has the same iterates as the weighted
    loss on all n rows with ω = _stdX!(w, X) and λ·sqrt(n_k / n) (standardizeX=False: ω = 1 and λ·n_k / n).  So per fold
    the weights are written on the device from the resident fold ids (cdh_set_fold_weights), the whole path is solved
    warm-started along λ exactly as LassoPath solves it, and one pass over the union support of the fold's path
    (cdh_path_sse) gives the held-out and training errors of every λ.  Nothing n-sized moves after the upload.

    folds: 0-based ids, one per row; otherwise np.random.default_rng(seed).permutation(n) % K.  There is no max_hat_s: the
    folds would be truncated at different λ.  A handle that was passed in is switched to the weighted loss for the folds
    and is back on least squares, without folds, when the call returns or raises (an iterate synced to it before the call
    is pushed again by its next use).  `path` is LassoPath on all rows (None with full_path=False), `fold_paths` the K
    fold paths as LassoPathResult (None unless keep_fold_paths)."""
    if isinstance(X, CoordinateDifferentiableFunction) and not isinstance(X, CDLeastSquaresLoss):
        raise TypeError("MethodError: cvLassoPath takes a matrix or a CDLeastSquaresLoss")
    lam = np.array(list(lambdapath), dtype=np.float64)
    if lam.size == 0:
        raise ArgumentError("lambdapath is empty")
    n = X.n if isinstance(X, _HipLoss) else np.shape(X)[0]
    ids, sizes = _cv_fold_ids(int(n), K, folds, seed)
    if isinstance(X, _HipLoss):
        return _cv_lasso_path(X, lam, ids, sizes, options, standardizeX, full_path, keep_fold_paths)
    f = CDLeastSquaresLoss(Y, X)
    try:
        return _cv_lasso_path(f, lam, ids, sizes, options, standardizeX, full_path, keep_fold_paths)
    finally:
        f.close()                  # the handle this call made goes with it, also when a fold raises


def _cv_lasso_path(f, lam, ids, sizes, options, standardizeX, full_path, keep_fold_paths):
    n, K, m = f.n, len(sizes), lam.size
    if f.n_total != f.n:
        raise ArgumentError("cvLassoPath does not run on row-sharded handles")
    fold_mse, train_mse = np.zeros((K, m)), np.zeros((K, m))
    fold_paths = [] if keep_fold_paths else None
    try:
        check(f._L.cdh_set_loss(f._h, CDH_WLS), f._h)
        f._synced = None
        f.set_folds(ids, K)
        for k in range(K):
            f.set_fold_weights(k)
            nk = n - sizes[k]
            sx = stdX(f, weighted=True) if standardizeX else np.ones(f.p)
            scale = np.sqrt(nk / n) if standardizeX else nk / n
            res = _solve_path(f, lam * scale, sx, options, np.inf, True)
            beta = np.stack([b.dense() for b in res.betapath], axis=1)         # p x m
            S = np.nonzero(np.any(beta != 0.0, axis=1))[0]
            if len(S) > 4096:
                raise ArgumentError("union support of a fold's path larger than 4096 columns")
            if len(S) == 0:
                S, B = np.zeros(1, dtype=np.int64), np.zeros((1, m))          # held-out SSE = Σ y² over the fold
            else:
                B = beta[S, :]
            for j0 in range(0, m, 1024):
                held, train = f.path_sse(k, S + 1, B[:, j0:j0 + 1024])
                fold_mse[k, j0:j0 + 1024] = held / sizes[k]
                train_mse[k, j0:j0 + 1024] = train / nk
            if keep_fold_paths:
                fold_paths.append(LassoPathResult(list(lam), res.betapath))
    finally:
        f._synced = None
        f.set_folds(None, 0)
        check(f._L.cdh_set_loss(f._h, CDH_LS), f._h)
    cvm, cvsd, imin, i1se = _cv_select(lam, sizes, fold_mse)
    path = LassoPath(f, None, lam, options, standardizeX=standardizeX) if full_path else None
    return CVLassoPathResult(lam, sizes, fold_mse, train_mse, cvm, cvsd, imin, float(lam[imin]), i1se, float(lam[i1se]),
                             path, fold_paths)


# --------------------------------------------------------------------------------------
# l1-penalised logistic regression by IRLS (no reference counterpart)
# --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class IRLSOptions:
    """The outer loop of logisticLasso_: at most maxIter rounds, stopped when max_j |Δβ_j| < optTol between two rounds; the
    working weights are clamped below at wmin (only the weights: the fixed point keeps the KKT conditions of F).  etaMax
    (the Poisson family only) caps the linear predictor before exp: a chosen guard, not a measurement -- exp and w x² stay
    finite, and it is far beyond any fitted model."""
    maxIter: int = 25
    optTol: float = 1e-7
    wmin: float = 1e-5
    etaMax: float = 50.0


@dataclass
class LogisticLassoSolution:
    """What logisticLasso_ and logisticLasso return.  nll is (1/n) Σ [log(1 + e^η) - y η] at the final β; monotone is False
    if the penalised objective F rose between two rounds by more than 1e-10 max(1, F) (there is no step halving: the rise is
    only reported); intercept is None unless one was fitted."""
    x: SparseIterate
    nll: float
    rounds: int
    converged: bool
    monotone: bool
    intercept: float = None
    penalty: ProxL1 = None
    held_nll: float = None       # with fold=k: Σ nll_i and Σ misclassification over the held-out rows at the final β
    held_miss: float = None


@dataclass
class LogisticLassoPathResult(LassoPathResult):
    """LassoPathResult with, per λ, the nll at the solution, the IRLS rounds taken, convergence and the intercept."""
    nll: list = None
    rounds: list = None
    converged: list = None
    intercepts: list = None


@dataclass
class CVLogisticLassoPathResult:
    """What cvLogisticLassoPath returns.  Per fold k and λ_j, by the path fitted without the rows of fold k:
    fold_deviance[k, j] = 2 Σ nll_i / size_k and fold_class[k, j] = misclassified rows / size_k over the held-out rows,
    train_deviance[k, j] = 2 Σ nll_i / n_k over the rows it was fitted on, rounds and converged of its IRLS loop.  cvm, cvsd
    and the two selections (0-based positions in lambdapath) are taken from `measure`, the folds weighted by their sizes."""
    lambdapath: np.ndarray
    fold_sizes: np.ndarray
    fold_deviance: np.ndarray
    train_deviance: np.ndarray
    fold_class: np.ndarray
    rounds: np.ndarray
    converged: np.ndarray
    measure: str
    cvm: np.ndarray
    cvsd: np.ndarray
    index_min: int
    lambda_min: float
    index_1se: int
    lambda_1se: float
    path: LogisticLassoPathResult = None
    fold_paths: list = None


@dataclass
class PoissonLassoSolution:
    """What poissonLasso_ and poissonLasso return.  nll is (1/n) Σ [μ_i - y_i η_i] and deviance Σ dev_i over the training rows
    at the final β; capped counts the rows whose η the final step capped at etaMax; monotone is False if the penalised
    objective F rose between two rounds by more than 1e-10 max(1, F) (there is no step halving: the rise is only reported);
    intercept is None unless one was fitted; held_deviance (with fold=k) is Σ dev_i over the held-out rows."""
    x: SparseIterate
    nll: float
    deviance: float
    rounds: int
    converged: bool
    monotone: bool
    capped: int = 0
    intercept: float = None
    penalty: ProxL1 = None
    held_deviance: float = None


@dataclass
class PoissonLassoPathResult(LassoPathResult):
    """LassoPathResult with, per λ, the nll and the deviance at the solution, the IRLS rounds taken, convergence and the
    intercept."""
    nll: list = None
    deviance: list = None
    rounds: list = None
    converged: list = None
    intercepts: list = None


@dataclass
class CVPoissonLassoPathResult:
    """What cvPoissonLassoPath returns.  Per fold k and λ_j, by the path fitted without the rows of fold k:
    fold_deviance[k, j] = Σ dev_i / size_k over the held-out rows, train_deviance[k, j] = Σ dev_i / n_k over the rows it was
    fitted on, rounds and converged of its IRLS loop.  cvm, cvsd and the two selections (0-based positions in lambdapath) are
    taken from fold_deviance, the folds weighted by their sizes."""
    lambdapath: np.ndarray
    fold_sizes: np.ndarray
    fold_deviance: np.ndarray
    train_deviance: np.ndarray
    rounds: np.ndarray
    converged: np.ndarray
    measure: str
    cvm: np.ndarray
    cvsd: np.ndarray
    index_min: int
    lambda_min: float
    index_1se: int
    lambda_1se: float
    path: PoissonLassoPathResult = None
    fold_paths: list = None


@dataclass
class CoxLassoSolution:
    """What coxLasso_ and coxLasso return.  nll is (1/n) Σ δ_i (log S_i - η_i) over the training rows at the final β and
    events the events among them (Σ v_i δ_i, a float, on a loss with observation weights; so is held_events); capped counts the rows whose η the final step capped at etaMax; monotone is False if the
    penalised objective F rose between two rounds by more than 1e-10 max(1, F) (there is no step halving: the rise is only
    reported).  With fold=k: held_deviance = -2 (ℓ_all - ℓ_train) and held_events, the events among the held-out rows."""
    x: SparseIterate
    nll: float
    rounds: int
    converged: bool
    monotone: bool
    capped: int = 0
    events: int = 0
    penalty: ProxL1 = None
    held_deviance: float = None
    held_events: int = None


@dataclass
class CoxLassoPathResult(LassoPathResult):
    """LassoPathResult with, per λ, the nll at the solution, the IRLS rounds taken and convergence (intercepts: None
    throughout -- the Cox model has none)."""
    nll: list = None
    rounds: list = None
    converged: list = None
    intercepts: list = None


@dataclass
class CVCoxLassoPathResult:
    """What cvCoxLassoPath returns.  Per fold k and λ_j, by the path fitted without the rows of fold k:
    fold_deviance[k, j] = -2 (ℓ_all - ℓ_train) / (held-out events of fold k), ℓ the log partial likelihood of all rows and of
    the training rows at that β; train_deviance[k, j] = -2 ℓ_train / (training events); rounds and converged of its IRLS
    loop.  cvm, cvsd and the two selections (0-based positions in lambdapath) are taken from fold_deviance, the folds
    weighted by their held-out events (fold_events)."""
    lambdapath: np.ndarray
    fold_sizes: np.ndarray
    fold_deviance: np.ndarray
    train_deviance: np.ndarray
    rounds: np.ndarray
    converged: np.ndarray
    measure: str
    cvm: np.ndarray
    cvsd: np.ndarray
    index_min: int
    lambda_min: float
    index_1se: int
    lambda_1se: float
    path: CoxLassoPathResult = None
    fold_paths: list = None
    fold_events: np.ndarray = None


@dataclass
class CVCoxConcordancePathResult(CVCoxLassoPathResult):
    """What cvCoxLassoPath(measure="C") returns: CVCoxLassoPathResult with fold_concordance[k, j], Harrell's C of the held-out
    rows of fold k at the β of λ_j fitted without them.  cvm, cvsd and the two selections are taken from it, the folds
    weighted by their held-out Σ v (their sizes without weights): index_min is the position of the LARGEST cvm, index_1se the
    largest λ whose cvm is at least that maximum less its cvsd."""
    fold_concordance: np.ndarray = None


def _penalty_value(g, beta):
    return g.lambda0 * float(np.sum(np.abs(beta) * (1.0 if g.lam is None else g.lam)))


def _irls_rounds(x, f, g, options, irls, fold):
    """The outer loop of every family: f._irls(apply, irls, fold) is the family's f.irls_step with the caller's options and
    fold.  -> (the dict of the read-only step that ends the solve, rounds, converged, monotone)."""
    options = options or CDOptions()
    if not options.warmStart:
        raise ArgumentError("the rounds of IRLS are warm starts: options.warmStart must be true")
    _check_dims(x, f, g)
    f._ensure_synced(x)
    check(f._L.cdh_set_reuse_residual(f._h, 1), f._h)
    rounds, converged, monotone, F_prev = 0, False, True, None

    def rose(F):
        return F_prev is not None and F - F_prev > 1e-10 * max(1.0, F_prev)

    try:
        beta = x.dense()
        for _ in range(int(irls.maxIter)):
            F = f._irls(True, irls, fold)["nll"] + _penalty_value(g, beta)      # F at the iterate this round starts from
            monotone, F_prev = monotone and not rose(F), F
            coordinateDescent_(x, f, g, options)
            rounds += 1
            beta, old = x.dense(), beta
            if float(np.max(np.abs(beta - old))) < irls.optTol:
                converged = True
                break
        f._ensure_synced(x)
        last = f._irls(False, irls, fold)
        monotone = monotone and not rose(last["nll"] + _penalty_value(g, beta))
    finally:
        check(f._L.cdh_set_reuse_residual(f._h, 0), f._h)
    return last, rounds, converged, monotone


def _logit_start(labels, weights=None):
    """The intercept of the null model: logit(ȳ), ȳ = Σvy / Σv with observation weights."""
    ybar = float(np.mean(labels)) if weights is None else float(np.sum(weights * labels) / np.sum(weights))
    if not 0.0 < ybar < 1.0:
        raise ArgumentError("fit_intercept needs labels of both kinds: the null model's intercept is infinite")
    return float(np.log(ybar / (1.0 - ybar)))


def _poisson_start(counts, offset=None, weights=None):
    """The intercept of the null model: log(Σy / Σ e^o), log(Σvy / Σ v e^o) with observation weights."""
    total = float(np.sum(counts)) if weights is None else float(np.sum(weights * counts))
    if not total > 0.0:
        raise ArgumentError("fit_intercept needs a positive count: the null model's intercept is -infinity")
    if weights is None:
        expo = float(len(counts)) if offset is None else float(np.sum(np.exp(offset)))
    else:
        expo = float(np.sum(weights)) if offset is None else float(np.sum(weights * np.exp(offset)))
    return float(np.log(total / expo))


def _split_intercept(x, p):
    """x of length p + 1 -> (its first p coordinates as a SparseIterate, the last)."""
    beta = x.dense()
    return SparseIterate(p, beta[:p]), float(beta[p])


# ---- what the front ends know of a family, and the front ends written once ----------------------------------------------
@dataclass(frozen=True)
class _GLMFamily:
    name: str                    # "logistic", "poisson": the front ends' names (logisticLasso_, cvLogisticLassoPath, ...)
    loss: type
    start: object                # (observations, offset or None, weights or None) -> the null model's intercept, or the
                                 # family's refusal
    observed: object             # f -> (observations, offset or None, weights or None), fetched from the loss
    start_before_upload: bool    # a matrix's front ends refuse an infinite start before the upload (the Poisson ones), or
                                 # find it on the way: after the upload, a path from the labels the handle returns
    solution: object             # (x, the last read-only step's dict, rounds, converged, monotone, g) -> the Solution
    path_result: type
    path_fields: tuple           # the Solution's fields a path keeps per λ, between betapath and intercepts
    cv_result: type
    cv_measures: dict            # measure -> (sol, size_k) -> its value over the held-out rows; the first is fold_deviance
                                 # (size_k: the held-out rows, or their Σ v on a loss with observation weights)
    cv_train: object             # (sol, n, n_k) -> train_deviance (n_k: the training rows, or their Σ v)
    cv_weight: object = None     # sol -> the fold's weight in cvm and cvsd (None: the fold's size)


_LOGISTIC = _GLMFamily(
    name="logistic", loss=CDLogisticLoss, start=lambda labels, offset=None, weights=None: _logit_start(labels, weights),
    observed=lambda f: (f.labels, None, f._prior()), start_before_upload=False,
    solution=lambda x, last, rounds, converged, monotone, g: LogisticLassoSolution(
        x, last["nll"], rounds, converged, monotone, None, g, last.get("held_nll"), last.get("held_miss")),
    path_result=LogisticLassoPathResult, path_fields=("nll", "rounds", "converged"), cv_result=CVLogisticLassoPathResult,
    cv_measures={"deviance": lambda sol, size: 2.0 * sol.held_nll / size, "class": lambda sol, size: sol.held_miss / size},
    cv_train=lambda sol, n, nk: 2.0 * n * sol.nll / nk)

_POISSON = _GLMFamily(
    name="poisson", loss=CDPoissonLoss, start=_poisson_start,
    observed=lambda f: (f.counts, f.offset, f._prior()), start_before_upload=True,
    solution=lambda x, last, rounds, converged, monotone, g: PoissonLassoSolution(
        x, last["nll"], last["deviance"], rounds, converged, monotone, last["capped"], None, g, last.get("held_deviance")),
    path_result=PoissonLassoPathResult, path_fields=("nll", "deviance", "rounds", "converged"),
    cv_result=CVPoissonLassoPathResult,
    cv_measures={"deviance": lambda sol, size: sol.held_deviance / size},
    cv_train=lambda sol, n, nk: sol.deviance / nk)

_COX = _GLMFamily(
    name="cox", loss=CDCoxLoss, start=None, observed=lambda f: (f.status, f.offset, None), start_before_upload=False,
    solution=lambda x, last, rounds, converged, monotone, g: CoxLassoSolution(
        x, last["nll"], rounds, converged, monotone, last["capped"], last["events"], g, last.get("held_deviance"),
        last.get("held_events")),
    path_result=CoxLassoPathResult, path_fields=("nll", "rounds", "converged"), cv_result=CVCoxLassoPathResult,
    cv_measures={"deviance": lambda sol, size: sol.held_deviance / sol.held_events},
    cv_train=lambda sol, n, nk: 2.0 * n * sol.nll / sol.events,
    cv_weight=lambda sol: sol.held_events)


def _glm_solve(fam, x, f, g, options, irls, fold):
    if not isinstance(f, fam.loss):
        raise TypeError("MethodError: %sLasso_ takes a %s" % (fam.name, fam.loss.__name__))
    irls = irls or IRLSOptions()
    last, rounds, converged, monotone = _irls_rounds(x, f, g, options, irls, fold)
    return fam.solution(x, last, rounds, converged, monotone, g)


def _glm_loss(fam, X, y, fit_intercept, offset, extra=None):
    """-> (f, owned): the family's loss over X (with a trailing column of ones when an intercept is fitted).  extra: further
    keywords of the loss (the Cox family's strata and weights), None where not given; "ties" among them is the Cox family's
    tie rule, which is not a keyword of the loss: it is set on the loss right after it is built, and on a loss that was passed in
    it must be the loss's own."""
    extra = {k: v for k, v in (extra or {}).items() if v is not None}
    ties = extra.pop("ties", None)
    if isinstance(X, fam.loss):
        if fit_intercept:
            raise ArgumentError("fit_intercept appends a column of ones: pass the matrix, not a loss")
        if offset is not None:
            raise ArgumentError("the offset belongs to the loss: pass the matrix, or a loss made with it")
        for name in extra:
            raise ArgumentError("%s belongs to the loss: pass the matrix, or a loss made with it" % name)
        if ties is not None and ties != X.ties:
            raise ArgumentError('ties="%s" disagrees with the loss, whose rule is "%s": the tie rule belongs to the loss '
                                "(set_ties)" % (ties, X.ties))
        return X, False
    if isinstance(X, CoordinateDifferentiableFunction):
        raise TypeError("MethodError: takes a matrix or a %s" % fam.loss.__name__)
    X = np.asarray(X)
    if fit_intercept:
        X = np.asfortranarray(np.hstack([X, np.ones((X.shape[0], 1), dtype=X.dtype)]))
    f = fam.loss(y, X, **extra) if offset is None else fam.loss(y, X, offset, **extra)
    if ties is not None:
        try:
            f.set_ties(ties)
        except Exception:
            f.close()
            raise
    return f, True


def _glm_host_start(fam, y, offset, weights=None):
    return fam.start(np.asarray(y, dtype=np.float64), None if offset is None else np.asarray(offset, dtype=np.float64), weights)


def _glm_host_weights(X, fit_intercept, extra):
    """The observation weights a matrix's front end was given, checked and normalised as the loss will store them -- what
    an intercept's start is computed from; None without an intercept, without weights, or with a loss (which refuses them)."""
    v = (extra or {}).get("weights")
    if v is None or not fit_intercept or isinstance(X, CoordinateDifferentiableFunction):
        return None
    return _strata_weights(None, v, np.shape(X)[0])[1]


def _glm_early_start(fam, X, y, fit_intercept, offset, weights=None):
    if fit_intercept and fam.start_before_upload and not isinstance(X, CoordinateDifferentiableFunction):
        return _glm_host_start(fam, y, offset, weights)
    return None


def _glm_lasso(fam, X, y, lam, omega, options, irls, fit_intercept, offset=None, extra=None):
    v = _glm_host_weights(X, fit_intercept, extra)
    start = _glm_early_start(fam, X, y, fit_intercept, offset, v)
    f, owned = _glm_loss(fam, X, y, fit_intercept, offset, extra)
    try:
        p = f.p - (1 if fit_intercept else 0)
        om = None if omega is None else np.asarray(omega, dtype=np.float64)
        x = SparseIterate(f.p)
        if fit_intercept:
            om = np.r_[np.ones(p) if om is None else om, 0.0]
            x[p + 1] = _glm_host_start(fam, y, offset, v) if start is None else start
        sol = _glm_solve(fam, x, f, ProxL1(lam, om), options, irls, None)
        if fit_intercept:
            sol.x, sol.intercept = _split_intercept(x, p)
        return sol
    finally:
        if owned:
            f.close()


def _glm_path(fam, X, y, lambdapath, options, irls, max_hat_s, standardizeX, fit_intercept, offset=None, extra=None):
    start = _glm_early_start(fam, X, y, fit_intercept, offset, _glm_host_weights(X, fit_intercept, extra))
    f, owned = _glm_loss(fam, X, y, fit_intercept, offset, extra)
    try:
        return _glm_path_on(fam, f, lambdapath, options, irls, max_hat_s, standardizeX, fit_intercept, start)
    finally:
        if owned:
            f.close()


def _glm_keep(fam, res, sol, x, p, fit_intercept, nll=None):
    """One λ of a path: β (without the intercept), the family's fields of the solution -- nll as given, where the caller
    rescales it -- and the intercept.  -> β."""
    b, b0 = _split_intercept(x, p) if fit_intercept else (x.copy(), None)
    res.betapath.append(b)
    for name in fam.path_fields:
        getattr(res, name).append(nll if name == "nll" and nll is not None else getattr(sol, name))
    res.intercepts.append(b0)
    return b


def _glm_path_on(fam, f, lambdapath, options, irls, max_hat_s, standardizeX, fit_intercept, start=None):
    """The family's path on the loss f (its last column the column of ones when an intercept is fitted; start: the null
    model's intercept, where the caller has computed it from its host copies -- otherwise from what the loss returns)."""
    p = f.p - (1 if fit_intercept else 0)
    sx = stdX(f) if standardizeX else np.ones(f.p)
    x = SparseIterate(f.p)
    if fit_intercept:
        sx[p] = 0.0
        x[p + 1] = fam.start(*fam.observed(f)) if start is None else start
    lambdapath = list(lambdapath)
    res = fam.path_result(lambdapath, [], *[[] for _ in fam.path_fields], [])
    mode_before = f.gradient_cache_mode()          # a path is many solves on one X, as in _solve_path: 1 -> 2 for its duration
    if mode_before == 1:
        check(f._L.cdh_set_gradient_cache(f._h, 2), f._h)
    try:
        for i, lam in enumerate(lambdapath):
            sol = _glm_solve(fam, x, f, ProxL1(lam, sx), options, irls, None)
            if _glm_keep(fam, res, sol, x, p, fit_intercept).nnz > max_hat_s:
                res.lambdapath = lambdapath[: i + 1]
                break
    finally:
        if mode_before == 1:
            check(f._L.cdh_set_gradient_cache(f._h, 1), f._h)
    return res


def _cv_glm_path(fam, X, y, lambdapath, K, folds, options, irls, standardizeX, fit_intercept, seed, measure, offset,
                 full_path, keep_fold_paths, extra=None, after_solve=None):
    """after_solve(f, k, j): called after the solve of fold k at λ_j, at the β it left (None: nothing is called)."""
    front = "cv%sLassoPath" % fam.name.capitalize()
    if measure not in fam.cv_measures:
        raise ArgumentError("measure must be " + " or ".join('"%s"' % m for m in fam.cv_measures))
    if isinstance(X, CoordinateDifferentiableFunction) and not isinstance(X, fam.loss):
        raise TypeError("MethodError: %s takes a matrix or a %s" % (front, fam.loss.__name__))
    lam = np.array(list(lambdapath), dtype=np.float64)
    if lam.size == 0:
        raise ArgumentError("lambdapath is empty")
    n = X.n if isinstance(X, _HipLoss) else np.shape(X)[0]
    ids, sizes = _cv_fold_ids(int(n), K, folds, seed)
    obs = off = v = None
    if fit_intercept and not isinstance(X, _HipLoss):
        obs = np.ascontiguousarray(y, dtype=np.float64)
        off = None if offset is None else np.ascontiguousarray(offset, dtype=np.float64)
        v = _glm_host_weights(X, fit_intercept, extra)
        fam.start(obs, off, v)
        for k in range(len(sizes)):                     # before the upload: a fold whose start would be infinite
            fam.start(obs[ids != k], None if off is None else off[ids != k], None if v is None else v[ids != k])
    f, owned = _glm_loss(fam, X, y, fit_intercept, offset, extra)
    try:
        return _cv_glm_path_on(fam, front, f, owned, lam, ids, sizes, options, irls, standardizeX, fit_intercept, obs, off,
                               measure, full_path, keep_fold_paths, after_solve)
    finally:
        if owned:
            f.close()                  # the handle this call made goes with it, also when a fold raises


def _cv_glm_path_on(fam, front, f, owned, lam, ids, sizes, options, irls, standardizeX, fit_intercept, obs, off, measure,
                    full_path, keep_fold_paths, after_solve=None):
    n, K, m = f.n, len(sizes), lam.size
    if f.n_total != f.n:
        raise ArgumentError("%s does not run on row-sharded handles" % front)
    p = f.p - (1 if fit_intercept else 0)
    held, tdev = {name: np.zeros((K, m)) for name in fam.cv_measures}, np.zeros((K, m))
    rounds, conv = np.zeros((K, m), dtype=np.int64), np.zeros((K, m), dtype=bool)
    fold_paths = [] if keep_fold_paths else None
    # Observation weights v (the binomial and the Poisson family; they sum to n): fold k's problem is the weighted path on its
    # training rows with their weights renormalised to sum to n_k, F_k = (1/V_k) Σ_train v nll + λ Σ ω|β|, V_k = Σ_train v;
    # the handle minimises (1/n) Σ_train v nll + λ' Σ ω|β|, so λ' = λ V_k / n, and the held-out sums divide by Σ_held v.
    # Without weights V_k = n_k and Σ_held v = size_k: today's numbers.
    v = f._prior()
    held_v = sizes if v is None else np.bincount(ids, weights=v, minlength=K)
    wts = held_v if fam.cv_weight is None else np.zeros(K)
    if fit_intercept and obs is None:
        obs, off, _ = fam.observed(f)                    # (a loss that was passed in has no intercept: not reached in practice)
    # The path on all rows.  On the handle this call has just made it runs FIRST: the very calls the family's path makes on a
    # fresh handle, so the same bits (after the folds an intercept's start η = b0 would be read as y - (y - b0) off the working
    # response they left, and the handle's cache policy has a history).  A loss that was passed in gets it LAST, and comes
    # back as the family's path leaves it: the weights of all rows, no folds.
    path = None
    if full_path and owned:
        path = _glm_path_on(fam, f, lam, options, irls, np.inf, standardizeX, fit_intercept,
                            fam.start(obs, off, v) if fit_intercept else None)
    mode_before = f.gradient_cache_mode()                # a path is many solves on one X, as in _solve_path: 1 -> 2 for its duration
    try:
        f.set_folds(ids, K)
        if mode_before == 1:
            check(f._L.cdh_set_gradient_cache(f._h, 2), f._h)
        for k in range(K):
            f.set_fold_weights(k)
            nk = n - sizes[k]
            sx = stdX(f, weighted=True) if standardizeX else np.ones(f.p)     # while w still holds the 0/1 weights
            scale = np.sqrt(nk / n) if standardizeX else nk / n
            vk = nk if v is None else float(np.sum(v[ids != k]))              # V_k
            if v is not None:
                scale = (vk / n) / np.sqrt(nk / n) if standardizeX else vk / n
            x = SparseIterate(f.p)
            if fit_intercept:
                sx[p] = 0.0
                x[p + 1] = fam.start(obs[ids != k], None if off is None else off[ids != k], None if v is None else v[ids != k])
            res = fam.path_result(list(lam), [], *[[] for _ in fam.path_fields], [])
            for j in range(m):
                sol = _glm_solve(fam, x, f, ProxL1(lam[j] * scale, sx), options, irls, k)
                for name, value in fam.cv_measures.items():
                    held[name][k, j] = value(sol, held_v[k])
                tdev[k, j] = fam.cv_train(sol, n, vk)
                rounds[k, j], conv[k, j] = sol.rounds, sol.converged
                if fam.cv_weight is not None:
                    wts[k] = fam.cv_weight(sol)
                if keep_fold_paths:
                    _glm_keep(fam, res, sol, x, p, fit_intercept, nll=sol.nll * n / vk)
                if after_solve is not None:
                    after_solve(f, k, j)
            if keep_fold_paths:
                fold_paths.append(res)
    finally:
        f._synced = None
        if mode_before == 1:
            check(f._L.cdh_set_gradient_cache(f._h, 1), f._h)
        f.set_folds(None, 0)
    cvm, cvsd, imin, i1se = _cv_select(lam, wts, held[measure])
    if full_path and not owned:
        path = _glm_path_on(fam, f, lam, options, irls, np.inf, standardizeX, fit_intercept)
    dev, *others = held.values()
    return fam.cv_result(lam, sizes, dev, tdev, *others, rounds, conv, measure, cvm, cvsd, imin, float(lam[imin]), i1se,
                         float(lam[i1se]), path, fold_paths)


# ---- the binomial family -------------------------------------------------------------------------------------------------
def logisticLasso_(x, f, g, options=None, irls=None, fold=None):
    """Minimise F(β) = (1/n) Σ [log(1 + e^η_i) - y_i η_i] + λ0 Σ ω_j |β_j| over the CDLogisticLoss f by IRLS, warm-started
    from x (updated in place).  A round is one f.irls_step -- working weights, working response and their residual formed on
    the device from the linear predictor the handle holds, nothing n-sized on the host -- and one coordinateDescent_ of the
    weighted lasso they define, which keeps the residual the step left (cdh_set_reuse_residual for the duration).

    fold=k: every step, the final read-only one included, holds the rows of fold k out (irls_step(fold=k), after
    f.set_folds); the minimised F is then (1/n) Σ over the training rows, and the solution carries the held-out rows'
    held_nll and held_miss at the final β."""
    return _glm_solve(_LOGISTIC, x, f, g, options, irls, fold)


def logisticLasso(X, y, lam, omega=None, options=None, irls=None, fit_intercept=False, *, weights=None):
    """ℓ1-penalised logistic regression (glmnet's family = "binomial"): the minimiser of
    (1/n) Σ [log(1 + e^η_i) - y_i η_i] + λ Σ ω_j |β_j|, η = Xβ (+ b with fit_intercept: a column of ones appended as
    coordinate p + 1 with ω = 0, started at log(ȳ / (1 - ȳ)) and returned apart from x, which has length p).  X may also be
    an existing CDLogisticLoss (y is then ignored; no intercept).  weights: CDLogisticLoss's observation weights (glmnet's weights =; normalised to
    sum to n): F = (1/n) Σ v_i nll_i, the penalty scales not weighted by v; refused when a loss is passed in (they are then its own).  With
    weights the intercept starts at logit(Σvy / Σv)."""
    return _glm_lasso(_LOGISTIC, X, y, lam, omega, options, irls, fit_intercept, None, dict(weights=weights))


def logisticLambdaMax(f, omega=None, fit_intercept=False):
    """The smallest λ at which every penalised coordinate of the logistic lasso is zero: max_j |X_j'(y - p̂)| / (n ω_j) at the
    null model (β = 0; with fit_intercept the last column of f is the column of ones, its coordinate log(ȳ / (1 - ȳ)) and
    left out of the maximum).  One irls_step at the null model and one cdh_xt_r: the step leaves r = (y - p̂) / w, and at
    the null model every row has the same weight w̄ = Σw / n, so X'(y - p̂) = w̄ X'r.  The handle is left at the null model.

    On a loss with observation weights the maximum is that of |X_j'(v∘(y - p̂))| / (n ω_j), the intercept logit(Σvy / Σv), and
    the route poissonLambdaMax's: the stored null weights v_i w̄ differ by row, so the shortcut does not hold -- one applied
    step and cdh_lambda_max (X_j'W r / n), which leaves the handle with the penalty scales of the maximum."""
    if not isinstance(f, CDLogisticLoss):
        raise TypeError("MethodError: logisticLambdaMax takes a CDLogisticLoss")
    p = f.p - (1 if fit_intercept else 0)
    x = SparseIterate(f.p)
    if f._has_weights:
        return _lambda_max_by_step(f, x, p, omega, fit_intercept and _logit_start(f.labels, f.weights), 1e-12)
    if fit_intercept:
        x[p + 1] = _logit_start(f.labels)
    f._push(x, rebuild=True)
    f._synced = None
    wbar = f.irls_step(True, 1e-12)["sum_w"] / f.n
    out = np.zeros(f.p)
    check(f._L.cdh_xt_r(f._h, _vp(out)), f._h)
    t = np.abs(out[:p]) * wbar / f.n
    if omega is not None:
        t = t / np.asarray(omega, dtype=np.float64)[:p]
    return float(t.max())


def _lambda_max_by_step(f, x, p, omega, start, wmin):
    """max_j |X_j'W r| / (n ω_j) after one applied step at the null model (start: the intercept's coordinate, or False): the
    body of poissonLambdaMax, and of logisticLambdaMax on a loss with observation weights."""
    om = None if omega is None else np.asarray(omega, dtype=np.float64)[:p]
    if start is not False:
        x[p + 1] = start
        om = np.r_[np.ones(p) if om is None else om, np.inf]        # (|g| / inf = 0: the intercept is out of the maximum)
    f._push(x, rebuild=True)
    f._synced = None
    f.irls_step(True, wmin)
    f._set_penalty(ProxL1(1.0, om))
    out = C.c_double()
    check(f._L.cdh_lambda_max(f._h, C.byref(out)), f._h)
    return out.value


def LogisticLassoPath(X, y, lambdapath, options=None, irls=None, max_hat_s=np.inf, standardizeX=True, fit_intercept=False, *,
                      weights=None):
    """LassoPath's loop (src/lasso.jl:229-260) with logisticLasso_ per λ: one handle, one x warm-started along λ,
    ω = _stdX!(X) (cdh_col_rms) when standardising, the intercept -- if any -- unpenalised.  βpath[i] has length p.  weights: CDLogisticLoss's observation weights (glmnet's weights =; normalised to
    sum to n): F = (1/n) Σ v_i nll_i, the penalty scales not weighted by v; refused when a loss is passed in (they are then its own)."""
    return _glm_path(_LOGISTIC, X, y, lambdapath, options, irls, max_hat_s, standardizeX, fit_intercept, None,
                     dict(weights=weights))


def cvLogisticLassoPath(X, y, lambdapath, K=10, folds=None, options=None, irls=None, standardizeX=True, fit_intercept=False,
                        seed=0, measure="deviance", full_path=True, keep_fold_paths=False, *, weights=None):
    """K-fold cross-validation of LogisticLassoPath(X, y, λpath, options, irls; standardizeX, fit_intercept) on the device
    (glmnet's cv.glmnet(family = "binomial")); no reference counterpart.  X may also be an existing CDLogisticLoss (y is then
    ignored; no intercept); the design is uploaded once.

    A fold is a 0/1 observation weight, as in cvLassoPath: the logistic lasso on the n_k training rows of fold k has the
    iterates of IRLS on all n rows with the held-out rows at w = 0, z = η (irls_step(fold=k): cdh_glm_irls_fold), ω =
    _stdX!(w, X) of the 0/1 weights and λ·sqrt(n_k / n) (standardizeX=False: ω = 1 and λ·n_k / n).  Per fold the path is
    LogisticLassoPath's loop, warm-started along λ, and the read-only step that ends every solve returns the held-out
    deviance and class error of that λ.  Nothing n-sized moves after the upload.

    folds: 0-based ids, one per row; otherwise np.random.default_rng(seed).permutation(n) % K.  measure: "deviance" or
    "class" -- what cvm, cvsd and the selections are taken from.  There is no max_hat_s: the folds would be truncated at
    different λ.  With fit_intercept every fold starts at the logit of its own training rows' mean label.  The folds are
    dropped when the call returns or raises.  `path` is LogisticLassoPath on all rows (None with full_path=False): from a
    matrix it runs before the folds, on the fresh handle, and is that call's result bit for bit; on a loss that was passed
    in it runs after them, so that the loss comes back with the weights of all rows.  `fold_paths`: the K fold paths as LogisticLassoPathResult (None unless keep_fold_paths).

    weights (or a loss made with them): fold k's problem is the weighted path on its training rows with their weights
    renormalised to sum to n_k.  With V_k = Σ v over the training rows, λ is scaled by (V_k / n) / sqrt(n_k / n)
    (standardizeX=False: V_k / n) -- today's factors when v ≡ 1 -- and ω stays _stdX!(w, X) of the 0/1 weights, not weighted
    by v.  The held-out measures divide by Σ v over the held-out rows, which is also the fold's weight in cvm and cvsd;
    train_deviance divides by V_k; fold_sizes stay row counts."""
    return _cv_glm_path(_LOGISTIC, X, y, lambdapath, K, folds, options, irls, standardizeX, fit_intercept, seed, measure, None,
                        full_path, keep_fold_paths, dict(weights=weights))


# ---- the Poisson family with an offset ----------------------------------------------------------------------------------------
def poissonLasso_(x, f, g, options=None, irls=None, fold=None):
    """Minimise F(β) = (1/n) Σ [μ_i - y_i η_i] + λ0 Σ ω_j |β_j|, η = Xβ + o, μ = e^η, over the CDPoissonLoss f by IRLS,
    warm-started from x (updated in place): logisticLasso_'s loop with f.irls_step of the Poisson family (irls.wmin,
    irls.etaMax).  fold=k: every step holds the rows of fold k out, F is (1/n) Σ over the training rows, and the solution
    carries the held-out rows' held_deviance at the final β."""
    return _glm_solve(_POISSON, x, f, g, options, irls, fold)


def poissonLasso(X, y, lam, omega=None, options=None, irls=None, fit_intercept=False, offset=None, *, weights=None):
    """ℓ1-penalised Poisson regression (glmnet's family = "poisson" with offset): the minimiser of
    (1/n) Σ [μ_i - y_i η_i] + λ Σ ω_j |β_j|, η = Xβ + o (+ b with fit_intercept: a column of ones appended as coordinate
    p + 1 with ω = 0, started at log(Σy / Σ e^o) and returned apart from x, which has length p).  X may also be an existing
    CDPoissonLoss (y and offset are then its own; no intercept).  weights: CDPoissonLoss's observation weights (glmnet's weights =; normalised to
    sum to n): F = (1/n) Σ v_i nll_i, the penalty scales not weighted by v; refused when a loss is passed in (they are then its own).  With
    weights the intercept starts at log(Σvy / Σ v e^o)."""
    return _glm_lasso(_POISSON, X, y, lam, omega, options, irls, fit_intercept, offset, dict(weights=weights))


def poissonLambdaMax(f, omega=None, fit_intercept=False):
    """The smallest λ at which every penalised coordinate of the Poisson lasso is zero: max_j |X_j'(y - μ)| / (n ω_j) at the
    null model (β = 0, μ = e^o; with fit_intercept the last column of f is the column of ones, its coordinate
    log(Σy / Σ e^o) and left out of the maximum).  One applied irls_step at the null model leaves r = (y - μ) / w, and the
    weighted gradient of the handle (cdh_lambda_max: X_j'W r / n) is X_j'(y - μ) / n -- with an offset the null weights differ
    by row, so the binomial's w̄ X'r does not hold here.  Nothing n-sized crosses the host beyond the counts and the offset of
    an intercept's start.  The handle is left at the null model, with the penalty scales of the maximum.  On a loss with
    observation weights the same step leaves X'W r = X'(v∘(y - μ)), and the intercept is log(Σvy / Σ v e^o)."""
    if not isinstance(f, CDPoissonLoss):
        raise TypeError("MethodError: poissonLambdaMax takes a CDPoissonLoss")
    p = f.p - (1 if fit_intercept else 0)
    return _lambda_max_by_step(f, SparseIterate(f.p), p, omega,
                               fit_intercept and _poisson_start(f.counts, f.offset, f._prior()), 1e-300)


def PoissonLassoPath(X, y, lambdapath, options=None, irls=None, max_hat_s=np.inf, standardizeX=True, fit_intercept=False,
                     offset=None, *, weights=None):
    """LassoPath's loop (src/lasso.jl:229-260) with poissonLasso_ per λ: one handle, one x warm-started along λ,
    ω = _stdX!(X) (cdh_col_rms) when standardising, the intercept -- if any -- unpenalised.  βpath[i] has length p.  weights: CDPoissonLoss's observation weights (glmnet's weights =; normalised to
    sum to n): F = (1/n) Σ v_i nll_i, the penalty scales not weighted by v; refused when a loss is passed in (they are then its own)."""
    return _glm_path(_POISSON, X, y, lambdapath, options, irls, max_hat_s, standardizeX, fit_intercept, offset,
                     dict(weights=weights))


def cvPoissonLassoPath(X, y, lambdapath, K=10, folds=None, options=None, irls=None, standardizeX=True, fit_intercept=False,
                       seed=0, measure="deviance", offset=None, full_path=True, keep_fold_paths=False, *, weights=None):
    """K-fold cross-validation of PoissonLassoPath(X, y, λpath, options, irls; standardizeX, fit_intercept, offset) on the
    device (glmnet's cv.glmnet(family = "poisson", offset = ...)); no reference counterpart.  X may also be an existing
    CDPoissonLoss (y and offset are then its own; no intercept); the design is uploaded once.

    cvLogisticLassoPath's structure: a fold is a 0/1 observation weight, the held-out rows kept at w = 0, z = Xβ by
    irls_step(fold=k), ω = _stdX!(w, X) of the 0/1 weights and λ·sqrt(n_k / n) (standardizeX=False: ω = 1 and λ·n_k / n);
    with fit_intercept every fold starts at log(Σy / Σ e^o) of its own training rows.  The read-only step that ends every
    solve returns the held-out Poisson deviance of that λ: the only measure.  Nothing n-sized moves after the upload.

    folds: 0-based ids, one per row; otherwise np.random.default_rng(seed).permutation(n) % K.  There is no max_hat_s.  The
    folds are dropped when the call returns or raises.  `path` is PoissonLassoPath on all rows (None with full_path=False):
    from a matrix it runs before the folds, on the fresh handle, and is that call's result bit for bit; on a loss that was
    passed in it runs after them, so that the loss comes back with the weights of all rows.  `fold_paths`: the K fold paths
    as PoissonLassoPathResult (None unless keep_fold_paths).

    weights (CDPoissonLoss's; or a loss made with them): fold k's problem is the weighted path on its training rows with their weights
    renormalised to sum to n_k.  With V_k = Σ v over the training rows, λ is scaled by (V_k / n) / sqrt(n_k / n)
    (standardizeX=False: V_k / n) -- today's factors when v ≡ 1 -- and ω stays _stdX!(w, X) of the 0/1 weights, not weighted
    by v.  The held-out measures divide by Σ v over the held-out rows, which is also the fold's weight in cvm and cvsd;
    train_deviance divides by V_k; fold_sizes stay row counts."""
    return _cv_glm_path(_POISSON, X, y, lambdapath, K, folds, options, irls, standardizeX, fit_intercept, seed, measure, offset,
                        full_path, keep_fold_paths, dict(weights=weights))


# ---- the Cox family, Breslow ties ------------------------------------------------------------------------------------------
def coxLasso_(x, f, g, options=None, irls=None, fold=None):
    """Minimise F(β) = -(1/n) Σ δ_i (η_i - log S_i) + λ0 Σ ω_j |β_j|, η = Xβ + o, over the CDCoxLoss f by IRLS, warm-started
    from x (updated in place): logisticLasso_'s loop with f.irls_step of the Cox family (irls.wmin, irls.etaMax).  fold=k:
    every step holds the rows of fold k out of the risk sets and the event sums, F is (1/n) Σ over the training rows, and the
    solution carries held_deviance = -2 (ℓ_all - ℓ_train) and held_events at the final β."""
    return _glm_solve(_COX, x, f, g, options, irls, fold)


def coxLasso(X, y, lam, omega=None, options=None, irls=None, offset=None, strata=None, weights=None, ties="breslow"):
    """ℓ1-penalised Cox regression with Breslow ties (glmnet's family = "cox"): the minimiser of
    -(1/n) Σ δ_i (η_i - log S_i) + λ Σ ω_j |β_j|, η = Xβ + o, y = [time, status] (n x 2).  There is no intercept: it cancels
    in the partial likelihood.  y = [start, stop, status] (n x 3): start-stop times, row i at risk over (start_i, stop_i]
    (CDCoxLoss).  strata and weights: CDCoxLoss's (glmnet's stratifySurv and weights =; the weights are
    normalised to sum to n).  ties: "breslow" or "efron" (CDCoxLoss.set_ties; survival::coxph's default is "efron"), refused
    with start-stop times.  X may also be an existing CDCoxLoss (y, offset, strata and weights are then its own, and ties must
    name the loss's own rule)."""
    _cox_ties(ties, X, y)
    if not isinstance(X, CoordinateDifferentiableFunction):
        _survival(y, np.shape(X)[0] if np.ndim(X) == 2 else None)
    return _glm_lasso(_COX, X, y, lam, omega, options, irls, False, offset, dict(strata=strata, weights=weights, ties=ties))


def coxLambdaMax(f, omega=None):
    """The smallest λ at which every coordinate of the Cox lasso is zero: max_j |X_j'(δ - eA)| / (n ω_j) at β = 0.
    poissonLambdaMax's recipe: one applied irls_step at β = 0 leaves r = (δ - eA) / w, and the weighted gradient of the
    handle (cdh_lambda_max: X_j'W r / n) is X_j'(δ - eA) / n whatever the clamp did to w.  On a loss with strata and weights
    the same step leaves X'W r = X'(vδ - v e A), A that of the row's stratum: the gradient of the weighted stratified partial
    likelihood.  The handle is left at β = 0, with the penalty scales of the maximum."""
    if not isinstance(f, CDCoxLoss):
        raise TypeError("MethodError: coxLambdaMax takes a CDCoxLoss")
    x = SparseIterate(f.p)
    om = None if omega is None else np.asarray(omega, dtype=np.float64)[:f.p]
    f._push(x, rebuild=True)
    f._synced = None
    f.irls_step(True, 1e-300)
    f._set_penalty(ProxL1(1.0, om))
    out = C.c_double()
    check(f._L.cdh_lambda_max(f._h, C.byref(out)), f._h)
    return out.value


def coxResiduals(f, type="martingale", eta_max=50.0):
    """residuals(coxph, type) of a fitted CDCoxLoss at the iterate its handle holds: CDCoxLoss.residuals."""
    if not isinstance(f, CDCoxLoss):
        raise TypeError("MethodError: coxResiduals takes a CDCoxLoss")
    return f.residuals(type, eta_max)


def coxBaselineHazard(f, eta_max=50.0):
    """basehaz(fit, centered = FALSE) of a fitted CDCoxLoss at the iterate its handle holds: CDCoxLoss.baseline_hazard,
    uncentred (x = 0, offset 0)."""
    if not isinstance(f, CDCoxLoss):
        raise TypeError("MethodError: coxBaselineHazard takes a CDCoxLoss")
    return f.baseline_hazard(eta_max)


def coxConcordance(f, fold=None):
    """Harrell's concordance index of a fitted CDCoxLoss at the iterate its handle holds (survival::concordance, glmnet's
    Cindex): CDCoxLoss.concordance."""
    if not isinstance(f, CDCoxLoss):
        raise TypeError("MethodError: coxConcordance takes a CDCoxLoss")
    return f.concordance(fold)


def coxScoreResiduals(f, columns=None, weighted=False, eta_max=50.0):
    """residuals(coxph, "score") of a fitted CDCoxLoss at the iterate its handle holds: CDCoxLoss.score_residuals."""
    if not isinstance(f, CDCoxLoss):
        raise TypeError("MethodError: coxScoreResiduals takes a CDCoxLoss")
    return f.score_residuals(columns, weighted, eta_max)


def coxSchoenfeldResiduals(f, columns=None, eta_max=50.0):
    """residuals(coxph, "schoenfeld") of a fitted CDCoxLoss at the iterate its handle holds: CDCoxLoss.schoenfeld_residuals."""
    if not isinstance(f, CDCoxLoss):
        raise TypeError("MethodError: coxSchoenfeldResiduals takes a CDCoxLoss")
    return f.schoenfeld_residuals(columns, eta_max)


def coxInformation(f, columns=None, eta_max=50.0):
    """The information matrix of a fitted CDCoxLoss at the iterate its handle holds, on `columns`: CDCoxLoss.information."""
    if not isinstance(f, CDCoxLoss):
        raise TypeError("MethodError: coxInformation takes a CDCoxLoss")
    return f.information(columns, eta_max)


def coxInferenceFrom(columns, beta, info, score=None, weights=None, cluster=None):
    """CoxInference from the device's answers, in plain numpy: var = info⁻¹, se, z; with `score` (the n x m unweighted score
    residuals) also dfbeta = diag(weights) score var, robust_var = D'D with D = dfbeta summed over the `cluster` ids (None:
    every row its own cluster) and robust_se -- R's coxph(robust = TRUE).  A singular information matrix is refused."""
    cols = np.atleast_1d(np.asarray(columns, dtype=np.int64))
    b = np.atleast_1d(np.asarray(beta, dtype=np.float64))
    I = np.asarray(info, dtype=np.float64)
    m = len(cols)
    if I.shape != (m, m) or b.shape != (m,):
        raise DimensionMismatch("info must be m x m and beta of length m for the m columns")
    if not np.all(np.isfinite(I)) or np.linalg.matrix_rank(I) < m:
        raise ArgumentError("the information matrix is singular on these columns: no variance")
    var = np.linalg.inv(I)
    var = (var + var.T) / 2.0
    if np.any(np.diag(var) <= 0.0):
        raise ArgumentError("the information matrix is singular on these columns: no variance")
    se = np.sqrt(np.diag(var))
    out = CoxInference(cols, b, var, se, b / se)
    if score is not None:
        L = np.asarray(score, dtype=np.float64)
        v = np.ones(L.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
        if L.ndim != 2 or L.shape[1] != m or v.shape != (L.shape[0],):
            raise DimensionMismatch("score must be n x m and weights of length n")
        out.dfbeta = (v[:, None] * L) @ var
        D = out.dfbeta
        if cluster is not None:
            ids = np.asarray(cluster)
            if ids.shape != (L.shape[0],):
                raise DimensionMismatch("cluster must hold one id per row")
            _, inverse = np.unique(ids, return_inverse=True)
            D = np.zeros((inverse.max() + 1, m))
            np.add.at(D, inverse, out.dfbeta)
        out.robust_var = D.T @ D
        out.robust_se = np.sqrt(np.diag(out.robust_var))
    return out


def coxInference(f, columns=None, robust=False, cluster=None, eta_max=50.0):
    """Standard errors of a fitted CDCoxLoss at the iterate its handle holds, on `columns` (1-based; None: the support of β):
    a CoxInference with var = I⁻¹ (coxph's var on those columns, the others held at their values), se and z; robust=True adds
    the sandwich of R's coxph(robust = TRUE): dfbeta, robust_var and robust_se, clustered by `cluster` ids when given.  One
    device call (cdh_glm_cox_score) and plain numpy on its m x m and n x m answers.  After an l1-penalised fit these are the
    usual post-selection quantities: the penalty is not accounted for.  Breslow ties; no start-stop times yet."""
    if not isinstance(f, CDCoxLoss):
        raise TypeError("MethodError: coxInference takes a CDCoxLoss")
    if cluster is not None and not robust:
        raise ArgumentError("cluster needs robust=True")
    if cluster is not None and np.shape(cluster) != (f.n,):
        raise DimensionMismatch("cluster must hold one id per row")
    cols, _, L, I, _ = f._score(columns, eta_max, score=bool(robust), info=True)
    beta = np.zeros(f.p)
    check(f._L.cdh_get_beta(f._h, _vp(beta)), f._h)
    return coxInferenceFrom(cols, beta[cols - 1], I, L, f.weights if robust else None, cluster)


def coxSurvival(baseline, eta_new, times, strata_new=None):
    """Survival curves of new rows (survfit.coxph / glmnet's survfit.coxnet with newx): the m x len(times) array
    exp(-H0_g(t) exp(eta_new)), eta_new = x_new'β + offset of the m new rows and g their strata (strata_new; None: every row
    in the table's only stratum).  H0_g is the right-continuous step function of the CoxBaseline table, which is uncentred
    (x = 0, offset 0): 0 before the stratum's first event time, and its value at an event time includes that time's events.
    Plain numpy on the compact table; a stratum that the table does not hold is refused."""
    eta = np.atleast_1d(np.asarray(eta_new, dtype=np.float64))
    tt = np.atleast_1d(np.asarray(times, dtype=np.float64))
    if eta.ndim != 1 or tt.ndim != 1:
        raise DimensionMismatch("eta_new and times must be vectors")
    ids = np.unique(baseline.stratum)
    if strata_new is None:
        if len(ids) > 1:
            raise ArgumentError("the baseline holds %d strata: strata_new must name the stratum of every new row" % len(ids))
        g = np.full(len(eta), ids[0] if len(ids) else 0, dtype=np.int64)
    else:
        g = np.atleast_1d(np.asarray(strata_new)).astype(np.int64)
        if g.shape != eta.shape:
            raise DimensionMismatch("length(strata_new) != length(eta_new)")
    H = np.zeros((len(eta), len(tt)))
    for s in np.unique(g):
        rows = baseline.stratum == s
        if not rows.any():
            raise ArgumentError("stratum %d is not in the baseline table" % int(s))
        ts, cs = baseline.time[rows], baseline.cumhaz[rows]
        at = np.searchsorted(ts, tt, side="right")              # the event times <= t
        H[g == s] = np.where(at > 0, cs[np.maximum(at - 1, 0)], 0.0)[None, :]
    return np.exp(-H * np.exp(eta)[:, None])


def CoxLassoPath(X, y, lambdapath, options=None, irls=None, max_hat_s=np.inf, standardizeX=True, offset=None, strata=None,
                 weights=None, ties="breslow"):
    """LassoPath's loop (src/lasso.jl:229-260) with coxLasso_ per λ: one handle, one x warm-started along λ,
    ω = _stdX!(X) (cdh_col_rms) when standardising.  βpath[i] has length p.  y may be n x 3, [start, stop, status]
    (CDCoxLoss).  strata and weights: CDCoxLoss's; the penalty
    scales ω stay the root mean square over the rows present, not weighted by the observation weights.  ties: coxLasso's."""
    _cox_ties(ties, X, y)
    if not isinstance(X, CoordinateDifferentiableFunction):
        _survival(y, np.shape(X)[0] if np.ndim(X) == 2 else None)
    return _glm_path(_COX, X, y, lambdapath, options, irls, max_hat_s, standardizeX, False, offset,
                     dict(strata=strata, weights=weights, ties=ties))


def cvCoxLassoPath(X, y, lambdapath, K=10, folds=None, options=None, irls=None, standardizeX=True, seed=0, measure="deviance",
                   offset=None, full_path=True, keep_fold_paths=False, strata=None, weights=None, ties="breslow"):
    """K-fold cross-validation of CoxLassoPath(X, y, λpath, options, irls; standardizeX, offset) on the device (glmnet's
    cv.glmnet(family = "cox", grouped = TRUE)); no reference counterpart.  X may also be an existing CDCoxLoss (y and offset
    are then its own); the design is uploaded once.

    cvLogisticLassoPath's structure: a fold is a 0/1 observation weight, and irls_step(fold=k) takes the held-out rows out
    of the risk sets and the event sums and keeps them at w = 0, z = Xβ.  The Cox lasso on the n_k training rows of fold k
    alone, at λ, has the iterates of that loop at λ·sqrt(n_k / n) with ω = _stdX!(w, X) of the 0/1 weights
    (standardizeX=False: ω = 1 and λ·n_k / n): the loss is (1/n) Σ here and (1/n_k) Σ there.  The read-only steps that end
    every solve give fold_deviance[k, j] = -2 (ℓ_all - ℓ_train) / (held-out events of fold k), the default measure; cvm and cvsd
    weight the folds by those event counts.  A fold without a held-out event, or without a training event, is refused
    before the upload.  Nothing n-sized moves after the upload.

    measure="C" (glmnet's type.measure = "C"): after every solve of fold k the held-out rows' concordance index at that β
    (CDCoxLoss.concordance(fold=k): counted on the device, four doubles come back) goes into fold_concordance[k, j] of a
    CVCoxConcordancePathResult; cvm and cvsd weight the folds by their held-out Σ v (their sizes without weights), index_min
    is the position of the LARGEST cvm and index_1se the largest λ whose cvm is at least that maximum less its cvsd.
    fold_deviance and the rest are filled as under "deviance", whose calls the handle sees unchanged.  A fold whose held-out
    rows hold no comparable pair is refused.  Not offered with start-stop times.

    strata and weights: CDCoxLoss's (refused, like offset, when a loss is passed in: they are then its own).  The folds keep
    the λ scaling above and the unweighted penalty scales; "events" are then Σ v_i δ_i, floats: a fold is weighted by its
    held-out Σ v δ (fold_events), and the refusals apply to those sums.

    Start-stop times (y n x 3, or a CDCoxLoss made with them): a subject may be several rows, and the library does not know
    subjects -- the rows of one subject should share a fold, so pass folds= with one id per subject repeated over its rows;
    the random folds split rows.

    folds: 0-based ids, one per row; otherwise np.random.default_rng(seed).permutation(n) % K.  There is no max_hat_s.  The
    folds are dropped when the call returns or raises.  `path` is CoxLassoPath on all rows (None with full_path=False):
    from a matrix it runs before the folds, on the fresh handle, and is that call's result bit for bit; on a loss that was
    passed in it runs after them.  `fold_paths`: the K fold paths as CoxLassoPathResult (None unless keep_fold_paths).

    ties: coxLasso's.  With "efron" a fold's tie groups count their TRAINING rows only (d, D and m), the held-out deviance is
    2 (ℓ_all - ℓ_train) of Efron's likelihood, and the λ scaling of the folds is the same: all three follow from the step."""
    _cox_ties(ties, X, y)
    if measure not in ("deviance", "C"):
        raise ArgumentError('measure must be "deviance" or "C"')
    if measure == "C" and (X._interval if isinstance(X, CDCoxLoss) else np.ndim(y) == 2 and np.shape(y)[1] == 3):
        raise ArgumentError('measure="C": concordance with start-stop times is not offered yet')     # (before the upload)
    extra = dict(strata=strata, weights=weights, ties=ties)
    v = None
    if isinstance(X, CDCoxLoss):
        _glm_loss(_COX, X, y, False, offset, extra)               # (its refusals of what belongs to the loss)
        status = X.status
        v = X.weights if X._weighted else None
        dv = status * v if X._weighted else None
    elif isinstance(X, CoordinateDifferentiableFunction):
        raise TypeError("MethodError: cvCoxLassoPath takes a matrix or a CDCoxLoss")
    else:
        _, status = _survival(y, np.shape(X)[0] if np.ndim(X) == 2 else None)
        _, v = _strata_weights(strata, weights, len(status))
        dv = None if v is None else status * v
    ids, sizes = _cv_fold_ids(len(status), K, folds, seed)
    count = np.bincount(ids, weights=status, minlength=len(sizes)).astype(np.int64)
    events = count if dv is None else np.bincount(ids, weights=dv, minlength=len(sizes))
    for k in range(len(sizes)):                                   # (v > 0: Σ v δ is zero exactly where the count is)
        if events[k] == 0 or count[k] == 0:
            raise ArgumentError("fold %d holds no event: its held-out deviance is undefined" % k)
        if count[k] == count.sum():
            raise ArgumentError("fold %d holds every event: its training rows have none" % k)
    if measure == "deviance":
        res = _cv_glm_path(_COX, X, y, lambdapath, K, folds, options, irls, standardizeX, False, seed, measure, offset,
                           full_path, keep_fold_paths, extra)
        res.fold_events = events
        return res
    lam = np.array(list(lambdapath), dtype=np.float64)
    conc = np.zeros((len(sizes), lam.size))

    def held_out_c(f, k, j):
        c = f.concordance(fold=k)
        if not c.comparable > 0:
            raise ArgumentError("fold %d holds no comparable pair: its concordance index is undefined" % k)
        conc[k, j] = c.C

    res = _cv_glm_path(_COX, X, y, lam, K, folds, options, irls, standardizeX, False, seed, "deviance", offset,
                       full_path, keep_fold_paths, extra, held_out_c)
    held_v = sizes.astype(np.float64) if v is None else np.bincount(ids, weights=v, minlength=len(sizes))
    cvm, cvsd, _, _ = _cv_select(lam, held_v, conc)
    imax = int(np.argmax(cvm))
    ok = np.nonzero(cvm >= cvm[imax] - cvsd[imax])[0]
    i1se = int(ok[np.argmax(lam[ok])])           # the largest λ within one standard error of the best
    kept = {k: getattr(res, k) for k in CVCoxLassoPathResult.__dataclass_fields__}
    kept.update(measure="C", cvm=cvm, cvsd=cvsd, index_min=imax, lambda_min=float(lam[imax]), index_1se=i1se,
                lambda_1se=float(lam[i1se]), fold_events=events)
    return CVCoxConcordancePathResult(**kept, fold_concordance=conc)


# --------------------------------------------------------------------------------------
# Varying-coefficient lasso (src/varying_coefficient_lasso.jl:30-79)
# --------------------------------------------------------------------------------------
def _vc_refit(f, beta, S):
    """(Xs'W Xs) \\ (Xs'W y) (:73-75) without a second copy of y or anything n-sized on the host: with β supported inside S,
    Xs'Wy = Xs'Wr + (Xs'WXs) β_S, so the solution is β_S + (Xs'WXs)⁻¹ Xs'Wr -- one weighted Gram block at the solve's own
    residual, solved on the host after scaling it to unit diagonal."""
    idx1 = np.ascontiguousarray(np.nonzero(S)[0] + 1, dtype=np.int64)
    m = idx1.shape[0]
    if m > 4096:
        raise ArgumentError("refit support larger than 4096 columns")
    G, c = np.zeros((m, m)), np.zeros(m)
    check(f._L.cdh_gram_weighted(f._h, m, _vp(idx1), _vp(G), _vp(c), None), f._h)
    d = np.sqrt(np.diag(G))
    return beta[idx1 - 1] + np.linalg.solve(G / np.outer(d, d), c / d) / d


def locpolyl1(X, z, y, zgrid, degree, kernel, lambda0, refit, options=None):
    """locpolyl1(X, z, y, zgrid, degree, kernel, λ0, refit, options) (src/varying_coefficient_lasso.jl:30-79) ->
    (out, outR), two dense p (degree + 1) x length(zgrid) arrays (the reference returns them sparse).  β is carried from one
    grid point to the next (the inner options force warmStart, :39-42).  X may also be an existing
    CDVaryingCoefficientLoss (data already resident in HBM); z, y and degree are then the loss's own.  The statistics of
    every solve and the support in SparseIterate order are appended to f.point_stats."""
    o = options or CDOptions()
    opt = CDOptions(o.maxIter, o.optTol, o.randomize, True, o.numSteps, o.seed)
    if isinstance(X, CDVaryingCoefficientLoss):
        f = X
    else:
        X = np.asarray(X)
        if np.asarray(z).shape[0] != X.shape[0]:
            raise DimensionMismatch("length(z) != size(X, 1)")
        if np.asarray(y).shape[0] != X.shape[0]:
            raise DimensionMismatch("length(y) != size(X, 1)")
        f = CDVaryingCoefficientLoss(y, X, z, degree)
    zgrid = np.atleast_1d(np.asarray(zgrid, dtype=np.float64))
    ep = f.p
    out, outR = np.zeros((ep, zgrid.shape[0])), np.zeros((ep, zgrid.shape[0]))
    beta = SparseIterate(ep)
    for ind, z0 in enumerate(zgrid):
        sx = f.set_point(kernel, z0)                                   # :63-65
        coordinateDescent_(beta, f, ProxL1(lambda0, sx), opt)          # :68
        f.point_stats.append(dict(f.last_stats, support=beta.nzval2ind.copy()))
        b = beta.dense()
        out[:, ind] = b
        if refit:                                                      # :71-76
            S = get_nonzero_coordinates(b, f.p_base, f.degree, True)
            if S.any():
                outR[S, ind] = _vc_refit(f, b, S)
    return out, outR


def getSigma(f):
    """_getSigma(w, f.r) (src/utils.jl:167-175): sqrt(Σ w r² / Σ w) at the residual the handle stands for; both sums are
    taken on the device (cdh_resid_wmoments)."""
    sw, swr2 = C.c_double(), C.c_double()
    check(f._L.cdh_resid_wmoments(f._h, C.byref(sw), C.byref(swr2)), f._h)
    return float(np.sqrt(swr2.value / sw.value))


def findInitResiduals_(f, scores, s):
    """_findInitResiduals!(w, X, y, s, f.r) (src/utils.jl:79-92) given the scores |X_j'Wy| of _findLargestCorrelations
    (:108-124): S = the columns whose score is at least the s-th largest (ties kept), and f.r = y - X_S (X_S'WX_S) \\ (X_S'Wy),
    formed on the device -- the weighted normal equations from one Gram block at r = y, solved on the host as
    solve_screening_ols solves them, the residual by initialize!.  The handle's iterate is the fit afterwards (nobody's x).
    Returns the 1-based columns of S."""
    L = f._L
    scores = np.asarray(scores, dtype=np.float64)
    S = np.nonzero(scores >= np.sort(scores)[::-1][s - 1])[0]
    if len(S) > 4096:
        raise ArgumentError("screening set larger than 4096 columns")
    idx1 = np.ascontiguousarray(S + 1, dtype=np.int64)
    m = len(S)
    check(L.cdh_initialize(f._h, f.p, 0, None, None), f._h)            # beta = 0, r = y: X_S'Wr == X_S'Wy
    f._synced = None
    G, c = np.zeros((m, m)), np.zeros(m)
    check(L.cdh_gram_weighted(f._h, m, _vp(idx1), _vp(G), _vp(c), None), f._h)

    def normal_residual(b):                  # Xs'W(y - Xs b)
        check(L.cdh_initialize(f._h, f.p, m, _vp(idx1), _vp(np.ascontiguousarray(b))), f._h)
        out = np.zeros(m)
        check(L.cdh_xt_r_cols(f._h, m, _vp(idx1), _vp(out)), f._h)
        return out

    coef = solve_screening_ols(G, c, normal_residual)
    check(L.cdh_initialize(f._h, f.p, m, _vp(idx1), _vp(np.ascontiguousarray(coef))), f._h)
    return idx1


def _lvocv_point(f, beta, row, sx, scores, lambda0, opt, y_row, p_base, degree):
    """One point of lvocv_locpolyl1 (:114-133) on a loss whose weights, design and y are those of the point that left `row`
    out, given its stdX and screening scores: the screening σ, the σ loop, the refit and the prediction -> the point's record
    (lvocv_locpolyl1 lists its fields)."""
    Q1 = degree + 1
    findInitResiduals_(f, scores, min(10, f.p))                                      # :114
    sigma = getSigma(f)                                                              # :117
    sigmas, solves = [sigma], []
    for _ in range(10):                                                              # :119-127
        coordinateDescent_(beta, f, ProxL1(lambda0 * sigma, sx), opt)
        solves.append(f.last_stats)
        sigmanew = getSigma(f)
        sigmas.append(sigmanew)
        if abs(sigmanew - sigma) / sigma < 1e-2:
            break
        sigma = sigmanew
    b = beta.dense()
    S = get_nonzero_coordinates(b, p_base, degree, True)                             # :130
    coef, yhat = None, 0.0
    if S.any():                                                                      # :131-132
        coef = _vc_refit(f, b, S)
        base = np.ascontiguousarray(np.nonzero(S)[0][::Q1] + 1, dtype=np.int64)      # the power-0 column of every group in S
        xrow = np.zeros(base.shape[0])
        check(f._L.cdh_get_X_row(f._h, int(row), base.shape[0], _vp(base), _vp(xrow)), f._h)
        yhat = float(xrow @ coef[::Q1])
    return {"row": int(row), "sigma_iters": len(solves), "sigmas": sigmas, "sigma": sigma, "solves": solves,
            "support": beta.nzval2ind.copy(), "beta": b, "refit": coef, "yhat": yhat, "sq_err": (yhat - y_row) ** 2}


def lvocv_locpolyl1(X, z, y, degree, hArr, kernelType, lambda0, options=None):
    """lvocv_locpolyl1(X, z, y, degree, hArr, kernelType, λ0, options) (src/varying_coefficient_lasso.jl:82-137) -> MSE, a
    float64 array of length(hArr): for every bandwidth the sum over the observations i of (Yh_i - y_i)², Yh_i the refitted
    prediction at z0 = z[i] of the scaled lasso that left observation i out.  Per point: the leave-one-out setup and the
    screening scores in one pass on the device (set_point_leave_out), the weighted screening init for the first σ
    (findInitResiduals_, getSigma), at most ten warm-started solves with σ re-estimated after each (:119-127; the warm start
    rebuilds r = y - Xβ, so the screening residual feeds the first σ only), the refit on the support's groups (_vc_refit)
    and the prediction from the base row: at z0 = z[i] the expanded row i is X[i, j] at power 0 and exactly 0 above it.
    β is one iterate carried over all points and all bandwidths, as in the reference.

    An empty support -- which the reference never handles: its `\\` of a 0 x 0 system gives an empty vector and `dot` over
    an empty selection 0 -- predicts Yh = 0 here as well.

    X may also be an existing CDVaryingCoefficientLoss (z, y and degree are then the loss's own); a loss built here from
    arrays is closed before returning.  One record per point is appended to the caller's f.point_stats: h, row, sigma_iters (solves run), sigmas (the screening σ, then σnew after every solve), sigma
    (the σ of the last penalty), solves (the statistics of every solve), support (SparseIterate order), beta (dense), refit
    (the coefficients on the support's groups, None when it is empty), yhat, sq_err ((Yh - y[row])²)."""
    o = options or CDOptions()
    opt = CDOptions(o.maxIter, o.optTol, o.randomize, True, o.numSteps, o.seed)          # :94
    hArr = np.atleast_1d(np.asarray(hArr, dtype=np.float64))
    kernels = [createKernel(kernelType, h) for h in hArr]                                # :106
    if isinstance(X, CDVaryingCoefficientLoss):
        f = X
    else:
        X = np.asarray(X)
        if np.asarray(z).shape[0] != X.shape[0]:
            raise DimensionMismatch("length(z) != size(X, 1)")
        if np.asarray(y).shape[0] != X.shape[0]:
            raise DimensionMismatch("length(y) != size(X, 1)")
        f = CDVaryingCoefficientLoss(y, X, z, degree)
    try:
        yv = f.y.astype(np.float64)
        MSE = np.zeros(hArr.shape[0])
        beta = SparseIterate(f.p)
        for indH, kernel in enumerate(kernels):
            for i in range(f.n):
                sx, scores = f.set_point_leave_out(kernel, i)                            # :109-113
                rec = _lvocv_point(f, beta, i, sx, scores, lambda0, opt, yv[i], f.p_base, f.degree)
                MSE[indH] += rec["sq_err"]                                               # :133
                if f is X:                 # a caller's loss keeps the records; one built here is gone when this returns
                    f.point_stats.append(dict(rec, h=kernel.h))
    finally:
        if f is not X:
            f.close()
    return MSE


# --------------------------------------------------------------------------------------
# Local polynomial regression in low dimensions (src/varying_coefficient_lasso.jl:197-476)
# --------------------------------------------------------------------------------------
def _solve_scaled(G, c):
    """G \\ c from the symmetrically scaled normal equations (unit diagonal), as _vc_refit solves its block."""
    d = np.sqrt(np.diag(G))
    return np.linalg.solve(G / np.outer(d, d), c / d) / d


def _inv_scaled(G):
    d = np.sqrt(np.diag(G))
    return np.linalg.inv(G / np.outer(d, d)) / np.outer(d, d)


def _check_kernel(kernel):
    if not isinstance(kernel, SmoothingKernel) or kernel._kind is None:
        raise TypeError("MethodError: kernel::SmoothingKernel")
    return kernel


def _kernel_kind(kernel):
    """The cdh_vc_kernel code of a kernel type, of a kernel, or the code itself."""
    if isinstance(kernel, type) and issubclass(kernel, SmoothingKernel) and kernel._kind is not None:
        return int(kernel._kind)
    if isinstance(kernel, SmoothingKernel) and kernel._kind is not None:
        return int(kernel._kind)
    if isinstance(kernel, (int, np.integer)) and not isinstance(kernel, bool):
        return int(kernel)
    raise TypeError("MethodError: kernel::Type{<:SmoothingKernel}")


def _solve_scaled_stack(G, c):
    """_solve_scaled of every block of G[m, ep, ep], c[m, ep]: the same scaling to unit diagonal per point, one stacked solve."""
    d = np.sqrt(np.diagonal(G, axis1=1, axis2=2))
    return np.linalg.solve(G / (d[:, :, None] * d[:, None, :]), (c / d)[:, :, None])[:, :, 0] / d


_LOCPOLY_BATCH = 4096          # points per cdh_vc_gram_batch call of the front ends: 4096 blocks of ep x ep stay modest on the host


def _locpoly_batch(f, kind, h, z0, leave_out):
    """The local polynomial fits around m points -> (m, ep): cdh_vc_gram_batch in pieces of _LOCPOLY_BATCH points, each
    followed by the stacked solve of its scaled normal equations.  h, z0 (or None) and leave_out (or None) are m-vectors."""
    m = h.shape[0]
    out = np.zeros((m, f.p))
    for s in range(0, m, _LOCPOLY_BATCH):
        t = slice(s, min(m, s + _LOCPOLY_BATCH))
        G, c, _ = f.expanded_gram_batch(kind, h[t], None if z0 is None else z0[t],
                                        leave_out=None if leave_out is None else leave_out[t])
        out[t] = _solve_scaled_stack(G, c)
    return out


def _locpoly_loss(X, z, y, degree):
    """-> (loss, built here): X is either a resident CDVaryingCoefficientLoss (z, y and degree are then its own) or the
    reference's X::Matrix{T}, z::Vector{T}, y::Vector{T}; y may be None where the reference takes none."""
    if isinstance(X, CDVaryingCoefficientLoss):
        return X, False
    X, z = np.asarray(X), np.asarray(z)
    if X.ndim != 2 or X.dtype not in (np.float64, np.float32) or z.ndim != 1 or z.dtype != X.dtype:
        raise TypeError("MethodError: X::Matrix{T}, z::Vector{T}, y::Vector{T}, T<:AbstractFloat")
    y = np.zeros(X.shape[0], dtype=X.dtype) if y is None else np.asarray(y)
    if y.ndim != 1 or y.dtype != X.dtype:
        raise TypeError("MethodError: X::Matrix{T}, z::Vector{T}, y::Vector{T}, T<:AbstractFloat")
    if z.shape[0] != X.shape[0]:
        raise DimensionMismatch("length(z) != size(X, 1)")
    if y.shape[0] != X.shape[0]:
        raise DimensionMismatch("length(y) != size(X, 1)")
    if not isinstance(degree, (int, np.integer)) or isinstance(degree, bool):
        raise TypeError("MethodError: degree::Int64")
    if X.shape[1] > _lib.CDH_VC_GRAM_MAX_COLS:
        raise ArgumentError("locpoly on the device takes at most 64 base columns per call")
    return CDVaryingCoefficientLoss(y, X, z, degree), True


def locpoly(X, z, y, z0, degree, kernel=None):
    """locpoly(X, z, y, z0, degree, kernel) and locpoly(X, z, y, zgrid, degree, kernel) (src/varying_coefficient_lasso.jl:
    212-235; kernel defaults to GaussianKernel(1)): the local polynomial fit around a point -> p (degree + 1) coefficients,
    or around every point of a grid -> a p (degree + 1) x length(zgrid) array.  The reference solves each point by QR of
    √w · expandX (:206-209); here the weighted normal equations come from one pass over the base design on the device
    (cdh_vc_gram) and are solved on the host after scaling them to unit diagonal -- the route of the reference's own
    commented-out locpoly_alt (:322-344), which squares the condition number.  A grid is one batch of points
    (cdh_vc_gram_batch) and one stacked solve; its columns equal the single-point results bit for bit.  At most 64 base
    columns.  X may be a resident CDVaryingCoefficientLoss; z, y and degree are then its own."""
    kernel = GaussianKernel(1.0) if kernel is None else _check_kernel(kernel)
    f, owned = _locpoly_loss(X, z, y, degree)
    try:
        if np.ndim(z0) == 0:
            G, c, _ = f.expanded_gram(kernel, z0)
            return _solve_scaled(G, c)
        zgrid = np.asarray(z0, dtype=np.float64)
        if zgrid.ndim != 1:
            raise TypeError("MethodError: zgrid::Vector{T}")
        if zgrid.shape[0] == 0:
            return np.zeros((f.p, 0))
        return np.ascontiguousarray(_locpoly_batch(f, kernel._kind, np.full(zgrid.shape[0], kernel.h), zgrid, None).T)
    finally:
        if owned:
            f.close()


def lvocv_locpoly(X, z, y, degree, hArr, kernelType):
    """lvocv_locpoly(X, z, y, degree, hArr, kernelType) (src/varying_coefficient_lasso.jl:348-380) -> MSE per bandwidth: the
    sum over the observations i of (Yh_i - y_i)², Yh_i the prediction at z0 = z[i] of the local polynomial fit that left
    observation i out.  The reference deletes row i; here it gets weight zero in the device's pass (its own commented-out
    formulation, :413-444).  The points are all (bandwidth, observation) pairs, sent to the device in batches
    (cdh_vc_gram_batch) and solved stacked; the predictions come from the base columns, fetched once (the caller's X, or
    columns j (degree + 1) of a resident loss), and the MSE of a bandwidth is accumulated over its observations in index order."""
    hArr = np.atleast_1d(np.asarray(hArr, dtype=np.float64))
    kernels = [createKernel(kernelType, h) for h in hArr]
    f, owned = _locpoly_loss(X, z, y, degree)
    try:
        Q1, n = f.degree + 1, f.n
        yv = f.y.astype(np.float64)
        if owned:
            Xb = np.asarray(X, dtype=np.float64)
        else:
            Xb = np.concatenate([f.X_cols(j * Q1, 1) for j in range(f.p_base)], axis=1).astype(np.float64)
        MSE = np.zeros(hArr.shape[0])
        if not kernels or n == 0:
            return MSE
        pair = np.arange(len(kernels) * n)
        indH, obs = pair // n, pair % n
        hbeta = _locpoly_batch(f, kernels[0]._kind, hArr[indH], None, obs)
        sq = (np.einsum("ij,ij->i", Xb[obs], hbeta[:, ::Q1]) - yv[obs]) ** 2
        for k, v in zip(indH.tolist(), sq.tolist()):
            MSE[k] += v
        return MSE
    finally:
        if owned:
            f.close()


def get_beta_(out, zgrid, beta_grid, z0):
    """get_beta!(out, zgrid, beta_grid, z0) (src/varying_coefficient_lasso.jl:454-476): the coefficients at z0 from the two
    closest grid points, with the reference's weights exactly as written -- α = (z0 - z1) / (z2 - z1) multiplies the LEFT
    point's column, 1 - α the right one's.  z0 outside the grid indexes out of bounds, as in the reference."""
    zgrid = np.asarray(zgrid)
    id1 = int(np.searchsorted(zgrid, z0, side="right"))          # searchsortedlast, 1-based
    id2 = int(np.searchsorted(zgrid, z0, side="left")) + 1       # searchsortedfirst, 1-based
    if id1 < 1 or id2 > zgrid.shape[0]:
        raise IndexError("BoundsError: z0 lies outside zgrid")
    if id1 == id2:
        out[:] = beta_grid[:, id1 - 1]
    else:
        alpha = (z0 - zgrid[id1 - 1]) / (zgrid[id2 - 1] - zgrid[id1 - 1])
        out[:] = alpha * beta_grid[:, id1 - 1] + (1 - alpha) * beta_grid[:, id2 - 1]
    return out


def split_locpoly(X, z, y, Xtest, ztest, ytest, zgrid, degree, hArr, kernelType):
    """split_locpoly(X, z, y, Xtest, ztest, ytest, zgrid, degree, hArr, kernelType) (src/varying_coefficient_lasso.jl:383-409)
    -> MSE per bandwidth of the grid fit's interpolated predictions (get_beta!) on the test split.  As written in the
    reference, the loop over the test observations runs to size(X, 1), the TRAINING row count."""
    hArr = np.atleast_1d(np.asarray(hArr, dtype=np.float64))
    kernels = [createKernel(kernelType, h) for h in hArr]
    Xtest, ztest, ytest = np.asarray(Xtest), np.asarray(ztest), np.asarray(ytest)
    f, owned = _locpoly_loss(X, z, y, degree)
    try:
        Q1 = f.degree + 1
        MSE = np.zeros(hArr.shape[0])
        bi = np.zeros(f.p)
        for indH, kernel in enumerate(kernels):
            bhat = locpoly(f, None, None, zgrid, f.degree, kernel)
            for i in range(f.n):                                  # :400, n = size(X, 1)
                get_beta_(bi, zgrid, bhat, ztest[i])
                MSE[indH] += (float(ytest[i]) - float(Xtest[i, :] @ bi[::Q1])) ** 2
        return MSE
    finally:
        if owned:
            f.close()


def getResiduals_(ehat, X, z, y, zgrid, betahat, degree, kernel=None):
    """getResiduals!(ϵhat, X, z, y, zgrid, βhat, degree, kernel) (src/varying_coefficient_lasso.jl:237-255): ϵhat[i] =
    y[i] - X[i, :] · β(z[i])[1:(degree+1):ep], β(z[i]) interpolated by get_beta!.  Host numpy, n p work."""
    X, z, y = np.asarray(X), np.asarray(z), np.asarray(y)
    n, p = X.shape
    if z.shape[0] != n or y.shape[0] != n or ehat.shape[0] != n:
        raise DimensionMismatch("ϵhat, z and y need size(X, 1) entries")
    betahat = np.asarray(betahat)
    if betahat.shape[0] != p * (degree + 1):
        raise DimensionMismatch("size(βhat, 1) != p * (degree + 1)")
    bi = np.zeros(p * (degree + 1))
    for i in range(n):
        get_beta_(bi, zgrid, betahat, z[i])
        ehat[i] = y[i] - X[i, :] @ bi[::degree + 1]
    return ehat


def _sandwich(f, z0, kernel, e):
    """diag of A · (X'W Ψ W X) · A at the power-0 coefficients, A = inv(X'WX) (:272-283, :303-314); the products on the host."""
    XtwX, _, _ = f.expanded_gram(kernel, z0, rhs=False)
    XtwwX, _, _ = f.expanded_gram(kernel, z0, wpow=2, e=e, rhs=False)
    A = _inv_scaled(XtwX)
    return np.diag(A @ XtwwX @ A)[::f.degree + 1].copy()


def getStandardError(X, z, sigma2, z0, degree, kernel):
    """getStandardError(X, z, σ2, z0, degree, kernel) (src/varying_coefficient_lasso.jl:257-286) -> for every base column the
    diagonal entry of inv(X'WX) · X'W²X · inv(X'WX) at its power-0 coefficient.  σ2 is accepted and, as in the reference,
    not used.  Both Gram matrices come from the device (wpow 1 and 2)."""
    _check_kernel(kernel)
    f, owned = _locpoly_loss(X, z, None, degree)
    try:
        return _sandwich(f, z0, kernel, None)
    finally:
        if owned:
            f.close()


def getStandardErrorHEW(X, z, eps_sqr, z0, degree, kernel):
    """getStandardErrorHEW(X, z, ϵ_sqr, z0, degree, kernel) (src/varying_coefficient_lasso.jl:288-317): the same with
    X'W Ψ W X, Ψ = diag(ϵ_sqr), in the middle (wpow 2 and e = ϵ_sqr)."""
    _check_kernel(kernel)
    f, owned = _locpoly_loss(X, z, None, degree)
    try:
        eps_sqr = np.asarray(eps_sqr)
        if eps_sqr.shape != (f.n,):
            raise DimensionMismatch("length(ϵ_sqr) != size(X, 1)")
        return _sandwich(f, z0, kernel, eps_sqr)
    finally:
        if owned:
            f.close()


def refit_locpolyl1(X, z, y, z0, degree, kernel, beta):
    """refit_locpolyl1(X, z, y, z0, degree, kernel, β) (src/varying_coefficient_lasso.jl:139-154) -> (βr, S): S the base
    columns whose group of β holds a non-zero (get_nonzero_coordinates(β, p, degree, false)), βr = locpoly(X[:, S], ...)."""
    _check_kernel(kernel)
    f, owned = _locpoly_loss(X, z, y, degree)
    try:
        S = get_nonzero_coordinates(beta, f.p_base, f.degree, False)
        if not S.any():
            return np.zeros(0), S
        if int(S.sum()) > _lib.CDH_VC_GRAM_MAX_COLS:
            raise ArgumentError("refit support larger than 64 base columns")
        G, c, _ = f.expanded_gram(kernel, z0, base_cols=S)
        return _solve_scaled(G, c), S
    finally:
        if owned:
            f.close()
