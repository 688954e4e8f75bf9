"""coordinatedescent.jl_amd -- MI355X-native coordinate-descent sweep behind
CoordinateDescent.jl's operator interface.

The directory name contains a dot, so import it through the root-level shim:
``import coordinatedescent_jl_amd as cd``.

  csrc/        hand-written HIP kernels for gfx950 + the C-ABI (include/cdhip.h)
  _lib.py      ctypes binding + in-tree hipcc build
  api.py       host-side mirror of the reference's interface for this path
  sharded.py   row-sharded multi-process driver (torch.distributed + RCCL)
"""
from . import _lib
from ._lib import build, declared_symbols, needs_build, SO_PATH, CDH_QUAD_MAX_P, CDH_VC_GRAM_MAX_COLS, CDH_VC_GRAM_MAX_POINTS  # noqa: F401
from .api import *  # noqa: F401,F403
from .api import (CDOptions, IterLassoOptions, ProxL1, SparseIterate, CDLeastSquaresLoss,  # noqa: F401
                  CDSqrtLassoLoss, CDWeightedLSLoss, CDQuadraticLoss, CoordinateDifferentiableFunction,
                  OrderedIterator, RandomIterator, reset_, numCoordinates, initialize_, gradient,
                  descendCoordinate_, coordinateDescent_, cdPass_, findLambdaMax, stdX, objective,
                  lasso, sqrtLasso, scaledLasso_, LassoPath, LassoSolution, LassoPathResult,
                  getLoadings, feasibleLasso_, refitLassoPath, cvLassoPath, CVLassoPathResult,
                  CDLogisticLoss, IRLSOptions, logisticLasso_, logisticLasso, logisticLambdaMax, LogisticLassoPath,
                  LogisticLassoSolution, LogisticLassoPathResult, cvLogisticLassoPath, CVLogisticLassoPathResult,
                  CDPoissonLoss, poissonLasso_, poissonLasso, poissonLambdaMax, PoissonLassoPath, PoissonLassoSolution,
                  PoissonLassoPathResult, cvPoissonLassoPath, CVPoissonLassoPathResult,
                  CDCoxLoss, coxLasso_, coxLasso, coxLambdaMax, CoxLassoPath, CoxLassoSolution,
                  CoxLassoPathResult, cvCoxLassoPath, CVCoxLassoPathResult,
                  CoxBaseline, coxResiduals, coxBaselineHazard, coxSurvival,
                  CoxConcordance, coxConcordance, CVCoxConcordancePathResult,
                  CoxSchoenfeld, CoxInference, coxScoreResiduals, coxSchoenfeldResiduals, coxInformation, coxInference,
                  coxInferenceFrom,
                  SmoothingKernel, GaussianKernel, EpanechnikovKernel, createKernel, evaluate,
                  get_nonzero_coordinates, CDVaryingCoefficientLoss, locpolyl1, lvocv_locpolyl1,
                  getSigma, findInitResiduals_,
                  locpoly, lvocv_locpoly, split_locpoly, refit_locpolyl1, getStandardError, getStandardErrorHEW,
                  get_beta_, getResiduals_,
                  DimensionMismatch, ArgumentError, DomainError, HipError)
