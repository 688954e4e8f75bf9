# CoordinateDescentHIP.jl -- the binding a CoordinateDescent.jl maintainer would add to route the
# coordinate-descent path through libcdhip.so (include/cdhip.h) for a design matrix that lives in HBM.
#
# NOT EXECUTED in this repository's pipeline: there is no `julia` in the build image or on the GPU
# box.  It is deliberately a thin ccall shim with no arithmetic beyond an s x s solve: every number
# comes from the library.  tests/test_binding_call_sequence.py replays, with plain ctypes and nothing
# else in between, the exact sequence of C calls each method below makes (function by function) and
# checks the results against the oracle -- that is the executable evidence for this file.  (feasibleLasso! and
# refitLassoPath are replayed the same way in tests/test_binding_feasible_sequence.py.)
#
# lasso(), sqrtLasso(), scaledLasso!, feasibleLasso!, LassoPath, refitLassoPath, CDOptions, IterLassoOptions, ProxL1, SparseIterate and
# the loss constructors are untouched: the user passes a HipMatrix where a Matrix went, and multiple
# dispatch picks the methods below (each strictly more specific than the reference's generic one).
#
#   front-end (src/lasso.jl)              methods of this file it ends up in
#   lasso(X, y, λ[, ω])        :26-53     coordinateDescent!
#   sqrtLasso(X, y, λ, ω)      :84-98     coordinateDescent!      (standardizeX=true is dead code in the
#   sqrtLasso(...; standardizeX=false)                             reference itself: `Array{T}(p)`, :73)
#   scaledLasso!(x, X, y, λ, ω) :107-144  scaledLasso!(x, X::HipMatrix, ...) below: same loop, σ from the device
#                                         (cdh_resid_moments), the residual copied back ONCE at the end
#   LassoPath(X, Y, λpath)     :229-260   LassoPath(X::HipMatrix, ...) below: same loop, nothing n-sized moves
#                                         between the λ (carried residual reused, gradient cache from the start)
#   feasibleLasso!(x, X, y, λ0) :154-194  feasibleLasso!(x, X::HipMatrix, ...) below: the loop the reference intends, the
#                                         loadings of every round from one pass over X on the device (cdh_loadings)
#   refitLassoPath(path, X, Y) :208-225   refitLassoPath(path, X::HipMatrix, Y) below: X[:, S] \ Y per distinct support
#                                         from the s x s normal equations (cdh_gram), as the screening init solves them
# The generic front-ends still work on a HipMatrix through the operator methods (_findInitResiduals!,
# initialize!, coordinateDescent!, _stdX!), at the price of one n-sized device -> host copy per solve because
# their bodies read `f.r` on the host (lasso.jl:134); the two methods above exist to take that copy out of
# the σ loop and the λ loop.
module CoordinateDescentHIP

using CoordinateDescent, ProximalBase
using LinearAlgebra: Symmetric, eigen, dot
using SparseArrays: nnz
using DataStructures: nlargest
import CoordinateDescent: coordinateDescent!, initialize!, gradient, descendCoordinate!,
                          numCoordinates, CDOptions, CDLeastSquaresLoss, CDSqrtLassoLoss, CDWeightedLSLoss,
                          _stdX!, _findInitResiduals!, _findLargestCorrelations,
                          scaledLasso!, feasibleLasso!, LassoPath, refitLassoPath, LassoSolution, IterLassoOptions

const libcdhip = get(ENV, "LIBCDHIP", "libcdhip.so")

const CDH_OK, CDH_DIM_MISMATCH, CDH_BAD_ARG, CDH_DOMAIN = Int32(0), Int32(1), Int32(2), Int32(3)
const CDH_LS, CDH_SQRT, CDH_WLS = Int32(0), Int32(1), Int32(2)

struct CdhOptions            # cdh_options: CDOptions field for field (src/utils.jl:7-13) + seed
  maxIter::Int64
  optTol::Float64
  randomize::Int32
  warmStart::Int32
  numSteps::Int64
  seed::UInt64
end
CdhOptions(o::CDOptions) = CdhOptions(o.maxIter, o.optTol, o.randomize, o.warmStart, o.numSteps, rand(UInt64))

mutable struct CdhStats
  passes::Int64; full_passes::Int64; visits::Int64
  converged::Int32; domain_error::Int32; maxH::Float64; lambda_max::Float64
  CdhStats() = new(0, 0, 0, 0, 0, 0.0, 0.0)
end

function check(h::Ptr{Cvoid}, st::Int32)
  st == CDH_OK && return
  msg = unsafe_string(ccall((:cdh_last_error, libcdhip), Cstring, (Ptr{Cvoid},), h))
  st == CDH_DIM_MISMATCH && throw(DimensionMismatch(msg))
  st == CDH_BAD_ARG && throw(ArgumentError(msg))
  st == CDH_DOMAIN && throw(DomainError(NaN, msg))
  error("cdhip status $st: $msg")
end

# A matrix whose columns live in HBM behind a cdh handle.  <: DenseMatrix so it satisfies
# lasso(X::StridedMatrix{T}, ...) (src/lasso.jl:27); getindex is for display only.  The handle also
# holds y, r (and w) of whichever loss object used it last: `owner` IS that loss's residual vector
# (`f.r`, a fresh `copy(y)` per loss object, cd_differentiable_function.jl:54), held by reference and
# compared with `===`, so every method below can tell whether the device-side y / loss kind are still
# its own.  (A strong reference, not an objectid: the id of a Vector is its address, and the next
# `copy(y)` of the same length can land on the address of a collected one -- the handle would then
# solve against the previous y.  Holding the vector keeps it alive and unaliased; the cost is n
# elements of host memory per matrix until the next loss binds.)
mutable struct HipMatrix{T<:Union{Float32,Float64}} <: DenseMatrix{T}
  handle::Ptr{Cvoid}
  n::Int
  p::Int
  owner::Any
  # the iterate the handle holds, as last pushed to or pulled from it (support in slot order, values): an x that still
  # equals it is not pushed again -- cdh_set_iterate would declare the carried residual stale for nothing, and a
  # user-written pass over descendCoordinate! would upload p numbers per visit
  synced_idx::Vector{Int64}
  synced_val::Vector{Float64}
  synced::Bool
end
Base.size(X::HipMatrix) = (X.n, X.p)
Base.getindex(X::HipMatrix{T}, i::Int, j::Int) where {T} = begin
  col = Vector{T}(undef, X.n)
  check(X.handle, ccall((:cdh_get_X_cols, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64),
                        X.handle, j - 1, 1, col, X.n))
  col[i]
end

dtype_code(::Type{Float64}) = Int32(0)
dtype_code(::Type{Float32}) = Int32(1)

"Upload a host matrix once; every later lasso / sqrtLasso / scaledLasso! / LassoPath call on it runs in HBM."
function HipMatrix(X::StridedMatrix{T}; device::Integer=0) where {T}
  n, p = size(X)
  ref = Ref{Ptr{Cvoid}}(C_NULL)
  check(C_NULL, ccall((:cdh_create, libcdhip), Int32,
                      (Ref{Ptr{Cvoid}}, Int32, Int32, Int64, Int64, Int64, Int64, Int32),
                      ref, dtype_code(T), CDH_LS, n, n, 0, p, device))
  h = ref[]
  GC.@preserve X check(h, ccall((:cdh_set_X_cols, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64),
                                h, 0, p, X, stride(X, 2)))
  M = HipMatrix{T}(h, n, p, nothing, Int64[], Float64[], false)
  finalizer(m -> ccall((:cdh_destroy, libcdhip), Int32, (Ptr{Cvoid},), m.handle), M)
  M
end

const HipLS{T}   = CDLeastSquaresLoss{T,<:Any,<:HipMatrix{T}}
const HipSqrt{T} = CDSqrtLassoLoss{T,<:Any,<:HipMatrix{T}}
const HipWLS{T}  = CDWeightedLSLoss{T,<:Any,<:HipMatrix{T}}
const HipLoss{T} = Union{HipLS{T},HipSqrt{T},HipWLS{T}}

loss_kind(::HipLS) = CDH_LS
loss_kind(::HipSqrt) = CDH_SQRT
loss_kind(::HipWLS) = CDH_WLS

set_loss!(X::HipMatrix, kind::Int32) =
  check(X.handle, ccall((:cdh_set_loss, libcdhip), Int32, (Ptr{Cvoid}, Int32), X.handle, kind))

function upload_y!(X::HipMatrix{T}, y::AbstractVector{T}) where {T}
  length(y) == X.n || throw(DimensionMismatch())
  yy = y isa Vector{T} ? y : Vector{T}(y)            # contiguous host copy of a view / range
  GC.@preserve yy check(X.handle, ccall((:cdh_set_y, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), X.handle, yy))
end

function upload_w!(X::HipMatrix{T}, w::AbstractVector{T}) where {T}
  length(w) == X.n || throw(DimensionMismatch())
  ww = w isa Vector{T} ? w : Vector{T}(w)
  GC.@preserve ww check(X.handle, ccall((:cdh_set_obs_weights, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), X.handle, ww))
end

"Make the handle serve THIS loss object: its kind (the Julia type decides, never a flag given at upload
time), its y (and w).  A loss object is bound when first used and re-bound whenever another loss used
the same HipMatrix in between -- `lasso(Xh, y2, λ)` after `lasso(Xh, y1, λ)` solves against y2, and a
CDSqrtLassoLoss never runs the least-squares update.  (y mutated in place under a live loss object is
the one thing this cannot see: call `rebind!(f)`.)"
function bind!(f::HipLoss{T}) where {T}
  X = f.X
  X.owner === f.r && return f
  rebind!(f)
end
function rebind!(f::HipLoss{T}) where {T}
  X = f.X
  set_loss!(X, loss_kind(f))
  upload_y!(X, f.y)                                   # also r = copy(y), as the loss constructors do
  f isa HipWLS && upload_w!(X, f.w)
  X.owner = f.r
  f
end

numCoordinates(f::HipLoss) = f.X.p

"does the handle already hold exactly this iterate (same support order, same values)?"
function is_synced(X::HipMatrix, x::SparseIterate)
  X.synced || return false
  m = nnz(x)
  m == length(X.synced_idx) || return false
  @inbounds for i in 1:m
    (x.nzval2ind[i] == X.synced_idx[i] && Float64(x.nzval[i]) == X.synced_val[i]) || return false
  end
  true
end
function remember_iterate!(X::HipMatrix, x::SparseIterate)
  m = nnz(x)
  X.synced_idx = Int64.(x.nzval2ind[1:m]); X.synced_val = Float64.(x.nzval[1:m]); X.synced = true
  nothing
end

"x -> the handle.  `rebuild` = initialize! (r = y - X x is formed, cd_differentiable_function.jl:59-72); without it an
iterate the handle already holds is not sent again."
function push_iterate!(f::HipLoss, x::SparseIterate, rebuild::Bool)
  !rebuild && is_synced(f.X, x) && return nothing
  idx = Int64.(x.nzval2ind[1:nnz(x)])
  val = Float64.(x.nzval[1:nnz(x)])
  GC.@preserve idx val begin          # ccall needs a constant symbol: one call site per entry point
    st = rebuild ?
      ccall((:cdh_initialize, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
            f.X.handle, length(x), length(idx), idx, val) :
      ccall((:cdh_set_iterate, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
            f.X.handle, length(x), length(idx), idx, val)
    check(f.X.handle, st)
  end
  f.X.synced_idx = idx; f.X.synced_val = val; f.X.synced = true
  nothing
end

"callers read f.r afterwards (src/lasso.jl:37,134,143): one device -> host copy"
pull_residual!(f::HipLoss) =
  check(f.X.handle, ccall((:cdh_get_residual, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), f.X.handle, f.r))

"x <- the handle's iterate, support in the library's insertion order (p-sized; nothing n-sized moves)"
function pull_support!(f::HipLoss{T}, x::SparseIterate{T}) where {T}
  p = f.X.p
  idx = Vector{Int64}(undef, p); nz = Ref{Int64}(0); beta = Vector{Float64}(undef, p)
  check(f.X.handle, ccall((:cdh_get_support, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ref{Int64}), f.X.handle, idx, nz))
  check(f.X.handle, ccall((:cdh_get_beta, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Float64}), f.X.handle, beta))
  fill!(x, zero(T))
  for i in 1:nz[]                       # re-insert in the library's support order
    x[idx[i]] = T(beta[idx[i]])
  end
  remember_iterate!(f.X, x)
  x
end

function pull_iterate!(f::HipLoss{T}, x::SparseIterate{T}) where {T}
  pull_support!(f, x)
  pull_residual!(f)
  x
end

function set_penalty!(f::HipLoss, g::ProxL1)
  om = g.λ === nothing ? Float64[] : Vector{Float64}(g.λ)    # kept alive across the call
  GC.@preserve om check(f.X.handle,
    ccall((:cdh_set_penalty, libcdhip), Int32, (Ptr{Cvoid}, Float64, Ptr{Float64}, Int64),
          f.X.handle, Float64(g.λ0), g.λ === nothing ? Ptr{Float64}(C_NULL) : pointer(om), length(om)))
end

# ---- the four-function operator interface (src/cd_differentiable_function.jl:1-35) ----------
function initialize!(f::HipLoss{T}, x::SparseIterate{T}) where {T}
  bind!(f); push_iterate!(f, x, true); pull_residual!(f)   # scaledLasso! :WarmStart reads std(f.r) next (:125-126)
  nothing
end

function gradient(f::HipLoss{T}, x::SparseIterate{T}, k::Int64) where {T}
  bind!(f); push_iterate!(f, x, false)
  out = Ref{Float64}(0)
  check(f.X.handle, ccall((:cdh_gradient, libcdhip), Int32, (Ptr{Cvoid}, Int64, Ref{Float64}), f.X.handle, k, out))
  T(out[])
end

"""descendCoordinate!(f, g, x, k) (cd_differentiable_function.jl:83-111) on the device.  x is refreshed (p-sized); the
residual is NOT copied back per visit -- n elements per call would be 80 MB per visit at n = 1e7 -- so inside a user-written
pass over this operator `f.r` is stale until `pull_residual!(f)` (or `initialize!`, or `coordinateDescent!`, which end
with one).  The reference's own `_cdPass!` (coordinate_descent.jl:102-107) never reads f.r between visits."""
function descendCoordinate!(f::HipLoss{T}, g::ProxL1{T}, x::SparseIterate{T}, k::Int64) where {T}
  bind!(f); set_penalty!(f, g); push_iterate!(f, x, false)
  out = Ref{Float64}(0)
  check(f.X.handle, ccall((:cdh_descend, libcdhip), Int32, (Ptr{Cvoid}, Int64, Ref{Float64}), f.X.handle, k, out))
  pull_support!(f, x)
  T(out[])
end

# ---- the performance path: one ccall per solve (src/coordinate_descent.jl:7-39) ---------------
"coordinateDescent! up to the point where results leave the device: x is refreshed, f.r is NOT"
function solve_resident!(x::SparseIterate{T}, f::HipLoss{T}, g::ProxL1, options::CDOptions) where {T}
  ProximalBase.numCoordinates(x) == numCoordinates(f) || throw(DimensionMismatch())
  bind!(f)
  set_penalty!(f, g)                  # checks length(g.λ) == p (coordinate_descent.jl:14-16)
  push_iterate!(f, x, false)
  opt = Ref(CdhOptions(options)); st = CdhStats()
  code = ccall((:cdh_coordinate_descent, libcdhip), Int32, (Ptr{Cvoid}, Ref{CdhOptions}, Ref{CdhStats}),
               f.X.handle, opt, st)
  check(f.X.handle, code)
  st.domain_error != 0 && throw(DomainError(NaN, "sqrt-lasso update"))
  pull_support!(f, x)
end

function coordinateDescent!(x::SparseIterate{T}, f::HipLoss{T}, g::ProxL1, options::CDOptions=CDOptions()) where {T}
  solve_resident!(x, f, g, options)
  pull_residual!(f)                   # callers read f.r next (lasso.jl:37,52,81,97)
  x
end

# ---- the dense helpers the front-ends call on X itself (src/utils.jl) ---------------------------
# Without these, LassoPath(standardizeX=true) and scaledLasso!(:Screening) would fall into the
# reference's generic loops over X[i, j] (a device round trip per element) and into BLAS / `\\` on a
# matrix that has no host memory.

"_stdX!(out, X) (utils.jl:127-138): out[j] = sqrt(sum_i X[i,j]^2 / n), one pass over X in HBM."
function _stdX!(out::Vector{T}, X::HipMatrix{T}) where {T<:AbstractFloat}
  length(out) == X.p || throw(DimensionMismatch())
  buf = Vector{Float64}(undef, X.p)
  check(X.handle, ccall((:cdh_col_rms, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Float64}), X.handle, buf))
  out .= T.(buf)
  out
end

"X'y for every column (the `mul!(storage, transpose(X), y)` of utils.jl:103): y goes to the device, r = y."
function xt_y(X::HipMatrix{T}, y::AbstractVector{T}) where {T}
  set_loss!(X, CDH_LS)
  upload_y!(X, y)
  X.owner = nothing                    # whatever loss was bound has lost its y: it re-binds on its next call
  check(X.handle, ccall((:cdh_initialize, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                        X.handle, X.p, 0, C_NULL, C_NULL))
  X.synced = false                     # the handle's iterate is zero now, nobody's x
  out = Vector{Float64}(undef, X.p)
  check(X.handle, ccall((:cdh_xt_r, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Float64}), X.handle, out))
  out
end

"_findLargestCorrelations(X, y, s) (utils.jl:96-106): BitVector of the columns with |X_j'y| >= the s-th largest."
function _findLargestCorrelations(X::HipMatrix{T}, y::AbstractVector{T}, s::Int) where {T<:AbstractFloat}
  storage = abs.(xt_y(X, y))
  storage .>= nlargest(s, storage)[end]
end

"Xs \\ y (utils.jl:70; a QR in the reference) from the Gram block G = Xs'Xs and c = Xs'y: the minimum-norm solution of the
normal equations through the symmetric eigendecomposition of G (directions under 1e-13 of the largest eigenvalue are left
out, as a rank-revealing QR leaves them out), refined twice against the normal equations' own residual Xs'(y - Xs b) --
initialize! forms the residual on the device, cdh_xt_r_cols dots it with the s columns -- so that near-collinear
screening columns do not cost the squared condition number.  Leaves r = y - Xs b on the device."
function screening_ols!(X::HipMatrix, idx::Vector{Int64})
  m = length(idx)
  m <= 4096 || throw(ArgumentError("screening set larger than 4096 columns"))
  G = Matrix{Float64}(undef, m, m); c = Vector{Float64}(undef, m)
  check(X.handle, ccall((:cdh_gram, libcdhip), Int32,
                        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                        X.handle, m, idx, G, c, C_NULL))
  E = eigen(Symmetric(G))
  keep = E.values .> 1e-13 * max(E.values[end], 0.0)
  V = E.vectors[:, keep]
  pinvG = (V ./ E.values[keep]') * V'
  coef = pinvG * c
  res = Vector{Float64}(undef, m)
  for _ in 1:2
    check(X.handle, ccall((:cdh_initialize, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                          X.handle, X.p, m, idx, coef))
    check(X.handle, ccall((:cdh_xt_r_cols, libcdhip), Int32, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}),
                          X.handle, m, idx, res))
    coef .+= pinvG * res
  end
  check(X.handle, ccall((:cdh_initialize, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                        X.handle, X.p, m, idx, coef))
  X.synced = false                     # the handle's iterate is the OLS fit now, nobody's x
  coef
end

"_findInitResiduals!(X, y, s, storage) (utils.jl:65-77): storage = y - Xs (Xs \\ y), any s; the residual is formed on
the device (screening_ols!) and copied back once."
function _findInitResiduals!(X::HipMatrix{T}, y::AbstractVector{T}, s::Int, storage::Vector{T}) where {T<:AbstractFloat}
  S = _findLargestCorrelations(X, y, s)             # leaves y on the device and r = y
  screening_ols!(X, Int64.(findall(S)))
  check(X.handle, ccall((:cdh_get_residual, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), X.handle, storage))
  storage
end
# _findInitSigma!(X, y, s, storage) = std(_findInitResiduals!(X, y, s, storage)) (utils.jl:60-64) is
# generic and lands in the method above.

# ---- the σ loop and the λ loop with nothing n-sized crossing the bus (src/lasso.jl:107-144, 229-260) ------
"sum r, sum r^2 of the device-side residual (all shards)"
function resid_moments(X::HipMatrix)
  s = Ref{Float64}(0); ss = Ref{Float64}(0)
  check(X.handle, ccall((:cdh_resid_moments, libcdhip), Int32, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}), X.handle, s, ss))
  s[], ss[]
end
"std(f.r) as Statistics.std computes it -- the mean, then the centred sum of squares (two passes on the device), Bessel-corrected"
function resid_std(X::HipMatrix)
  out = Ref{Float64}(0)
  check(X.handle, ccall((:cdh_resid_std, libcdhip), Int32, (Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}), X.handle, out, C_NULL))
  out[]
end

function gradient_cache_mode(X::HipMatrix)
  m = Ref{Int32}(0)
  check(X.handle, ccall((:cdh_get_gradient_cache, libcdhip), Int32, (Ptr{Cvoid}, Ref{Int32}), X.handle, m))
  m[]
end

"scaledLasso!(x, X, y, λ, ω, options) (lasso.jl:107-144) for a design in HBM: the reference's loop with σ taken
from the device-side residual; `f.r` comes back to the host once, for the LassoSolution."
function scaledLasso!(x::SparseIterate{T}, X::HipMatrix{T}, y::AbstractVector{T}, λ::T, ω::AbstractVector{T},
                      options::IterLassoOptions=IterLassoOptions()) where {T<:AbstractFloat}
  n = X.n
  f = CDLeastSquaresLoss(y, X)
  if options.initProcedure == :Screening
    # _findInitSigma! (utils.jl:60-64) without its copy back: scores, s x s normal equations, residual on the device
    S = _findLargestCorrelations(X, y, options.sinit)      # leaves y on the device, loss kind LS, r = y
    screening_ols!(X, Int64.(findall(S)))
    σ = T(resid_std(X))
    X.owner = f.r                     # the device holds exactly this loss's y and kind: no second upload
  elseif options.initProcedure == :InitStd
    σ = options.σinit
  elseif options.initProcedure == :WarmStart
    bind!(f); push_iterate!(f, x, true)
    σ = T(resid_std(X))
  else
    throw(ArgumentError("Incorrect initialization Symbol"))
  end
  g = ProxL1(λ * σ, ω)
  for iter = 1:options.maxIter
    solve_resident!(x, f, g, options.optionsCD)
    σnew = T(sqrt(resid_moments(X)[2] / n))                # sqrt(sum(abs2, f.r) / n), lasso.jl:134
    abs(σnew - σ) / σ < options.optTol && break
    σ = σnew
    g = ProxL1(λ * σ, ω)
  end
  pull_residual!(f)
  LassoSolution{T, typeof(g)}(x, f.r, g, T(resid_std(X)))
end

"_getLoadings!(out, X, e) (utils.jl:153-164) at e = the residual the device holds: out[j] = sqrt(sum_i (X[i,j] r[i])^2 / n),
one pass over X in HBM; the handle is left as it was."
function device_loadings!(out::Vector{T}, X::HipMatrix{T}) where {T<:AbstractFloat}
  length(out) == X.p || throw(DimensionMismatch())
  buf = Vector{Float64}(undef, X.p)
  check(X.handle, ccall((:cdh_loadings, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Float64}), X.handle, buf))
  out .= T.(buf)
  out
end

"feasibleLasso!(x, X, y, λ0, options) (lasso.jl:154-194) for a design in HBM, as the reference intends it: its own body stops
at `Array{T}(p)` (:164-165) and at `LassoSolution(x, f.r, g, std(f.r))` (:193, no such outer constructor) on Julia >= 1.0.
g aliases Γ as in the reference (:181), so the returned penalty carries the loadings computed after the last solve.
Nothing n-sized crosses the bus inside the loop; `f.r` comes back once, for the LassoSolution."
function feasibleLasso!(x::SparseIterate{T}, X::HipMatrix{T}, y::AbstractVector{T}, λ0::T,
                        options::IterLassoOptions=IterLassoOptions()) where {T<:AbstractFloat}
  p = X.p
  f = CDLeastSquaresLoss(y, X)
  Γ = Array{T}(undef, p)
  Γold = Array{T}(undef, p)
  if options.initProcedure == :Screening
    S = _findLargestCorrelations(X, y, options.sinit)      # leaves y on the device, loss kind LS, r = y
    screening_ols!(X, Int64.(findall(S)))                  # r = y - Xs (Xs \ y) stays on the device
    X.owner = f.r                     # the device holds exactly this loss's y and kind: no second upload
  elseif options.initProcedure == :InitStd
    _stdX!(Γ, X)
    solve_resident!(x, f, ProxL1(λ0 * options.σinit, Γ), options.optionsCD)
  elseif options.initProcedure == :WarmStart
    bind!(f); push_iterate!(f, x, true)
  else
    throw(ArgumentError("Incorrect initialization Symbol"))
  end
  device_loadings!(Γ, X)
  g = ProxL1(λ0, Γ)
  for iter = 1:options.maxIter
    copyto!(Γold, Γ)
    solve_resident!(x, f, g, options.optionsCD)
    device_loadings!(Γ, X)
    maximum(abs.(Γold - Γ)) / maximum(Γ) < options.optTol && break
  end
  pull_residual!(f)
  LassoSolution{T, typeof(g)}(x, f.r, g, T(resid_std(X)))
end

"LassoPath(X, Y, λpath, options; max_hat_s, standardizeX) (lasso.jl:229-260) for a design in HBM: one x and one f
for all λ as in the reference; warm starts keep the carried residual (it already equals Y - X x) and the gradient
cache is engaged from the first full pass for the duration of the path (whatever the caller set otherwise stays)."
function LassoPath(X::HipMatrix{T}, Y::StridedVector{T}, λpath::Vector{T}, options=CDOptions();
                   max_hat_s=Inf, standardizeX::Bool=true) where {T<:AbstractFloat}
  p = X.p
  stdX = Array{T}(undef, p)
  standardizeX ? _stdX!(stdX, X) : fill!(stdX, one(T))
  x = SparseIterate(T, p)
  f = CDLeastSquaresLoss(Y, X)
  numλ = length(λpath)
  βpath = Vector{SparseIterate{T}}(undef, numλ)
  mode_before = gradient_cache_mode(X)
  set_reuse_residual!(X, true)
  mode_before == 1 && set_gradient_cache!(X, 2)
  try
    for indλ = 1:numλ
      solve_resident!(x, f, ProxL1(λpath[indλ], stdX), options)
      βpath[indλ] = copy(x)
      if nnz(x) > max_hat_s
        resize!(λpath, indλ)
        break
      end
    end
  finally
    set_reuse_residual!(X, false)
    mode_before == 1 && set_gradient_cache!(X, 1)
  end
  LassoPath{T}(copy(λpath), βpath)
end

"refitLassoPath(path, X, Y) (lasso.jl:208-225) for a design in HBM: X[:, S] \ Y for every distinct support S along the path,
from the normal equations of the S columns at r = Y (cdh_gram) with the refinement of screening_ols!; supports already
seen are skipped.  More than 4096 columns in one support: ArgumentError.  The handle is left at β = 0 with r = Y."
function refitLassoPath(path::LassoPath{T}, X::HipMatrix{T}, Y::StridedVector{T}) where {T<:AbstractFloat}
  out = Dict{Vector{Int64},Vector{Float64}}()
  set_loss!(X, CDH_LS)
  upload_y!(X, Y)
  X.owner = nothing
  for i = 1:length(path.λpath)
    S = findall(!iszero, path.βpath[i])
    haskey(out, S) && continue
    check(X.handle, ccall((:cdh_initialize, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                          X.handle, X.p, 0, C_NULL, C_NULL))
    out[S] = isempty(S) ? Float64[] : screening_ols!(X, Int64.(S))
  end
  check(X.handle, ccall((:cdh_initialize, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                        X.handle, X.p, 0, C_NULL, C_NULL))
  X.synced = false                     # the handle's iterate is zero now, nobody's x
  out
end

# ---- l1-penalised logistic regression by IRLS (no reference counterpart) --------------------------------------
# A round solves the weighted lasso of CDWeightedLSLoss (cd_differentiable_function.jl:118-194) on the working response
# and weights; the step between two rounds runs on the device (cdh_glm_irls), so nothing n-sized moves per round.
"the 0/1 labels (proportions in [0, 1] allowed) of a Float64 design under the weighted loss; the working response is zeroed"
function glm_set_labels!(X::HipMatrix{Float64}, labels::Vector{Float64})
  length(labels) == X.n || throw(DimensionMismatch())
  set_loss!(X, CDH_WLS)
  check(X.handle, ccall((:cdh_glm_set_labels, libcdhip), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}), X.handle, Int32(0), labels))
  X.owner = nothing
  X.synced = false
  X
end

function glm_get_labels(X::HipMatrix{Float64})
  out = Vector{Float64}(undef, X.n)
  check(X.handle, ccall((:cdh_glm_get_labels, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), X.handle, out))
  out
end

"one IRLS step at the iterate the handle holds: (Σ nll, Σ w, clamped rows); apply=false reads only"
function glm_irls!(X::HipMatrix{Float64}; apply::Bool=true, wmin::Float64=1e-5)
  out = Vector{Float64}(undef, 3)
  check(X.handle, ccall((:cdh_glm_irls, libcdhip), Int32, (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}),
                        X.handle, Int32(apply), wmin, out))
  (nll = out[1] / X.n, sum_w = out[2], clamped = Int(out[3]))
end

"the same step inside fold k (0-based, -1: none) of the folds the handle holds: held-out rows get w = 0, z = η and r = 0, and their Σ nll and misclassified rows are returned beside the training rows' sums"
function glm_irls_fold!(X::HipMatrix{Float64}, k::Integer; apply::Bool=true, wmin::Float64=1e-5)
  out = Vector{Float64}(undef, 5)
  check(X.handle, ccall((:cdh_glm_irls_fold, libcdhip), Int32, (Ptr{Cvoid}, Int32, Int32, Float64, Ptr{Float64}),
                        X.handle, Int32(k), Int32(apply), wmin, out))
  (nll = out[1] / X.n, sum_w = out[2], clamped = Int(out[3]), held_nll = out[4], held_miss = out[5])
end

# ---- l1-penalised Poisson regression with an offset, by the same loop (no reference counterpart) ---------------
"the counts (≥ 0) and, optionally, the offsets (log exposure) of a Float64 design under the weighted loss; the working response is zeroed"
function glm_set_counts!(X::HipMatrix{Float64}, counts::Vector{Float64}, offset::Union{Nothing,Vector{Float64}}=nothing)
  length(counts) == X.n || throw(DimensionMismatch())
  offset === nothing || length(offset) == X.n || throw(DimensionMismatch())
  set_loss!(X, CDH_WLS)
  check(X.handle, ccall((:cdh_glm_set_counts, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                        X.handle, counts, offset === nothing ? C_NULL : pointer(offset)))
  X.owner = nothing
  X.synced = false
  X
end

function glm_get_offset(X::HipMatrix{Float64})
  out = Vector{Float64}(undef, X.n)
  check(X.handle, ccall((:cdh_glm_get_offset, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), X.handle, out))
  out
end

"one Poisson IRLS step at the iterate the handle holds, fold k (0-based, -1: none) held out; apply=false reads only"
function glm_poisson_irls!(X::HipMatrix{Float64}, k::Integer=-1; apply::Bool=true, wmin::Float64=1e-5, eta_max::Float64=50.0)
  out = Vector{Float64}(undef, 6)
  check(X.handle, ccall((:cdh_glm_poisson_irls, libcdhip), Int32, (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Ptr{Float64}),
                        X.handle, Int32(k), Int32(apply), wmin, eta_max, out))
  (nll = out[1] / X.n, sum_w = out[2], clamped = Int(out[3]), capped = Int(out[4]), held_deviance = out[5], deviance = out[6])
end

"observation weights (finite, > 0; stored as given) of a design that holds labels or counts; nothing drops them. y, r and the iterate stay"
function glm_set_weights!(X::HipMatrix{Float64}, weights::Union{Nothing,Vector{Float64}})
  weights === nothing || length(weights) == X.n || throw(DimensionMismatch())
  check(X.handle, ccall((:cdh_glm_set_weights, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}),
                        X.handle, weights === nothing ? C_NULL : pointer(weights)))
  X
end

"the observation weights of a design that holds labels or counts; ones when none are set"
function glm_get_weights(X::HipMatrix{Float64})
  out = Vector{Float64}(undef, X.n)
  check(X.handle, ccall((:cdh_glm_get_weights, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), X.handle, out))
  out
end

# ---- l1-penalised Cox regression, Breslow ties, by the same loop (no reference counterpart) --------------------
"the times, the statuses (1: event, 0: censored) and, optionally, the offsets of a Float64 design under the weighted loss; the working response is zeroed"
function glm_set_survival!(X::HipMatrix{Float64}, time::Vector{Float64}, status::Vector{Float64}, offset::Union{Nothing,Vector{Float64}}=nothing)
  length(time) == X.n && length(status) == X.n || throw(DimensionMismatch())
  offset === nothing || length(offset) == X.n || throw(DimensionMismatch())
  set_loss!(X, CDH_WLS)
  check(X.handle, ccall((:cdh_glm_set_survival, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                        X.handle, time, status, offset === nothing ? C_NULL : pointer(offset)))
  X.owner = nothing
  X.synced = false
  X
end

function glm_get_survival(X::HipMatrix{Float64})
  time = Vector{Float64}(undef, X.n)
  status = Vector{Float64}(undef, X.n)
  check(X.handle, ccall((:cdh_glm_get_survival, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), X.handle, time, status))
  (time, status)
end

"glm_set_survival! with stratum ids (Int32; nothing: one stratum) and observation weights (stored as given; nothing: ones); with neither it is glm_set_survival!"
function glm_set_survival_strata!(X::HipMatrix{Float64}, time::Vector{Float64}, status::Vector{Float64}, offset::Union{Nothing,Vector{Float64}}=nothing;
                                  strata::Union{Nothing,Vector{Int32}}=nothing, weights::Union{Nothing,Vector{Float64}}=nothing,
                                  ties::Symbol=:breslow)
  length(time) == X.n && length(status) == X.n || throw(DimensionMismatch())
  for v in (offset, strata, weights)
    v === nothing || length(v) == X.n || throw(DimensionMismatch())
  end
  ties in (:breslow, :efron) || throw(ArgumentError("ties must be :breslow or :efron"))
  set_loss!(X, CDH_WLS)
  check(X.handle, ccall((:cdh_glm_set_survival_strata, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Cvoid}),
                        X.handle, time, status, offset === nothing ? C_NULL : pointer(offset),
                        strata === nothing ? C_NULL : pointer(strata), weights === nothing ? C_NULL : pointer(weights)))
  X.owner = nothing
  X.synced = false
  glm_set_cox_ties!(X, ties)
end

"the tie rule of a Cox handle's steps: :breslow (the default) or :efron (survival::coxph's default; refused with start times). The setters of survival data keep it, except that start times put it back to :breslow."
function glm_set_cox_ties!(X::HipMatrix{Float64}, ties::Symbol)
  ties in (:breslow, :efron) || throw(ArgumentError("ties must be :breslow or :efron"))
  check(X.handle, ccall((:cdh_glm_set_cox_ties, libcdhip), Int32, (Ptr{Cvoid}, Int32), X.handle, Int32(ties === :efron)))
  X
end

function glm_get_cox_ties(X::HipMatrix{Float64})
  out = Ref{Int32}(0)
  check(X.handle, ccall((:cdh_glm_get_cox_ties, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Int32}), X.handle, out))
  out[] == 1 ? :efron : :breslow
end

"the stratum ids (zeros without strata) and the observation weights (ones without weights) of a Cox handle, in the caller's row order"
function glm_get_survival_strata(X::HipMatrix{Float64})
  strata = Vector{Int32}(undef, X.n)
  weights = Vector{Float64}(undef, X.n)
  check(X.handle, ccall((:cdh_glm_get_survival_strata, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Cvoid}), X.handle, strata, weights))
  (strata, weights)
end

"glm_set_survival_strata! with start times: row i is at risk over (start[i], stop[i]]; start === nothing: it is glm_set_survival_strata!"
function glm_set_survival_interval!(X::HipMatrix{Float64}, start::Union{Nothing,Vector{Float64}}, stop::Vector{Float64}, status::Vector{Float64},
                                    offset::Union{Nothing,Vector{Float64}}=nothing;
                                    strata::Union{Nothing,Vector{Int32}}=nothing, weights::Union{Nothing,Vector{Float64}}=nothing)
  length(stop) == X.n && length(status) == X.n || throw(DimensionMismatch())
  for v in (start, offset, strata, weights)
    v === nothing || length(v) == X.n || throw(DimensionMismatch())
  end
  set_loss!(X, CDH_WLS)
  check(X.handle, ccall((:cdh_glm_set_survival_interval, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Cvoid}),
                        X.handle, start === nothing ? C_NULL : pointer(start), stop, status, offset === nothing ? C_NULL : pointer(offset),
                        strata === nothing ? C_NULL : pointer(strata), weights === nothing ? C_NULL : pointer(weights)))
  X.owner = nothing
  X.synced = false
  X
end

"the start times of a Cox handle set by glm_set_survival_interval!, in the caller's row order"
function glm_get_survival_start(X::HipMatrix{Float64})
  start = Vector{Float64}(undef, X.n)
  check(X.handle, ccall((:cdh_glm_get_survival_start, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), X.handle, start))
  start
end

"one Cox IRLS step at the iterate the handle holds, fold k (0-based, -1: none) held out; apply=false reads only"
function glm_cox_irls!(X::HipMatrix{Float64}, k::Integer=-1; apply::Bool=true, wmin::Float64=1e-5, eta_max::Float64=50.0)
  out = Vector{Float64}(undef, 5)
  check(X.handle, ccall((:cdh_glm_cox_irls, libcdhip), Int32, (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Ptr{Float64}),
                        X.handle, Int32(k), Int32(apply), wmin, eta_max, out))
  (nll = out[1] / X.n, sum_w = out[2], clamped = Int(out[3]), capped = Int(out[4]), events = isinteger(out[5]) ? Int(out[5]) : out[5])   # the sum of v delta: the event count, an Int, without weights
end

"residuals of the Cox model at the iterate the handle holds, in the caller's row order: (cumhaz, martingale, deviance); survival's residuals(coxph, type = \"martingale\" / \"deviance\"), cumhaz the baseline cumulative hazard over the row's time at risk (uncentred)"
function glm_cox_residuals(X::HipMatrix{Float64}; eta_max::Float64=50.0)
  cumhaz, martingale, deviance = (Vector{Float64}(undef, X.n) for _ in 1:3)
  check(X.handle, ccall((:cdh_glm_cox_residuals, libcdhip), Int32, (Ptr{Cvoid}, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                        X.handle, eta_max, cumhaz, martingale, deviance))
  (cumhaz = cumhaz, martingale = martingale, deviance = deviance)
end

"the cumulative baseline hazard of the Cox model at the iterate the handle holds (R's basehaz, uncentred): one entry per (stratum, event time) in that order; events: an upper bound of the table's length, the number of events"
function glm_cox_baseline(X::HipMatrix{Float64}, events::Integer; eta_max::Float64=50.0)
  stratum = Vector{Int32}(undef, events)
  time, n_event, risk_sum, cumhaz, cumvar = (Vector{Float64}(undef, events) for _ in 1:5)
  count = Ref{Int64}(0)
  check(X.handle, ccall((:cdh_glm_cox_baseline, libcdhip), Int32,
                        (Ptr{Cvoid}, Float64, Int64, Ptr{Int32}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}),
                        X.handle, eta_max, Int64(events), stratum, time, n_event, risk_sum, cumhaz, cumvar, count))
  m = Int(count[])
  (stratum = stratum[1:m], time = time[1:m], n_event = n_event[1:m], risk_sum = risk_sum[1:m], cumhaz = cumhaz[1:m], cumvar = cumvar[1:m])
end

"Harrell's concordance index of the Cox model at the iterate the handle holds (survival::concordance, glmnet's Cindex): over all rows (k = -1) or over the held-out rows of fold k (0-based, after set_folds!); the pair counts carry the weights v_i v_j"
function glm_cox_concordance(X::HipMatrix{Float64}, k::Integer=-1)
  out = Vector{Float64}(undef, 4)
  check(X.handle, ccall((:cdh_glm_cox_concordance, libcdhip), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}), X.handle, Int32(k), out))
  out[4] > 0 && throw(ArgumentError("eta is NaN in $(Int(out[4])) rows"))
  comparable = out[1] + out[2] + out[3]
  (concordant = out[1], discordant = out[2], tied = out[3], comparable = comparable, C = comparable > 0 ? (out[1] + out[3] / 2) / comparable : NaN)
end

"score residuals (n x m), Schoenfeld residuals (n x m, zero off the events) and the information matrix (m x m) of the Cox model at the iterate the handle holds, for the 1-based columns idx (at most 64), Breslow ties; centre: the columns' centres, or nothing for their means"
function glm_cox_score(X::HipMatrix{Float64}, idx::Vector{Int64}; centre::Union{Nothing,Vector{Float64}}=nothing, eta_max::Float64=50.0)
  n, m = size(X, 1), length(idx)
  sch, score = Matrix{Float64}(undef, n, m), Matrix{Float64}(undef, n, m)
  info, used = Matrix{Float64}(undef, m, m), Vector{Float64}(undef, m)
  check(X.handle, ccall((:cdh_glm_cox_score, libcdhip), Int32,
                        (Ptr{Cvoid}, Float64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}),
                        X.handle, eta_max, Int64(m), idx, centre === nothing ? C_NULL : centre, used, sch, score, info))
  (schoenfeld = sch, score = score, info = info, centre = used)
end

# ---- locpolyl1 with the design expanded on the device (src/varying_coefficient_lasso.jl:30-79) ----------------
# The reference rebuilds w, expandX and stdX on the host for every z0 (:63-65).  A HipVaryingDesign keeps the base
# design and z in HBM; cdh_vc_set_point regenerates all three there, and the refit (:71-76) reads its weighted normal
# equations off one Gram block at the solve's own residual.  Nothing n-sized crosses the bus per grid point.
kernel_code(::CoordinateDescent.GaussianKernel) = Int32(0)
kernel_code(::CoordinateDescent.EpanechnikovKernel) = Int32(1)

mutable struct HipVaryingDesign{T<:Union{Float32,Float64}}
  handle::Ptr{Cvoid}
  n::Int
  p::Int          # base columns
  degree::Int
end

"Upload X (n x p) and z once: base column j becomes column (j-1)(degree+1)+1 of the expanded design in HBM."
function HipVaryingDesign(X::StridedMatrix{T}, z::Vector{T}, degree::Int; device::Integer=0) where {T}
  n, p = size(X)
  length(z) == n || throw(DimensionMismatch())
  0 <= degree <= 3 || throw(ArgumentError("the polynomial degree must be 0 .. 3"))
  ref = Ref{Ptr{Cvoid}}(C_NULL)
  check(C_NULL, ccall((:cdh_create, libcdhip), Int32,
                      (Ref{Ptr{Cvoid}}, Int32, Int32, Int64, Int64, Int64, Int64, Int32),
                      ref, dtype_code(T), CDH_WLS, n, n, 0, p * (degree + 1), device))
  h = ref[]
  GC.@preserve X z check(h, ccall((:cdh_vc_set_data, libcdhip), Int32,
                                  (Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
                                  h, p, degree, X, stride(X, 2), z))
  D = HipVaryingDesign{T}(h, n, p, degree)
  finalizer(d -> ccall((:cdh_destroy, libcdhip), Int32, (Ptr{Cvoid},), d.handle), D)
  D
end

"w, expandX and stdX of one grid point (:63-65), on the device; returns stdX"
function set_point!(D::HipVaryingDesign{T}, kernel::CoordinateDescent.SmoothingKernel{T}, z0::T) where {T}
  out = Vector{Float64}(undef, D.p * (D.degree + 1))
  check(D.handle, ccall((:cdh_vc_set_point, libcdhip), Int32, (Ptr{Cvoid}, Int32, Float64, Float64, Ptr{Float64}),
                        D.handle, kernel_code(kernel), Float64(kernel.h), Float64(z0), out))
  out
end

"_stdX!(out, w, X) (utils.jl:140-151) of whatever weights and columns the handle holds"
function weighted_stdX(D::HipVaryingDesign)
  out = Vector{Float64}(undef, D.p * (D.degree + 1))
  check(D.handle, ccall((:cdh_col_wrms, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Float64}), D.handle, out))
  out
end

function CoordinateDescent.locpolyl1(D::HipVaryingDesign{T}, y::Vector{T}, zgrid::Vector{T},
                                     kernel::CoordinateDescent.SmoothingKernel{T}, λ0::T, refit::Bool,
                                     options::CDOptions=CDOptions()) where {T}
  length(y) == D.n || throw(DimensionMismatch())
  opt = CDOptions(options.maxIter, options.optTol, options.randomize, true, options.numSteps)   # :39-42
  h, ep = D.handle, D.p * (D.degree + 1)
  out = zeros(T, ep, length(zgrid)); outR = zeros(T, ep, length(zgrid))
  GC.@preserve y check(h, ccall((:cdh_set_y, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), h, y))
  check(h, ccall((:cdh_set_iterate, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                 h, ep, 0, C_NULL, C_NULL))                       # β = SparseIterate(ep), kept on the handle from here on
  beta = Vector{Float64}(undef, ep)
  for (ind, z0) in enumerate(zgrid)
    stdX = set_point!(D, kernel, z0)                              # :63-65
    check(h, ccall((:cdh_set_penalty, libcdhip), Int32, (Ptr{Cvoid}, Float64, Ptr{Float64}, Int64),
                   h, Float64(λ0), stdX, ep))
    o = Ref(CdhOptions(opt)); st = CdhStats()
    check(h, ccall((:cdh_coordinate_descent, libcdhip), Int32, (Ptr{Cvoid}, Ref{CdhOptions}, Ref{CdhStats}), h, o, st))   # :68
    check(h, ccall((:cdh_get_beta, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Float64}), h, beta))
    out[:, ind] .= T.(beta)
    refit || continue
    S = Int64[]                                                   # get_nonzero_coordinates!(S, β, p, degree, true)
    for j in 1:D.p
      ks = ((j - 1) * (D.degree + 1) + 1):(j * (D.degree + 1))
      any(!iszero, view(beta, ks)) && append!(S, ks)
    end
    isempty(S) && continue
    m = length(S)
    m <= 4096 || throw(ArgumentError("refit support larger than 4096 columns"))
    G = Matrix{Float64}(undef, m, m); c = Vector{Float64}(undef, m)
    check(h, ccall((:cdh_gram_weighted, libcdhip), Int32,
                   (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, m, S, G, c, C_NULL))
    # Xs'Wy = Xs'Wr + (Xs'WXs) β_S: (Xs'WXs) \ (Xs'Wy) = β_S + (Xs'WXs) \ (Xs'Wr), solved at unit diagonal (:73-75)
    d = sqrt.([G[i, i] for i in 1:m])
    outR[S, ind] .= T.(beta[S] .+ ((G ./ (d * d')) \ (c ./ d)) ./ d)
  end
  out, outR
end

# ---- lvocv_locpolyl1 on the same resident design (src/varying_coefficient_lasso.jl:82-137) --------------------------
# Per bandwidth and observation i the reference rebuilds w (with w[i] = 0), wX and stdX around z0 = z[i] on the host
# (:109-113).  cdh_vc_set_point_loo regenerates them on the device and returns the screening scores of
# _findLargestCorrelations(w, X, y, s) (utils.jl:108-124) from the same pass; the weighted OLS of _findInitResiduals!
# (utils.jl:79-92), _getSigma (utils.jl:167-175), the refit and the prediction read s x s blocks, two sums and one row.
"w (w[row] = 0), wX, stdX of the point z0 = z[row] (:109-113) and the scores |X_j'Wy|; `row` is 1-based; returns (stdX, scores)"
function set_point_leave_out!(D::HipVaryingDesign{T}, kernel::CoordinateDescent.SmoothingKernel{T}, row::Int) where {T}
  ep = D.p * (D.degree + 1)
  stdX = Vector{Float64}(undef, ep); scores = Vector{Float64}(undef, ep)
  check(D.handle, ccall((:cdh_vc_set_point_loo, libcdhip), Int32,
                        (Ptr{Cvoid}, Int32, Float64, Int64, Ptr{Float64}, Ptr{Float64}),
                        D.handle, kernel_code(kernel), Float64(kernel.h), row - 1, stdX, scores))
  stdX, scores
end

"_getSigma(w, f.r) (utils.jl:167-175) at the device-side residual"
function getSigma(D::HipVaryingDesign)
  sw = Ref{Float64}(0); swr2 = Ref{Float64}(0)
  check(D.handle, ccall((:cdh_resid_wmoments, libcdhip), Int32, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}), D.handle, sw, swr2))
  sqrt(swr2[] / sw[])
end

"_findInitResiduals!(w, wX, y, s, f.r) (utils.jl:79-92) from the scores: leaves r = y - X_S (X_S'WX_S) \\ (X_S'Wy) on the device"
function weighted_screening_init!(D::HipVaryingDesign, scores::Vector{Float64}, s::Int)
  h, ep = D.handle, D.p * (D.degree + 1)
  idx = Int64.(findall(scores .>= nlargest(s, scores)[end]))
  m = length(idx)
  m <= 4096 || throw(ArgumentError("screening set larger than 4096 columns"))
  check(h, ccall((:cdh_initialize, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                 h, ep, 0, C_NULL, C_NULL))                       # r = y: X_S'Wr == X_S'Wy
  G = Matrix{Float64}(undef, m, m); c = Vector{Float64}(undef, m)
  check(h, ccall((:cdh_gram_weighted, libcdhip), Int32,
                 (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, m, idx, G, c, C_NULL))
  E = eigen(Symmetric(G))
  keep = E.values .> 1e-13 * max(E.values[end], 0.0)
  V = E.vectors[:, keep]
  pinvG = (V ./ E.values[keep]') * V'
  coef = pinvG * c
  res = Vector{Float64}(undef, m)
  for _ in 1:2                                                    # refined against X_S'W(y - X_S b), as screening_ols! refines
    check(h, ccall((:cdh_initialize, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                   h, ep, m, idx, coef))
    check(h, ccall((:cdh_xt_r_cols, libcdhip), Int32, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}), h, m, idx, res))
    coef .+= pinvG * res
  end
  check(h, ccall((:cdh_initialize, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                 h, ep, m, idx, coef))
  idx
end

"lvocv_locpolyl1 (:82-137) for a design in HBM; an empty support, which the reference never handles, predicts Yh = 0"
function CoordinateDescent.lvocv_locpolyl1(D::HipVaryingDesign{T}, y::Vector{T}, hArr::Vector{T},
                                           kernelType::Type{<:CoordinateDescent.SmoothingKernel}, λ0::T,
                                           options::CDOptions=CDOptions()) where {T}
  length(y) == D.n || throw(DimensionMismatch())
  opt = CDOptions(options.maxIter, options.optTol, options.randomize, true, options.numSteps)   # :94
  h, ep, Q1 = D.handle, D.p * (D.degree + 1), D.degree + 1
  MSE = zeros(length(hArr))
  GC.@preserve y check(h, ccall((:cdh_set_y, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), h, y))
  nsup = 0; sup = Vector{Int64}(undef, ep); val = Vector{Float64}(undef, ep)   # β = SparseIterate(ep), carried over all points
  beta = Vector{Float64}(undef, ep)
  for (indH, bw) in enumerate(hArr)
    kernel = CoordinateDescent.createKernel(kernelType, bw)                   # :106
    for i in 1:D.n
      stdX, scores = set_point_leave_out!(D, kernel, i)                       # :109-113
      weighted_screening_init!(D, scores, min(10, ep))                        # :114
      σ = getSigma(D)                                                         # :117
      # the screening fit is the handle's iterate now: put β back (the warm start below rebuilds r = y - Xβ from it)
      check(h, ccall((:cdh_set_iterate, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                     h, ep, nsup, sup, val))
      for iter = 1:10                                                         # :119-127
        check(h, ccall((:cdh_set_penalty, libcdhip), Int32, (Ptr{Cvoid}, Float64, Ptr{Float64}, Int64),
                       h, Float64(λ0) * σ, stdX, ep))
        o = Ref(CdhOptions(opt)); st = CdhStats()
        check(h, ccall((:cdh_coordinate_descent, libcdhip), Int32, (Ptr{Cvoid}, Ref{CdhOptions}, Ref{CdhStats}), h, o, st))
        σnew = getSigma(D)
        abs(σnew - σ) / σ < 1e-2 && break
        σ = σnew
      end
      n_ref = Ref{Int64}(0)
      check(h, ccall((:cdh_get_support, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ref{Int64}), h, sup, n_ref))
      check(h, ccall((:cdh_get_beta, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Float64}), h, beta))
      nsup = n_ref[]
      for s in 1:nsup
        val[s] = beta[sup[s]]
      end
      S = Int64[]                                                             # get_nonzero_coordinates!(S, β, p, degree, true), :130
      for j in 1:D.p
        ks = ((j - 1) * Q1 + 1):(j * Q1)
        any(!iszero, view(beta, ks)) && append!(S, ks)
      end
      Yh = 0.0
      if !isempty(S)                                                          # :131-132
        m = length(S)
        m <= 4096 || throw(ArgumentError("refit support larger than 4096 columns"))
        G = Matrix{Float64}(undef, m, m); c = Vector{Float64}(undef, m)
        check(h, ccall((:cdh_gram_weighted, libcdhip), Int32,
                       (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, m, S, G, c, C_NULL))
        d = sqrt.([G[k, k] for k in 1:m])
        coef = beta[S] .+ ((G ./ (d * d')) \ (c ./ d)) ./ d
        base = S[1:Q1:end]                 # at z0 = z[i] row i of wX is X[i, j] at power 0 and exactly 0 above it
        row = Vector{Float64}(undef, length(base))
        check(h, ccall((:cdh_get_X_row, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Float64}),
                       h, i - 1, length(base), base, row))
        Yh = dot(row, coef[1:Q1:end])
      end
      MSE[indH] += (Yh - y[i])^2                                              # :133
    end
  end
  MSE
end

# ---- locpoly on a grid and lvocv_locpoly (src/varying_coefficient_lasso.jl:217-235, 348-380) -----------------------------
# The reference forms w, expandX and a QR per point.  cdh_vc_gram_batch takes _expand_Xt_w_X! / _expand_Xt_w_Y! (:572-647)
# of many points in one launch straight from the resident base design -- point t bit-identical to cdh_vc_gram at that
# point -- and the ep x ep systems are solved here from the symmetrically scaled normal equations.
const VC_GRAM_BATCH = 4096          # points per call: the host blocks of one call stay modest

"G (ep x ep x m), c (ep x m) and Σω (m) around m points: bandwidths bw, points z0 and/or left-out rows (1-based, 0 for none)"
function vc_gram_batch(D::HipVaryingDesign{T}, kind::Int32, bw::Vector{Float64}, z0::Union{Nothing,Vector{Float64}},
                       leave_out::Union{Nothing,Vector{Int}}) where {T}
  m, ep = length(bw), D.p * (D.degree + 1)
  (z0 === nothing || length(z0) == m) && (leave_out === nothing || length(leave_out) == m) || throw(DimensionMismatch())
  G = Array{Float64}(undef, ep, ep, m); c = Matrix{Float64}(undef, ep, m); sw = Vector{Float64}(undef, m)
  idx = collect(Int64, 1:D.p)
  lo = leave_out === nothing ? Int64[] : Int64.(leave_out .- 1)
  zz = z0 === nothing ? Float64[] : z0
  GC.@preserve zz lo check(D.handle, ccall((:cdh_vc_gram_batch, libcdhip), Int32,
        (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int32, Ptr{Cvoid}, Int64, Ptr{Int64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        D.handle, kind, m, bw, z0 === nothing ? C_NULL : pointer(zz), leave_out === nothing ? C_NULL : pointer(lo),
        1, C_NULL, D.p, idx, G, c, sw))
  G, c, sw
end

"the local polynomial fits around m points, ep x m: batches of VC_GRAM_BATCH points, each system scaled to unit diagonal"
function locpoly_points(D::HipVaryingDesign, kind::Int32, bw::Vector{Float64}, z0, leave_out)
  m, ep = length(bw), D.p * (D.degree + 1)
  out = Matrix{Float64}(undef, ep, m)
  for s in 1:VC_GRAM_BATCH:m
    t = s:min(m, s + VC_GRAM_BATCH - 1)
    G, c, _ = vc_gram_batch(D, kind, bw[t], z0 === nothing ? nothing : z0[t], leave_out === nothing ? nothing : leave_out[t])
    for (k, pt) in enumerate(t)
      d = sqrt.([G[i, i, k] for i in 1:ep])
      out[:, pt] .= ((view(G, :, :, k) ./ (d * d')) \ (view(c, :, k) ./ d)) ./ d
    end
  end
  out
end

"locpoly(X, z, y, zgrid, degree, kernel) (:217-235) for a design in HBM: ep x length(zgrid)"
function CoordinateDescent.locpoly(D::HipVaryingDesign{T}, y::Vector{T}, zgrid::Vector{T},
                                   kernel::CoordinateDescent.SmoothingKernel{T}) where {T}
  length(y) == D.n || throw(DimensionMismatch())
  GC.@preserve y check(D.handle, ccall((:cdh_set_y, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), D.handle, y))
  T.(locpoly_points(D, kernel_code(kernel), fill(Float64(kernel.h), length(zgrid)), Float64.(zgrid), nothing))
end

"lvocv_locpoly(X, z, y, degree, hArr, kernelType) (:348-380) for a design in HBM: the left-out row gets weight zero (:432-436)"
function CoordinateDescent.lvocv_locpoly(D::HipVaryingDesign{T}, y::Vector{T}, hArr::Vector{T},
                                         kernelType::Type{<:CoordinateDescent.SmoothingKernel}) where {T}
  length(y) == D.n || throw(DimensionMismatch())
  h, n, Q1 = D.handle, D.n, D.degree + 1
  GC.@preserve y check(h, ccall((:cdh_set_y, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), h, y))
  Xb = Matrix{T}(undef, n, D.p)                                   # the base columns, fetched once: column (j-1)(degree+1)+1
  GC.@preserve Xb for j in 1:D.p
    check(h, ccall((:cdh_get_X_cols, libcdhip), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64),
                   h, (j - 1) * Q1, 1, pointer(Xb, (j - 1) * n + 1), n))
  end
  kind = kernel_code(CoordinateDescent.createKernel(kernelType, hArr[1]))
  bw = repeat(Float64.(hArr), inner=n)                            # all (bandwidth, observation) pairs
  hbeta = locpoly_points(D, kind, bw, nothing, repeat(collect(1:n), outer=length(hArr)))
  MSE = zeros(length(hArr))
  for indH in 1:length(hArr), i in 1:n                            # in index order per bandwidth (:362-376)
    Yh = dot(Float64.(view(Xb, i, :)), view(hbeta, 1:Q1:size(hbeta, 1), (indH - 1) * n + i))
    MSE[indH] += (Yh - y[i])^2
  end
  MSE
end

# Optional knobs (no reference counterpart): blocked sweep width, screened full passes, the gradient
# cache of repeated solves, hipGraph replay, reuse of the carried residual by warm starts (what LassoPath
# wants: src/lasso.jl:250-252).
set_sweep_mode!(X::HipMatrix, blocked::Bool, block::Integer=32) =
  check(X.handle, ccall((:cdh_set_sweep_mode, libcdhip), Int32, (Ptr{Cvoid}, Int32, Int32), X.handle, blocked ? 1 : 0, block))
set_screening!(X::HipMatrix, level::Integer) =
  check(X.handle, ccall((:cdh_set_screening, libcdhip), Int32, (Ptr{Cvoid}, Int32), X.handle, level))
"0 off, 1 (default) engages once it has paid for itself, 2 from the first full pass: ask for 2 before LassoPath"
set_gradient_cache!(X::HipMatrix, mode::Integer) =
  check(X.handle, ccall((:cdh_set_gradient_cache, libcdhip), Int32, (Ptr{Cvoid}, Int32), X.handle, mode))
set_use_graph!(X::HipMatrix, on::Bool) =
  check(X.handle, ccall((:cdh_set_use_graph, libcdhip), Int32, (Ptr{Cvoid}, Int32), X.handle, on ? 1 : 0))
set_reuse_residual!(X::HipMatrix, on::Bool) =
  check(X.handle, ccall((:cdh_set_reuse_residual, libcdhip), Int32, (Ptr{Cvoid}, Int32), X.handle, on ? 1 : 0))
"The one-launch solve of problems whose Gram matrix fits on chip (p ≤ 1024; on by default): the reference's own shapes"
set_onchip_solve!(X::HipMatrix, on::Bool) =
  check(X.handle, ccall((:cdh_set_onchip_solve, libcdhip), Int32, (Ptr{Cvoid}, Int32), X.handle, on ? 1 : 0))
"(solves run in one launch, Gram matrices built) on this design so far"
function onchip_stats(X::HipMatrix)
  out = zeros(Int64, 2)
  check(X.handle, ccall((:cdh_onchip_stats, libcdhip), Int32, (Ptr{Cvoid}, Ptr{Int64}), X.handle, out))
  (out[1], out[2])
end

end # module
