"""cdh_profile_end's (launches, algorithmic bytes) of a streamed pass -- the figures behind the roofline fraction bench.py
reports -- are exactly what the plan's model gives for the moves the pass made (csrc/sweep_plan.hpp: chunk_traffic, through its
twin tests/_sweep_plan.py, which tests/test_sweep_plan_host.py holds to the header on the CPU).

One chunk per pass: n = 1000, p = 70 gives one full block and a short last one at every width up to 64.  The data is
test_gpu_residual_writers._data's: planted coordinates move, the others carry an infinite-looking penalty weight and stay
(h = 0 exactly), so both blocks see both kinds of visit; which visits moved is read off the iterate the pass returns (it
starts from zero and no coordinate repeats).  The gradient cache, screening and the one-launch solve are off: the pass is
streamed.  Every term of the model is an integer number of bytes, so the comparison is exact."""
import zlib

import numpy as np
import pytest

import coordinatedescent_jl_amd as cd
import _sweep_plan as SP
from test_gpu_kernel_sums import cus  # noqa: F401  (torch must meet the device before the library opens it: test_gpu_residual_writers)
from test_gpu_residual_writers import _data, _make_loss

pytestmark = pytest.mark.gpu

N, P = 1000, 70
MOVERS = [0, 3, 4, 17, 31, 32, 47, 63, 65, 69]          # in the full block of every width and in the short last one; the last visit moves
ROUTES = ["coord", 4, 16, 32, 64]


@pytest.mark.parametrize("weights", [False, True], ids=["ls", "wls"])
@pytest.mark.parametrize("route", ROUTES, ids=[str(r) for r in ROUTES])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_profile_of_a_streamed_pass_is_the_plans_model(cus, dtype, route, weights):
    what = f"profile {np.dtype(dtype).name} {route} {weights}"
    X8, y, rng = _data(zlib.crc32(what.encode()), N, P, dtype, MOVERS)
    w = rng.integers(1, 4, size=N).astype(dtype) if weights else None
    f = _make_loss("wls" if weights else "ls", dtype, X8, y, w)
    f.set_screening(False)
    f.set_gradient_cache(0)
    f.set_onchip_solve(False)
    if route == "coord":
        f.set_sweep_mode("coord")
    else:
        f.set_sweep_mode("block", route)
    om = np.full(P, 1e30)
    om[MOVERS] = 0.0
    x = cd.SparseIterate(P)
    cd.initialize_(f, x)
    st0 = f.cache_stats()
    f.profile_begin()
    cd.cdPass_(x, f, cd.ProxL1(1.0, om), np.arange(1, P + 1, dtype=np.int64))
    ms, launches, nbytes = f.profile_end()
    assert f.cache_stats()["covariance_visits"] == st0["covariance_visits"] == 0 and f.onchip_stats()["solves"] == 0
    moved = (x.dense() != 0.0).tolist()                  # visit i is coordinate i
    assert [i for i, mv in enumerate(moved) if mv] == MOVERS, what
    B = 32 if route == "coord" else route
    blocked = SP.chunk_route(route != "coord", B, weights, P)[0]
    assert blocked == (route != "coord" and (not weights or route >= 16))     # weights send a narrow block to the per-coordinate kernels
    want = SP.chunk_traffic(blocked, B, P, weights, moved, N, SP.esz(dtype))
    print(f"{what}: ms={ms:.3f} launches={launches} bytes={nbytes:.0f} model={want}")
    assert (launches, nbytes) == want, what
    assert ms > 0.0
    if blocked:
        assert launches == -(-P // B) and (P % B != 0) and any(moved[:B]) and not all(moved[:B]) \
            and any(moved[P // B * B:]) and not all(moved[P // B * B:])
    f.close()
