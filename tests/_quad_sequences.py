"""Seeded sequences of operations on one CDQuadraticLoss handle, mirrored on one oracle loss and iterate per problem
(tests/test_gpu_quad_batch.py runs them on the device; tests/test_quad_sequences_host.py runs the oracle's side alone, which is
where the generator's own guarantees -- every solve converges, nothing is skipped -- are checked without a GPU)."""
import numpy as np

import coordinatedescent_jl_amd as cd
import oracle as O
from _quad_cases import BETA_TOL, H_TOL, OPT, _A, _b, _grad_bar, _oracle_gradient, _same

P_S, MAXB = 70, 6
OPS = ("set_b", "warm", "cold", "edit", "init", "descend", "pass", "gradient", "lmax", "penalty")


class _Mirror:
    """One handle and, per problem, the oracle's loss and iterate; every operation goes to both."""

    def __init__(self, rng, device):
        self.rng, self.device, self.f = rng, device, None
        self.load(int(rng.integers(1, MAXB + 1)))

    def load(self, m):
        rng = self.rng
        self.m = m
        self.B = np.stack([_b(P_S, int(rng.integers(1 << 20)), s=1 + int(rng.integers(9))) for _ in range(m)], axis=1)
        if self.device:
            if self.f is None:
                self.f = cd.CDQuadraticLoss(_A(P_S), self.B, max_batch=MAXB)
            else:
                self.f.set_b(self.B)
        self.fos = [O.CDQuadraticLoss(_A(P_S), self.B[:, j].copy()) for j in range(m)]
        self.xs = [cd.SparseIterate(P_S) for _ in range(m)]
        self.xos = [O.SparseIterate(P_S) for _ in range(m)]
        self.oms = [None] * m
        self.lams = [0.0] * m
        for j in range(m):
            self.draw_lambda(j)

    def draw_lambda(self, j):
        """lambda_j in [0.05, 0.9] lambda_max of problem j under its omega: every solve converges within maxIter."""
        om = 1.0 if self.oms[j] is None else self.oms[j]
        self.lams[j] = float(self.rng.uniform(0.05, 0.9)) * float((np.abs(self.B[:, j]) / om).max())

    def pen(self, j):
        return cd.ProxL1(self.lams[j], self.oms[j]), O.ProxL1(self.lams[j], self.oms[j])

    def solve(self, warm):
        rng = self.rng
        o = dict(OPT, warmStart=warm, randomize=bool(rng.integers(2)), seed=int(rng.integers(100)), numSteps=int(rng.integers(1, 10)))
        if self.device:
            cd.coordinateDescent_(self.xs, self.f, [self.pen(j)[0] for j in range(self.m)], cd.CDOptions(**o))
        for j in range(self.m):
            st = O.coordinateDescent_(self.xos[j], self.fos[j], self.pen(j)[1], O.CDOptions(**o))
            assert st["converged"], ("the oracle's own solve did not converge", j, o)
            if self.device:
                _same(self.f.last_stats[j], self.xs[j], st, self.xos[j], tag=j)
                if not warm:
                    om = 1.0 if self.oms[j] is None else self.oms[j]
                    np.testing.assert_allclose(self.f.last_stats[j]["lambda_max"], (np.abs(self.B[:, j]) / om).max(), rtol=1e-15)

    def step(self, op):
        rng, f = self.rng, self.f
        j = int(rng.integers(self.m))
        k = int(rng.integers(1, P_S + 1))
        if op == "set_b":
            self.load(int(rng.integers(1, MAXB + 1)))
        elif op in ("warm", "cold"):
            self.solve(op == "warm")
        elif op == "edit":
            for kk in rng.integers(1, P_S + 1, size=int(rng.integers(1, 7))).tolist():
                v = 0.0 if rng.random() < 0.4 else float(rng.standard_normal())
                self.xs[j][kk] = v
                self.xos[j][kk] = v
        elif op == "init":                                   # (the handle's initialize! recomputes every problem's A x: so do we)
            for i in range(self.m):
                if self.device:
                    cd.initialize_(f, self.xs[i], problem=i)
                O.initialize_(self.fos[i], self.xos[i])
        elif op == "penalty":                                # the next drawn operation is the first to use it
            kind = ("lambda", "add", "drop")[int(rng.integers(3))]
            if kind == "add":
                self.oms[j] = rng.random(P_S) + 0.5
            elif kind == "drop":
                self.oms[j] = None
            self.draw_lambda(j)
        elif op == "descend":
            g, go = self.pen(j)
            ho = O.descendCoordinate_(self.fos[j], go, self.xos[j], k)
            if self.device:
                h = cd.descendCoordinate_(f, g, self.xs[j], k, problem=j)
                assert abs(h - ho) <= H_TOL, (h, ho)
        elif op == "pass":
            lst = rng.integers(1, P_S + 1, size=int(rng.integers(2, 100))).tolist()
            lst += lst[: 1 + len(lst) // 3]                  # repeats, whatever the draw
            g, go = self.pen(j)
            mho = O.cdPass_(self.xos[j], self.fos[j], go, lst)
            if self.device:
                mh = cd.cdPass_(self.xs[j], f, g, lst, problem=j)
                assert abs(mh - mho) <= H_TOL, (mh, mho)
        elif op == "gradient":
            ref = O.gradient(self.fos[j], self.xos[j], k)
            if self.device:
                assert abs(cd.gradient(f, self.xs[j], k, problem=j) - ref) <= _grad_bar(self.B[:, j])
        elif op == "lmax":
            g, go = self.pen(j)
            ref = O.findLambdaMax(self.xos[j], self.fos[j], go)
            if self.device:
                np.testing.assert_allclose(cd.findLambdaMax(self.xs[j], f, g, problem=j), ref, rtol=1e-12)
        if op != "edit":                                     # (an edit is on the host alone until the next call that takes x_j)
            self.compare()

    def compare(self):
        if not self.device:
            return
        assert self.f.m == self.m
        for j in range(self.m):
            x, xo = self.xs[j], self.xos[j]
            np.testing.assert_allclose(x.dense(), xo.dense(), rtol=0, atol=BETA_TOL, err_msg=str(j))
            assert x.nzval2ind.tolist() == xo.nzval2ind.tolist(), j
            np.testing.assert_allclose(self.f._gradient_vector(j), _oracle_gradient(self.fos[j]), rtol=0,
                                       atol=_grad_bar(self.B[:, j]), err_msg=str(j))


def _run_sequence(seed, device=True):
    """12 to 15 operations drawn from the seed alone (no draw depends on a result); returns the operations run, by name.
    Nothing can be skipped: every operation is defined in every state, and lambda is drawn where the oracle's solve
    converges (asserted on the oracle's side in `solve`).  device=False runs the oracle's side alone."""
    rng = np.random.default_rng(7000 + seed)
    mir = _Mirror(rng, device)
    ran = []
    try:
        for step in range(int(rng.integers(12, 16))):
            op = OPS[int(rng.integers(len(OPS)))]
            ran.append(op)
            try:
                mir.step(op)
            except AssertionError as e:
                raise AssertionError(f"seed {seed}, step {step} ({op}, m = {mir.m}): {e}") from e
    finally:
        if mir.f is not None:
            mir.f.close()
    return ran
