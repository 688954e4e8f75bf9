"""csrc/resid_state.hpp on the CPU (g++, no GPU): the move ledger against a dict-plus-list model, and the residual's state
driven through every transition against the table of LAB_NOTES.md "Residual state", with the invariants the transitions
exist to keep.  Two static checks go with it: the fields the state replaced are gone from csrc/, and every export of
include/cdhip.h that returns a status runs its body through the exception guard."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")
SO = os.path.join(HERE, "_resid_shim.so")


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "resid_shim.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("resid_state.hpp", "sparse_iterate.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", SO, src], check=True)
    L = C.CDLL(SO)
    vp, i64, f64, ci = C.c_void_p, C.c_int64, C.c_double, C.c_int
    x = [i64, vp, vp]                    # an iterate: nnz, coordinates, values
    for name, res, args in [
            ("ml_new", vp, [i64]), ("ml_free", None, [vp]), ("ml_add", None, [vp, i64, f64]), ("ml_set", None, [vp, i64, f64]),
            ("ml_clear", None, [vp]), ("ml_value", f64, [vp, i64]), ("ml_contains", ci, [vp, i64]), ("ml_empty", ci, [vp]),
            ("ml_size", i64, [vp]), ("ml_members", None, [vp, vp, vp]),
            ("rs_new", vp, [i64]), ("rs_free", None, [vp]), ("rs_stream", None, [vp, i64]), ("rs_rebuild", ci, [vp] + x),
            ("rs_demand", ci, [vp]), ("rs_set_y", None, [vp]), ("rs_generate", None, [vp]), ("rs_design_or_loss", None, [vp]),
            ("rs_iterate_loaded", None, [vp]), ("rs_iterate_moved", None, [vp]), ("rs_moved", None, [vp, i64, f64]),
            ("rs_left_lazy", None, [vp] + x), ("rs_dots_taken", None, [vp, vp, i64, ci]), ("rs_adopt", i64, [vp, vp]),
            ("rs_consistent", ci, [vp]), ("rs_lazy", ci, [vp]), ("rs_owes", ci, [vp]), ("rs_roundings", i64, [vp]),
            ("rs_skipped", i64, [vp]), ("rs_adopted", i64, [vp]), ("rs_noop", ci, [vp] + x), ("rs_can_adopt", ci, [vp, ci, i64]),
            ("rs_pending", i64, [vp, vp, vp])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def _same(a, b):
    """Equal as doubles, a NaN equal to a NaN."""
    return a == b or (a != a and b != b)


# ---- the ledger ----------------------------------------------------------------------------------------------------
def test_move_ledger_against_a_dict_and_a_list(shim):
    L, rng, p = shim, np.random.default_rng(11), 37
    m = L.ml_new(p)
    order, val = [], {}                  # the model: members in order of first insertion, their values
    out, out2 = np.zeros(p, dtype=np.int64), np.zeros(p, dtype=np.int64)
    seen = {"cancel": 0, "nan": 0, "clear": 0}
    for step in range(2500):
        u = rng.random()
        k = int(rng.integers(0, p))
        if u < 0.03:
            L.ml_clear(m)
            order, val = [], {}
            seen["clear"] += 1
        elif u < 0.55:
            if k in val and rng.random() < 0.3:
                d = -val[k]              # a move that cancels what the coordinate holds: it stays a member, at 0.0
                seen["cancel"] += d == d and d != 0.0
            elif rng.random() < 0.02:
                d = math.nan
                seen["nan"] += 1
            else:
                d = float(rng.standard_normal())
            L.ml_add(m, k, d)
            if k not in val:
                order.append(k)
                val[k] = 0.0
            val[k] += d
        else:
            v = 0.0 if rng.random() < 0.1 else float(rng.standard_normal())
            L.ml_set(m, k, v)
            if k not in val:
                order.append(k)
            val[k] = v
        assert L.ml_size(m) == len(order) and bool(L.ml_empty(m)) == (not order)
        L.ml_members(m, out.ctypes.data, out2.ctypes.data)
        assert out[:len(order)].tolist() == order and out2[:len(order)].tolist() == order
        for j in range(p):
            assert bool(L.ml_contains(m, j)) == (j in val)
            assert _same(L.ml_value(m, j), val.get(j, 0.0)), (step, j)      # non-members read 0.0: clear() left them alone,
        if not order:                                                       # ... and after it the dense array is all zero
            assert all(L.ml_value(m, j) == 0.0 for j in range(p))
    assert seen["cancel"] > 20 and seen["nan"] > 5 and seen["clear"] > 20, seen
    L.ml_free(m)


def test_move_ledger_members_that_cancel_or_hold_nan_stay_members(shim):
    L = shim
    m = L.ml_new(5)
    L.ml_add(m, 3, 1.5)
    L.ml_add(m, 1, math.nan)
    L.ml_add(m, 3, -1.5)
    L.ml_add(m, 1, 2.0)
    out, out2 = np.zeros(5, dtype=np.int64), np.zeros(5, dtype=np.int64)
    L.ml_members(m, out.ctypes.data, out2.ctypes.data)
    assert out[:2].tolist() == [3, 1] and L.ml_value(m, 3) == 0.0 and math.isnan(L.ml_value(m, 1))
    L.ml_clear(m)
    assert L.ml_empty(m) and all(L.ml_value(m, j) == 0.0 for j in range(5))
    L.ml_free(m)


# ---- the residual's state ------------------------------------------------------------------------------------------
class Model:
    """The table of LAB_NOTES.md "Residual state", one method per row, on plain Python values."""

    def __init__(self):
        self.consistent = self.lazy = self.pristine = self.dots_valid = self.dots_w = False
        self.x_lazy = self.x_pristine = ()
        self.order, self.val = [], {}
        self.stash = []
        self.roundings = self.skipped = self.adopted = 0

    def drop(self):
        self.order, self.val = [], {}

    def noop(self, x):
        return self.pristine and not self.lazy and not self.order and x == self.x_pristine

    def can_adopt(self, w, p):
        return self.dots_valid and self.dots_w == w and len(self.stash) == 2 * p

    def stream(self, launches):
        self.pristine = self.dots_valid = False
        self.roundings += launches

    def rebuild(self, x):
        if self.noop(x):
            self.roundings, self.consistent = 1, True
            self.skipped += 1
            return 1
        self.drop()
        self.lazy, self.roundings, self.consistent, self.pristine, self.x_pristine, self.dots_valid = False, 1, True, True, x, False
        return 0

    def demand(self):
        if self.lazy:
            self.lazy = False
            return 2 + self.rebuild(self.x_lazy)
        if not self.order:
            return 0
        self.pristine = False
        batches = (len(self.order) + 63) // 64
        self.roundings += batches
        self.drop()
        return -batches

    def set_y(self):
        self.consistent = self.pristine = self.dots_valid = self.lazy = False
        self.drop()

    def generate(self):
        self.pristine = self.dots_valid = self.lazy = False
        self.drop()

    def design_or_loss(self):
        self.consistent = self.pristine = self.dots_valid = False

    def moved(self, k, d):
        self.dots_valid = False
        if k not in self.val:
            self.order.append(k)
            self.val[k] = 0.0
        self.val[k] += d

    def left_lazy(self, x):
        self.dots_valid = False
        self.drop()
        self.lazy, self.x_lazy, self.consistent = True, x, True


def _xargs(x):
    idx = np.array([k for k, _ in x], dtype=np.int64)
    val = np.array([v for _, v in x], dtype=np.float64)
    return len(x), idx.ctypes.data, val.ctypes.data, (idx, val)


def test_residual_state_through_every_transition(shim):
    L, rng, p = shim, np.random.default_rng(12), 150
    s, M = L.rs_new(p), Model()
    # few iterates, so that equal ones meet; same support in another slot order or with another value is another iterate
    pool = [(), ((3, 1.0),), ((3, 1.0), (7, -2.0)), ((7, -2.0), (3, 1.0)), ((3, 1.5), (7, -2.0)), ((9, 0.25),)]
    pk, pv = np.zeros(p, dtype=np.int64), np.zeros(p)
    buf = np.zeros(2 * p)
    # what the invariants are stated in: the last event that wrote the buffer (and the iterate of a rebuild), whether X / y /
    # W / the loss changed since, whether anything was queued since, whether the residual stood for changed since dots were taken
    last_write, design_since, stood_for_since_dots, dots = None, False, True, None
    count = {}
    for step in range(3000):
        op = ["stream", "rebuild", "rebuild", "demand", "demand", "set_y", "generate", "design_or_loss", "iterate_loaded",
              "iterate_moved", "moved", "moved", "moved_many", "left_lazy", "dots_taken", "dots_taken", "adopt"][int(rng.integers(0, 17))]
        if op in ("moved", "moved_many") and M.lazy:
            op = "demand"                # (a move is never noted while r is lazy: whatever moves beta reads r or g first)
        before = dict(consistent=M.consistent, lazy=M.lazy, order=list(M.order), val=dict(M.val),
                      adopt=[M.can_adopt(w, p) for w in (False, True)])
        x = pool[int(rng.integers(0, len(pool)))]
        if op == "stream":
            n = int(rng.integers(1, 9))
            L.rs_stream(s, n)
            M.stream(n)
            last_write, stood_for_since_dots = ("stream", None), True
        elif op == "rebuild":
            a = _xargs(x)
            got = L.rs_rebuild(s, *a[:3])
            assert got == M.rebuild(x)
            if got == 0:
                last_write, design_since, stood_for_since_dots = ("rebuild", x), False, True
            else:                        # the no-op branch keeps the stash (asymmetry)
                assert [M.can_adopt(w, p) for w in (False, True)] == before["adopt"]
                count["skipped"] = count.get("skipped", 0) + 1
        elif op == "demand":
            was_lazy, xl = M.lazy, M.x_lazy
            got = L.rs_demand(s)
            assert got == M.demand()
            if got == 2:
                last_write, design_since, stood_for_since_dots = ("rebuild", xl), False, True
            elif got < 0:                # the catch-up wrote the buffer; what it stands for is the same: the stash is kept (asymmetry)
                last_write = ("catchup", None)
                assert [M.can_adopt(w, p) for w in (False, True)] == before["adopt"]
                count["batches>1"] = count.get("batches>1", 0) + (got < -1)
            count["lazy formed"] = count.get("lazy formed", 0) + (got >= 2)
            count["lazy found in the buffer"] = count.get("lazy found in the buffer", 0) + (got == 3)
            assert (got >= 2) == was_lazy
        elif op == "set_y":
            L.rs_set_y(s)
            M.set_y()
            last_write, design_since, stood_for_since_dots = ("y", None), True, True
            assert not L.rs_consistent(s)
        elif op == "generate":
            L.rs_generate(s)
            M.generate()
            last_write, design_since, stood_for_since_dots = ("generate", None), True, True
            assert bool(L.rs_consistent(s)) == before["consistent"]          # generate leaves `consistent` (asymmetry)
        elif op == "design_or_loss":
            L.rs_design_or_loss(s)
            M.design_or_loss()
            design_since, stood_for_since_dots = True, True
            assert M.order == before["order"] and M.lazy == before["lazy"]   # pending and lazy are kept (asymmetry)
            assert not L.rs_consistent(s)
        elif op == "iterate_loaded":
            L.rs_iterate_loaded(s)
            M.consistent = False
            assert [M.can_adopt(w, p) for w in (False, True)] == before["adopt"]   # consistent only: r is left alone
        elif op == "iterate_moved":
            L.rs_iterate_moved(s)
            M.dots_valid = False
            stood_for_since_dots = True
        elif op in ("moved", "moved_many"):
            for _ in range(1 if op == "moved" else int(rng.integers(60, 140))):
                k = int(rng.integers(0, p))
                d = -M.val[k] if k in M.val and rng.random() < 0.2 else math.nan if rng.random() < 0.01 else float(rng.standard_normal())
                L.rs_moved(s, k, d)
                M.moved(k, d)
            stood_for_since_dots = True
        elif op == "left_lazy":
            a = _xargs(x)
            L.rs_left_lazy(s, *a[:3])
            M.left_lazy(x)
            stood_for_since_dots = True
        elif op == "dots_taken":
            w, n = bool(rng.integers(0, 2)), 2 * p if rng.random() < 0.9 else p
            cd = rng.standard_normal(n)
            L.rs_dots_taken(s, cd.ctypes.data, n, int(w))
            M.stash, M.dots_valid, M.dots_w = cd.tolist(), True, w
            stood_for_since_dots, dots = False, (w, n)
        elif op == "adopt":
            if M.can_adopt(False, p) or M.can_adopt(True, p):
                n = L.rs_adopt(s, buf.ctypes.data)
                M.adopted += 1
                assert buf[:n].tolist() == M.stash
        count[op] = count.get(op, 0) + 1

        # ---- the state is the table's ----
        assert bool(L.rs_consistent(s)) == M.consistent and bool(L.rs_lazy(s)) == M.lazy, (step, op)
        assert L.rs_roundings(s) == M.roundings and L.rs_skipped(s) == M.skipped and L.rs_adopted(s) == M.adopted, (step, op)
        n = L.rs_pending(s, pk.ctypes.data, pv.ctypes.data)
        assert pk[:n].tolist() == M.order and all(_same(pv[i], M.val[M.order[i]]) for i in range(n)), (step, op)
        assert bool(L.rs_owes(s)) == (M.lazy or bool(M.order))
        # ---- the invariants ----
        assert not (M.lazy and M.order), (step, op)                           # lazy implies nothing pending
        for w in (False, True):
            got = bool(L.rs_can_adopt(s, int(w), p))
            assert got == M.can_adopt(w, p)
            # adoptable only if dots of the right kind and length were taken and the residual stood for has not changed since
            assert got == (not stood_for_since_dots and dots == (w, 2 * p)), (step, op, w)
        for xi in pool:
            a = _xargs(xi)
            got = bool(L.rs_noop(s, *a[:3]))
            assert got == M.noop(xi)
            # a no-op only if the buffer was last written by a rebuild from this very iterate, X / y / W / the loss have stood
            # since, and nothing is queued or left lazy
            want = last_write == ("rebuild", xi) and not design_since and not M.order and not M.lazy
            assert got == want, (step, op, xi, last_write)
    for op in ("stream", "rebuild", "demand", "set_y", "generate", "design_or_loss", "iterate_loaded", "iterate_moved", "moved",
               "moved_many", "left_lazy", "dots_taken", "adopt", "skipped", "batches>1", "lazy formed", "lazy found in the buffer"):
        assert count.get(op, 0) > 0, (op, count)
    assert M.adopted > 0
    L.rs_free(s)


# ---- static checks --------------------------------------------------------------------------------------------------
# what the handle and the gradient cache held loose before resid_state.hpp, and the helpers that wrote them
FORMER = ["r_consistent", "r_lazy", "x_lazy", "r_pristine", "x_pristine", "dots_valid", "dots_w", "dots_stash", "n_rebuild_skipped",
          "n_dots_adopted", "r_roundings", "r_pending", "r_pending_list", "r_in_pending", "dbeta", "in_moved", "touch_r",
          "drop_r_pending"]


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".h", ".cpp")):
            yield name, open(os.path.join(CSRC, name)).read()


def test_the_former_fields_are_gone_from_csrc():
    found = [(name, k) for name, txt in _sources() for k in FORMER if re.search(r"\b%s\b" % k, txt)]
    assert not found, f"fields the residual state replaced are still named in csrc/: {found}"
    # ... and nothing outside the header reaches into the state: its members are private (trailing underscore), and
    # the only spellings of them are in resid_state.hpp
    private = re.findall(r"\b([a-z_]+_)\b(?= = |;|,)", open(os.path.join(CSRC, "resid_state.hpp")).read().split("private:")[-1])
    assert {"consistent_", "lazy_", "pristine_", "dots_valid_", "dots_w_", "pending_", "stash_", "roundings_"} <= set(private)
    stray = [(name, k) for name, txt in _sources() if name != "resid_state.hpp" for k in set(private) if re.search(r"\brs\.%s\b|->rs\.%s\b" % (k, k), txt)]
    assert not stray, stray


def _status_exports():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cdhip.h")).read(), flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    return sorted(set(re.findall(r"\bint32_t\s+(cdh_[a-z_A-Z0-9]+)\s*\(", txt)))


def test_every_status_export_runs_through_the_guard():
    names = _status_exports()
    assert len(names) >= 60 and "cdh_create" in names and "cdh_last_error" not in names
    txt = open(os.path.join(CSRC, "cdhip.hip")).read()
    assert "CDH_CATCH" not in txt and not re.search(r"try\s*\{[^}]*_impl\(", txt)
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))     # (comments may say "try")
    assert len(re.findall(r"\btry\b", code)) == 1, "one try in the library: the guard's"
    bad = []
    for name in names:
        m = re.search(r"^int32_t %s\(([^{;]*)\) \{(.*)$" % name, txt, flags=re.M)
        if not m:
            bad.append((name, "no definition"))
            continue
        handle = "cdh_handle h" in m.group(1)
        if name == "cdh_create":         # frees the half-built handle after the guard: its body is the guard's all the same
            body = txt[m.end():txt.index("\n}\n", m.end())]
            ok = body.count("guarded([&]() -> int32_t {") == 1 and body.rstrip().endswith("return status;") \
                and re.search(r"^    cdh_handle h = nullptr;[^\n]*\n    const int32_t status = guarded\(", body.lstrip("\n"), flags=re.M)
        elif handle and name != "cdh_destroy":     # (cdh_destroy takes NULL, and its handle is gone when it returns)
            ok = m.group(2) == " return guarded(h, [&]() -> int32_t {"
        else:
            ok = m.group(2) == " return guarded([&]() -> int32_t {"
        if ok:                           # ... and the guard's lambda closes the definition
            end = txt.index("\n}", m.end())
            ok = name == "cdh_create" or txt[end:end + 6] == "\n}); }"
        if not ok:
            bad.append((name, m.group(2)[:60]))
    assert not bad, bad
