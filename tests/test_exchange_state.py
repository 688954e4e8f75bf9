"""csrc/exchange_state.hpp on the CPU (g++, no GPU): who serves a row shard, where an all-reduce goes, the epochs of the
direct exchange and the capture bookkeeping, against the rules as they stood in csrc/cdhip.hip before the struct existed
(commit 5bc4a7c; the line numbers in the comments below are that file's).  The oracle is that restatement -- the same
five flags, the same `if` ladders, the three epoch rules -- never the struct.  Static checks go with it: the handle
fields the struct replaced are gone from csrc/, and graph executables and the epoch constants have one home each."""
import ctypes as C
import os
import random
import re
import subprocess
from collections import Counter, deque

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "coordinatedescent.jl_amd", "csrc")
SO = os.path.join(HERE, "_exchange_shim.so")

OK, BAD_ARG, RCCL_ERROR = 0, 2, 5
HOST, DIRECT, RCCL, NOTHING, REFUSE = range(5)
MAXC, MAXR = 2688, 8                     # kP2PMaxCount, kP2PMaxRanks (asserted against the header's below)
WRAP, SOFT = 0xfffffff0, 0xf0000000      # kEpochWrap, kEpochSoftWrap (likewise)
COUNTS = (1, 4, MAXC, MAXC + 1, 2 * MAXC + 1)


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "exchange_shim.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("exchange_state.hpp", "p2p_limits.hpp")] + [os.path.join(ROOT, "include", "cdhip.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", SO, src], check=True)
    L = C.CDLL(SO)
    vp, i32, u32, u64, ci = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_int
    for name, res, args in [
            ("xs_new", vp, []), ("xs_free", None, [vp]), ("xs_msg", C.c_char_p, [vp]), ("xs_max_count", ci, []), ("xs_max_ranks", ci, []),
            ("xs_epoch_wrap", u32, []), ("xs_epoch_soft_wrap", u32, []),
            ("xs_comm_init", i32, [vp, ci, ci, ci]), ("xs_comm_drop", i32, [vp]), ("xs_p2p_local_handle", i32, [vp]),
            ("xs_p2p_connect", i32, [vp, ci, ci]), ("xs_p2p_enable", i32, [vp, ci]), ("xs_raise_timeout_flag", None, [vp]),
            ("xs_p2p_check", i32, [vp]), ("xs_host_set", i32, [vp, ci, ci, ci]), ("xs_capture_begins", None, [vp]),
            ("xs_capture_ends_and_replays", None, [vp, vp]), ("xs_allreduce", i32, [vp, u64]),
            ("xs_sharded", ci, [vp]), ("xs_alive", i32, [vp]), ("xs_route", ci, [vp, u64]), ("xs_route_status", i32, [vp, u64]),
            ("xs_route_hands_back_what_was_installed", ci, [vp]), ("xs_may_capture", ci, [vp]), ("xs_graph_key_bits", u32, [vp]),
            ("xs_reported_ranks", ci, [vp]), ("xs_rank", ci, [vp]), ("xs_nranks", ci, [vp]), ("xs_counters", None, [vp, vp]),
            ("xs_seed_epoch", None, [vp, u32]), ("xs_last_epoch", u32, [vp]), ("xs_chunk", None, [vp, u32, ci, u32, vp])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    assert (L.xs_max_count(), L.xs_max_ranks(), L.xs_epoch_wrap(), L.xs_epoch_soft_wrap()) == (MAXC, MAXR, WRAP, SOFT)
    return L


# ---- the parent's rules, restated ----------------------------------------------------------------------------------
M_HOST = "the handle already exchanges through a host transport"
M_RANKS = "bad rank / nranks"
M_P2P_RANKS = "p2p exchange: bad rank / nranks (at most 8 ranks)"
M_NO_INBOX = "cdh_p2p_local_handle must be called first"
M_DIFFER = "p2p exchange: rank / nranks differ from the RCCL communicator's"
M_CONNECTED = "p2p exchange is already connected"
M_NOT_CONNECTED = "p2p exchange is not connected"
M_STAYS_OFF = "p2p exchange timed out earlier on this handle; it stays off"
M_HAS_EXCHANGE = "the handle already has an exchange (RCCL / direct)"
M_TIMED_OUT = "p2p exchange timed out waiting for a peer (rank died, or ranks ran different sweeps)"
M_DEAD = "the shard lost its exchange (p2p timed out earlier); rebuild the handle"
M_LOST = "the shard's host exchange was removed and nothing replaced it: its sums would cover local rows only"
M_NO_CAPTURE = "the host-staged exchange cannot be recorded in a graph"
MESSAGES = [M_HOST, M_RANKS, M_P2P_RANKS, M_NO_INBOX, M_DIFFER, M_CONNECTED, M_NOT_CONNECTED, M_STAYS_OFF, M_HAS_EXCHANGE,
            M_TIMED_OUT, M_DEAD, M_LOST, M_NO_CAPTURE]


class Parent:
    """cdh_handle_s's exchange fields (cdhip.hip:338-357) and the code that read and wrote them."""

    def __init__(self):
        self.comm = self.p2p_on = self.p2p_dead = self.lost_exchange = self.host_fn = False      # the five flags
        self.rank, self.nranks, self.p2p_ranks = 0, 1, 0
        self.inbox = self.flag = False           # h->p2p_inbox exists; *h->p2p_timeout
        self.capturing, self.cap_exchanges, self.cap_rccl = False, 0, 0
        self.n_rccl = self.n_p2p = self.n_host = 0
        self.epoch = 0

    def key(self):
        return (self.comm, self.rank, self.nranks, self.p2p_ranks, self.p2p_on, self.p2p_dead, self.lost_exchange, self.host_fn,
                self.inbox, self.flag)

    def sharded(self):                           # :421-423
        return self.comm or self.p2p_on or self.p2p_dead or self.lost_exchange or self.host_fn

    def alive(self):                             # exchange_alive, :427-431
        if self.p2p_dead:
            return RCCL_ERROR, M_DEAD
        if self.lost_exchange:
            return RCCL_ERROR, M_LOST
        return OK, None

    def p2p_check(self):                         # :433-443
        if self.p2p_on and self.flag:
            self.p2p_on, self.p2p_dead = False, True
            return RCCL_ERROR, M_TIMED_OUT
        return OK, None

    def route(self, count):                      # the ladder of allreduce, :468-504, without its side effects
        if self.host_fn:                         # :469
            return (REFUSE, BAD_ARG, M_NO_CAPTURE) if self.capturing else (HOST, OK, None)      # :470
        if self.p2p_on and (count <= MAXC or not self.comm):      # :483
            return DIRECT, OK, None
        st, msg = self.alive()                   # :494
        if st != OK:
            return REFUSE, st, msg
        return (RCCL, OK, None) if self.comm else (NOTHING, OK, None)      # :495-496

    def allreduce(self, count):                  # :468-504 with them
        where, st, msg = self.route(count)
        if where == REFUSE:
            return st, msg
        if where == HOST:
            self.n_host += 1                     # :480
        elif where == DIRECT:
            st, msg = self.p2p_check()           # :484
            if st != OK:
                return st, msg
            for _ in range(0, count, MAXC):      # :485-490
                self.next_p2p_call()
                if not self.capturing:
                    self.n_p2p += 1
        elif where == RCCL:
            if self.capturing:                   # :502
                self.cap_rccl += 1
            else:
                self.n_rccl += 1
        return OK, None

    def may_capture(self):                       # run_chunk, :931
        return not self.host_fn and not self.p2p_dead

    def key_bits(self):                          # :933
        return (32 if self.comm else 0) | (16 if self.p2p_on else 0)

    def reported_ranks(self):                    # cdh_exchange_stats, :2308-2316 (ncclCommCount aside)
        return self.nranks if self.comm else self.p2p_ranks if self.p2p_on else self.nranks if self.host_fn else 1

    # -- the exports --
    def comm_init(self, rank, nranks, force):    # :2193-2212
        if self.host_fn:
            return BAD_ARG, M_HOST
        if nranks < 1 or rank < 0 or rank >= nranks:
            return BAD_ARG, M_RANKS
        if nranks == 1 and not force:            # :2198
            self.rank, self.nranks = 0, 1
            return OK, None
        self.comm, self.rank, self.nranks, self.lost_exchange = True, rank, nranks, False
        return OK, None

    def comm_drop(self):                         # :2214-2224
        if not self.comm:
            return OK, None
        self.comm = False
        if self.nranks > 1 and not self.p2p_on and not self.host_fn:      # :2222
            self.lost_exchange = True
        return OK, None

    def local_handle(self):                      # :2227-2248
        self.inbox = True
        return OK, None

    def connect(self, rank, nranks):             # :2250-2271
        if self.host_fn:
            return BAD_ARG, M_HOST
        if nranks < 1 or nranks > MAXR or rank < 0 or rank >= nranks:
            return BAD_ARG, M_P2P_RANKS
        if not self.inbox:
            return BAD_ARG, M_NO_INBOX
        if self.comm and (rank != self.rank or nranks != self.nranks):
            return BAD_ARG, M_DIFFER
        if self.p2p_ranks:
            return BAD_ARG, M_CONNECTED
        self.rank, self.nranks, self.p2p_ranks = rank, nranks, nranks
        return OK, None

    def enable(self, on):                        # :2273-2280
        if on and not self.p2p_ranks:
            return BAD_ARG, M_NOT_CONNECTED
        if on and self.flag:
            return RCCL_ERROR, M_STAYS_OFF
        self.p2p_on = bool(on)
        if self.p2p_on:
            self.lost_exchange = False
        return OK, None

    def raise_flag(self):                        # p2p_exchange_value's bounded spin: only a running direct exchange writes it
        if self.p2p_on:
            self.flag = True

    def host_set(self, install, rank, nranks):   # :2282-2300
        if not install:
            if self.host_fn and self.nranks > 1 and not self.comm and not self.p2p_ranks:      # :2285
                self.lost_exchange = True
            self.host_fn = False
            return OK, None
        if nranks < 1 or rank < 0 or rank >= nranks:
            return BAD_ARG, M_RANKS
        if self.comm or self.p2p_ranks:
            return BAD_ARG, M_HAS_EXCHANGE
        self.host_fn, self.rank, self.nranks, self.lost_exchange = True, rank, nranks, False
        return OK, None

    def capture_begins(self):                    # :940
        self.capturing, self.cap_exchanges, self.cap_rccl = True, 0, 0

    def capture_ends_and_replays(self):          # :944, :955, :960-967
        self.capturing = False
        ex, rc = self.cap_exchanges, self.cap_rccl
        if ex:
            self.replay(ex)
            self.n_p2p += ex
        self.n_rccl += rc
        return ex, rc

    # -- the three epoch rules --
    def next_p2p_call(self):                     # :456-463 with epoch_after, :453
        if self.capturing:
            self.cap_exchanges += 1
            return self.cap_exchanges
        e = self.epoch
        self.epoch = (2 if e & 1 else 3) if e >= WRAP else e + 1
        return self.epoch

    def chunk_begins(self):                      # :901
        if self.epoch >= SOFT:
            self.epoch = 1 if self.epoch & 1 else 2

    def replay(self, k):                         # :962-964; returns the base
        if self.epoch + k >= WRAP:
            self.epoch = 1 if self.epoch & 1 else 2
        base = self.epoch
        self.epoch += k
        return base


# an operation: (name, arguments); applied to the model and to the struct alike
def _apply(L, s, M, op):
    """-> (status, message) of the model and of the struct."""
    name, a = op[0], op[1:]
    if name == "comm_init":
        got, want = L.xs_comm_init(s, *a), M.comm_init(*a)
    elif name == "comm_drop":
        got, want = L.xs_comm_drop(s), M.comm_drop()
    elif name == "local_handle":
        got, want = L.xs_p2p_local_handle(s), M.local_handle()
    elif name == "connect":
        got, want = L.xs_p2p_connect(s, *a), M.connect(*a)
    elif name == "enable":
        got, want = L.xs_p2p_enable(s, *a), M.enable(*a)
    elif name == "timeout":              # the flag goes up, and the host finds it (finish_chunk's p2p_check)
        L.xs_raise_timeout_flag(s)
        M.raise_flag()
        got, want = L.xs_p2p_check(s), M.p2p_check()
    elif name == "host":
        got, want = L.xs_host_set(s, *a), M.host_set(*a)
    elif name == "capture_begin":
        L.xs_capture_begins(s)
        M.capture_begins()
        got, want = OK, (OK, None)
    elif name == "capture_end":
        out = (C.c_uint32 * 2)()
        L.xs_capture_ends_and_replays(s, out)
        assert (out[0], out[1]) == M.capture_ends_and_replays()
        got, want = OK, (OK, None)
    elif name == "allreduce":
        got, want = L.xs_allreduce(s, *a), M.allreduce(*a)
    else:
        raise AssertionError(name)
    return want, (got, L.xs_msg(s).decode() if got != OK else None)


def _compare(L, s, M, tally=None):
    """Every question the struct answers, against the model."""
    assert bool(L.xs_sharded(s)) == bool(M.sharded())
    st = L.xs_alive(s)
    assert (st, L.xs_msg(s).decode() if st else None) == M.alive()
    for count in COUNTS:
        where, st, msg = M.route(count)
        assert L.xs_route(s, count) == where and L.xs_route_status(s, count) == st, (count, where)
        if where == REFUSE:
            assert L.xs_msg(s).decode() == msg
        if tally is not None:
            tally["route", where] += 1
            if msg:
                tally[msg] += 1
    assert bool(L.xs_may_capture(s)) == M.may_capture() and L.xs_graph_key_bits(s) == M.key_bits()
    assert L.xs_reported_ranks(s) == M.reported_ranks() and (L.xs_rank(s), L.xs_nranks(s)) == (M.rank, M.nranks)
    out = (C.c_int64 * 3)()
    L.xs_counters(s, out)
    assert list(out) == [M.n_rccl, M.n_p2p, M.n_host]
    assert L.xs_last_epoch(s) == M.epoch and L.xs_route_hands_back_what_was_installed(s)


def _random_op(rng, M):
    u = rng.random()
    ranks = lambda: (rng.choice([0, 0, 1, 1, 7, -1, 2]), rng.choice([1, 2, 2, 8, 8, 0, 9]))      # mismatches and bad pairs too
    if u < 0.12:
        r, n = ranks()
        return ("comm_init", r, n, int(rng.random() < 0.3))
    if u < 0.20:
        return ("comm_drop",)
    if u < 0.27:
        return ("local_handle",)
    if u < 0.39:
        # half the time what the communicator has, so that a connect next to RCCL goes through
        return ("connect", M.rank, M.nranks) if rng.random() < 0.5 else ("connect",) + ranks()
    if u < 0.51:
        return ("enable", int(rng.random() < 0.7))
    if u < 0.55:
        return ("timeout",)
    if u < 0.66:
        return ("host", 0, 0, 0) if rng.random() < 0.4 else ("host", 1) + ranks()
    if u < 0.71:
        return ("capture_begin",)
    if u < 0.78:
        return ("capture_end",)
    return ("allreduce", rng.choice(COUNTS))


# ---- 1. transport state against the parent's rules ------------------------------------------------------------------
def test_transport_state_against_the_parents_rules(shim):
    L, rng, tally, checks = shim, random.Random(20261018), Counter(), 0
    for seq in range(2000):
        s, M = L.xs_new(), Parent()
        for step in range(40):
            op = _random_op(rng, M)
            want, got = _apply(L, s, M, op)
            assert got == want, (seq, step, op)
            if want[1]:
                tally[want[1]] += 1
            _compare(L, s, M, tally)
            checks += len(COUNTS)
        L.xs_free(s)
    # a generator that never reaches a state cannot hide it: every route in at least 1 % of the checks, every refusal once
    for where in (HOST, DIRECT, RCCL, NOTHING, REFUSE):
        assert tally["route", where] >= checks // 100, (where, tally["route", where], checks)
    for msg in MESSAGES:
        assert tally[msg] > 0, msg
    # the counters moved, and calls made while capturing were counted at the replay (the model says when)
    assert checks == 2000 * 40 * len(COUNTS)


# ---- 2. every reachable state where nranks > 1 and sharded() is false --------------------------------------------
def _all_ops():
    pairs = [(r, n) for n in (1, 2, 8) for r in (0, 1) if r < n]
    ops = [("comm_drop",), ("local_handle",), ("enable", 0), ("enable", 1), ("timeout",), ("host", 0, 0, 0)]
    ops += [("comm_init", r, n, f) for r, n in pairs for f in (0, 1)]
    ops += [("connect", r, n) for r, n in pairs] + [("host", 1, r, n) for r, n in pairs]
    return ops


def _walk():
    """Breadth-first over the model from a fresh handle: state -> the shortest list of operations that reaches it."""
    import copy
    start = Parent()
    paths, todo = {start.key(): []}, deque([start])
    while todo:
        M = todo.popleft()
        for op in _all_ops():
            N = copy.copy(M)
            getattr(N, {"host": "host_set", "timeout": "raise_flag"}.get(op[0], op[0]))(*op[1:])
            if op[0] == "timeout":
                N.p2p_check()
            if N.key() not in paths:
                paths[N.key()] = paths[M.key()] + [op]
                todo.append(N)
    return paths


def _replayed(path):
    M = Parent()
    for op in path:
        getattr(M, {"host": "host_set", "timeout": "raise_flag"}.get(op[0], op[0]))(*op[1:])
        if op[0] == "timeout":
            M.p2p_check()
    return M


# (communicator, direct exchange connected, on, dead, lost_exchange, host transport) of a handle that has nranks > 1 and is
# not sharded(): its all-reduces do nothing and its sums cover local rows only.  One field state, reached two ways: between
# cdh_p2p_connect and the first cdh_p2p_enable(h, 1), and after cdh_p2p_enable(h, 0) -- also where an RCCL communicator
# was dropped while the direct exchange was on.  Kept as it is (LAB_NOTES.md "Exchange state: open questions").
UNSERVED = {(False, True, False, False, False, False)}


def test_every_reachable_state_of_a_shard_that_nothing_serves(shim):
    L = shim
    paths = _walk()
    assert 100 < len(paths) < 5000, len(paths)
    unserved, told_apart_in_drop, told_apart_in_remove = set(), 0, 0
    for key, path in paths.items():
        s, M = L.xs_new(), Parent()
        for op in path:
            want, got = _apply(L, s, M, op)
            assert got == want, (path, op)
        assert M.key() == key
        _compare(L, s, M)                        # the struct agrees state for state
        if M.nranks > 1 and not M.sharded():
            assert not L.xs_sharded(s) and L.xs_nranks(s) > 1
            assert all(L.xs_route(s, c) == NOTHING for c in COUNTS)      # ... and quietly does nothing
            unserved.add((M.comm, M.p2p_ranks > 0, M.p2p_on, M.p2p_dead, M.lost_exchange, M.host_fn))
        # the two lost_exchange conditions (cdh_comm_drop: !p2p_on; removing the host transport: !p2p_ranks) differ where
        # the direct exchange is connected and off
        if M.p2p_ranks and not M.p2p_on and M.nranks > 1:
            told_apart_in_drop += bool(M.comm)           # a drop here marks the shard lost; with !p2p_ranks it would not
            told_apart_in_remove += bool(M.host_fn)      # a removal here does not; with !p2p_on it would
        L.xs_free(s)
    assert unserved == UNSERVED
    # the two ways the issue names
    for path in ([("local_handle",), ("connect", 0, 2)], [("local_handle",), ("connect", 1, 2), ("enable", 1), ("enable", 0)]):
        M = _replayed(path)
        assert M.nranks > 1 and not M.sharded() and M.route(4)[0] == NOTHING
    # reachable states tell the two conditions apart in cdh_comm_drop only: a host transport and a connected direct
    # exchange never meet (each install refuses the other)
    assert told_apart_in_drop > 0 and told_apart_in_remove == 0
    # cdh_comm_init with one rank and no CDH_FORCE_RCCL leaves lost_exchange alone: a lost shard stays lost, now with nranks == 1
    M = _replayed([("host", 1, 0, 2), ("host", 0, 0, 0), ("comm_init", 0, 1, 0)])
    assert M.lost_exchange and M.nranks == 1 and M.route(4) == (REFUSE, RCCL_ERROR, M_LOST)


# ---- 3. epochs ----------------------------------------------------------------------------------------------------
# What makes the rules hold: a chunk issues fewer than kEpochWrap - kEpochSoftWrap = 2^28 - 16 exchanges, so a chunk that
# starts below the soft wrap never reaches the hard one.  The largest chunk here is 2^20.
CHUNK_BOUND = WRAP - SOFT
SIZES = (1, 2, 3, 7, 64, 1000, 1 << 20)
STARTS = [0, 1, 2, 3] + [SOFT + d for d in (-2, -1, 0, 1)] + [WRAP + d for d in (-3, -2, -1, 0, 1)] + [0xfffffffe, 0xffffffff]


def _connected(L, rank):
    s = L.xs_new()
    assert (L.xs_p2p_local_handle(s), L.xs_p2p_connect(s, rank, 2), L.xs_p2p_enable(s, 1)) == (OK, OK, OK)
    return s


def _model_chunk(M, k):
    """The parent's node-by-node chunk: (first, last, epochs that are not their predecessor + 1)."""
    M.chunk_begins()
    first, breaks, prev = None, 0, None
    while k:
        if prev is not None and M.epoch + k < WRAP:      # epoch_after below the wrap is + 1, k times: no need to count them out
            M.epoch += k
            break
        e = M.next_p2p_call()
        first = e if first is None else first
        breaks += prev is not None and e != prev + 1
        prev, k = e, k - 1
    return first, M.epoch, breaks


def test_epochs_alternate_slots_and_keep_two_paths_in_step(shim):
    L, rng = shim, random.Random(3)
    assert max(SIZES) < CHUNK_BOUND == 2 ** 28 - 16
    out = (C.c_uint64 * 8)()
    chunks = Counter()
    for start in STARTS:
        for seq in range(300):
            a, b = _connected(L, 0), _connected(L, 1)        # a launches every chunk node by node, b replays every chunk
            M = Parent()
            M.inbox, M.p2p_ranks, M.nranks, M.p2p_on, M.epoch = True, 2, 2, True, start
            L.xs_seed_epoch(a, start)
            L.xs_seed_epoch(b, start)
            prev, recorded = start, set()                    # the epoch issued last (0: none yet); graph sizes b has captured
            for step in range(60):
                # The largest size costs 2^20 calls on rank a, so it is drawn where it can matter and rarely elsewhere: a
                # start near a wrap is met in a sequence's first steps (after a wrap the epochs are small, and 60 chunks of
                # 2^20 come nowhere near the next one).  Sequences 0, 1, 2 of every start take it as their first, second,
                # third step; every eighth sequence draws it like any other size in its first three steps; later steps
                # one time in 1000.
                if step == seq < 3:
                    k = SIZES[-1]
                elif rng.random() < 0.3:
                    k = 0
                elif step < 3 and seq % 8 == 0:
                    k = rng.choice(SIZES)
                else:
                    k = SIZES[-1] if rng.random() < 0.001 else rng.choice(SIZES[:-1])
                chunks[k] += 1
                if k == 0:               # a loose exchange (the column dots of lambda_max, say): node by node on both ranks
                    want = M.allreduce(4)
                    assert want == (OK, None) and L.xs_allreduce(a, 4) == OK and L.xs_allreduce(b, 4) == OK
                    assert L.xs_last_epoch(a) == M.epoch
                    assert M.epoch != 0 and (prev == 0 or (M.epoch ^ prev) & 1)
                else:
                    first, last, breaks = _model_chunk(M, k)
                    L.xs_chunk(a, k, 0, prev, out)
                    # every issued epoch equals the parent model's: the first, the last, the count and the number of places
                    # where the run is broken pin all k of them
                    assert out[:5] == [OK, first, last, k, breaks], (start, seq, step, k, list(out))
                    assert out[5] == 0 and out[6] == 0       # none is 0; no two in a row share a slot
                    if k not in recorded:                    # b's first chunk of this size records it: positions 1 .. k
                        L.xs_chunk(b, k, 1, 0, out)
                        assert out[:5] == [OK, 1, k, k, 0] and out[7] == k
                        recorded.add(k)
                    L.xs_chunk(b, k, 2, prev, out)
                    base = out[7]
                    assert (out[1], out[2], out[3], out[4]) == (base + 1, base + k, k, 0) and base + k < 2 ** 32
                    assert (out[1], out[2]) == (first, last) and breaks == 0 and out[5] == 0 and out[6] == 0
                prev = M.epoch
                # the two ranks hold the same epoch after every step, the model's
                assert L.xs_last_epoch(a) == L.xs_last_epoch(b) == M.epoch, (start, seq, step, k)
            ca, cb = (C.c_int64 * 3)(), (C.c_int64 * 3)()
            L.xs_counters(a, ca)
            L.xs_counters(b, cb)
            assert list(ca) == list(cb) == [0, ca[1], 0] and ca[1] > 0      # counted call for call on both paths
            L.xs_free(a)
            L.xs_free(b)
    assert all(chunks[k] > 100 for k in SIZES + (0,)), chunks


# ---- 4. static checks ----------------------------------------------------------------------------------------------
# the handle fields the struct replaced.  The first three are everyday words (kernels have a `rank` of their own): they
# are looked for as members of the handle; the rest must not be spelled at all
FORMER_MEMBERS = ["comm", "rank", "nranks"]
FORMER = ["p2p_ranks", "p2p_on", "p2p_dead", "lost_exchange", "host_fn", "host_user", "p2p_epoch", "capturing", "cap_exchanges",
          "cap_rccl", "n_rccl_calls", "n_p2p_calls", "n_host_calls", "epoch_after"]


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".h", ".cpp")):
            yield name, open(os.path.join(CSRC, name)).read()


def test_the_former_exchange_fields_are_gone_from_csrc():
    found = [(name, k) for name, txt in _sources() if name != "exchange_state.hpp" for k in FORMER if re.search(r"\b%s\b" % k, txt)]
    found += [(name, k) for name, txt in _sources() if name != "exchange_state.hpp" for k in FORMER_MEMBERS
              if re.search(r"\bh->%s\b|\bh\.%s\b" % (k, k), txt)]
    assert not found, f"fields the exchange state replaced are still named in csrc/: {found}"
    # nothing outside the header reaches into the state: its members are private (trailing underscore)
    hdr = open(os.path.join(CSRC, "exchange_state.hpp")).read()
    private = set(re.findall(r"\b([a-z0-9_]+_)\b(?= = |;|,)", hdr.split("private:")[-1]))
    assert {k + "_" for k in FORMER[:-1] if k != "p2p_epoch"} | {"comm_", "rank_", "nranks_", "epoch_"} <= private
    stray = [(name, k) for name, txt in _sources() if name != "exchange_state.hpp" for k in private if re.search(r"\bxs\.%s\b" % k, txt)]
    assert not stray, stray
    # host only: nothing from HIP
    assert "hip" not in re.sub(r"//[^\n]*", "", hdr).replace("cdhip.h", "").lower()


def test_graph_executables_and_epoch_constants_have_one_home():
    txt = open(os.path.join(CSRC, "cdhip.hip")).read()
    owner = re.search(r"^class GraphCache \{.*?^\};", txt, flags=re.S | re.M)
    assert owner and owner.group(0).count("hipGraphExecDestroy") == 2          # insert's eviction, clear()
    for name, src in _sources():
        rest = src.replace(owner.group(0), "") if name == "cdhip.hip" else src
        assert "hipGraphExecDestroy" not in rest, name
        if name != "exchange_state.hpp":
            assert "kEpochWrap" not in src and "kEpochSoftWrap" not in src, name
    # the two sizes the struct shares with the kernels are defined once
    for k in ("kP2PMaxCount", "kP2PMaxRanks"):
        assert [name for name, src in _sources() if re.search(r"constexpr int %s\b" % k, src)] == ["p2p_limits.hpp"]
