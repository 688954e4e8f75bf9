// Stand-alone program over csrc/cache_state.hpp for the host sanitizers (tests/test_cache_state.py builds it with
// -fsanitize=address,undefined and runs it): one fixed sequence through every transition, the answers checked on the way.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "../coordinatedescent.jl_amd/csrc/cache_state.hpp"

using cdh::CacheState;
using cdh::MoveKind;
using cdh::SupportList;

#define REQUIRE(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const int64_t p = 5;
    const double nan = std::nan("");
    CacheState st;
    REQUIRE(!st.sized() && !st.valid() && !st.tracks_r() && st.host_g_current() && !st.dev_g_current() && st.table_void());
    SupportList x(p);
    x.set(1, 2.0); x.set(3, -1.0);
    st.rebuilt(x, p);                                    // never sized: nothing happens
    st.invalidated(true);
    REQUIRE(!st.sized() && !st.beta_known() && st.moved().empty());
    REQUIRE(!st.moved(2, 1.0, MoveKind::streamed));      // tracks nothing: the chunk has nothing to tell
    st.size(p, true, x);
    REQUIRE(st.sized() && st.beta_known() && st.beta_ref()[1] == 2.0 && st.beta_ref()[3] == -1.0 && st.tracks_r());
    st.mirrors_allocated();
    st.referenced(st.beta_known());
    REQUIRE(st.valid() && st.beta_known() && st.host_g_current() && !st.dev_g_current() && st.cov_since_ref() == 0);
    // moves of each kind; the ledger keeps the order of first arrival, a cancelled member stays
    REQUIRE(st.moved(3, 0.5, MoveKind::streamed) && st.moved(0, 1.0, MoveKind::streamed) && st.moved(3, -0.5, MoveKind::streamed));
    REQUIRE(st.moved().size() == 2 && st.moved()[0] == 3 && st.moved()[1] == 0 && st.moved().value(3) == 0.0 && st.beta_ref()[3] == -1.0);
    st.moved(4, 2.0, MoveKind::carried, false);
    REQUIRE(st.moved().size() == 2 && st.beta_ref()[4] == 2.0);
    st.moved(4, nan, MoveKind::carried, false);
    REQUIRE(st.beta_ref()[4] == 2.0 && st.valid());
    st.moved(2, 1.5, MoveKind::off_stream);
    REQUIRE(st.moved().size() == 3 && st.moved()[2] == 2 && st.beta_ref()[2] == 1.5);
    // the copies of g, a, slot
    st.dev_a_uploaded(); st.dev_g_uploaded(); st.dev_slot_uploaded();
    REQUIRE(st.dev_a_current() && st.dev_g_current() && st.dev_slot_current());
    st.dev_g_moved_on(); st.folded();
    REQUIRE(!st.host_g_current() && st.dev_g_current() && st.moved().empty());
    st.host_g_fetched();
    const bool was = st.host_g_current();
    st.dev_g_moved_on(); st.dev_g_rolled_back(was);
    REQUIRE(st.host_g_current());
    st.dev_g_moved_on(); st.dev_g_rejected();
    REQUIRE(st.host_g_current() && !st.dev_g_current());
    st.dev_g_uploaded(); st.dev_g_dropped();
    REQUIRE(st.host_g_current() && !st.dev_g_current());
    // the device loop hands back what is still pending; zeros are none
    const int32_t idx[3] = {4, 0, 2};
    const double val[3] = {1.0, 0.0, -2.0};
    st.pending_replaced(idx, val, 3);
    REQUIRE(st.moved().size() == 2 && st.moved()[0] == 4 && st.moved()[1] == 2 && st.moved().value(2) == -2.0);
    st.cov_visited(40); st.cov_visited(2);
    REQUIRE(st.cov_since_ref() == 42);
    // y'y and r'r
    st.yy_summed(3.0);
    REQUIRE(st.yy_current() && st.yy() == 3.0);
    st.yy_void();
    REQUIRE(!st.yy_current());
    st.q_summed(4.0); st.q_carried(1.0); st.q_guard(1e-4);
    REQUIRE(st.q_usable() && st.q() == 1.0 && st.q_exact() == 4.0);
    st.q_carried(1e-5); st.q_guard(1e-4);
    REQUIRE(!st.q_usable());
    st.q_summed(2.0); st.q_void();
    REQUIRE(!st.q_usable() && st.q() == 2.0);
    // re-reference keeping beta; a rebuild from another iterate is moves in ascending k
    {
        const bool known = st.beta_known();
        st.invalidated(false);
        REQUIRE(!st.valid() && !st.beta_known() && st.moved().empty());
        st.referenced(known);
        REQUIRE(st.valid() && st.beta_known() && st.beta_ref()[2] == 1.5 && st.cov_since_ref() == 0 && !st.dev_a_current());
    }
    SupportList y(p);
    y.set(4, 2.0); y.set(0, 3.0);
    st.q_summed(1.0);
    st.rebuilt(y, p);                                    // beta_ref was (1, 2, 1.5, -1, 2)
    REQUIRE(st.moved().size() == 4 && st.moved()[0] == 0 && st.moved()[1] == 1 && st.moved()[2] == 2 && st.moved()[3] == 3);
    REQUIRE(st.moved().value(0) == 2.0 && st.moved().value(3) == 1.0 && st.beta_ref()[0] == 3.0 && !st.q_usable());
    // a NaN: the off-stream kind goes on, the streamed kind stops; either voids the cache
    REQUIRE(st.moved(1, nan, MoveKind::off_stream));
    REQUIRE(!st.valid() && !st.beta_known() && st.moved().empty() && st.host_g_current());
    REQUIRE(st.moved(1, 1.0, MoveKind::off_stream) && st.moved().empty());
    st.rebuilt(y, p); st.referenced(st.beta_known());
    REQUIRE(st.valid() && st.beta_known());
    REQUIRE(st.moved(2, 1.0, MoveKind::streamed) && !st.moved(2, nan, MoveKind::streamed) && !st.valid() && st.moved().empty());
    st.rebuilt(y, p); st.referenced(st.beta_known());
    st.moved(0, nan, MoveKind::carried, true);           // the device loop's moves reach the reference, NaN or not
    REQUIRE(st.valid() && st.beta_ref()[0] != st.beta_ref()[0]);
    // a cache whose reference is unknown does not survive a rebuild
    st.invalidated(false); st.referenced(false);
    st.rebuilt(x, p);
    REQUIRE(!st.valid() && st.beta_known() && st.beta_ref()[1] == 2.0 && st.beta_ref()[0] == 0.0);
    // the device loop's table, the prepared verdict, the forced marks, the stall rule
    st.table_allocated();
    REQUIRE(st.table_void() && st.table_entries() == 0);
    st.table_reset_done(); st.table_holds(17);
    REQUIRE(!st.table_void() && st.table_entries() == 17);
    st.dev_slot_uploaded(); st.dev_a_uploaded();
    st.invalidated(true);
    REQUIRE(st.table_void() && st.table_entries() == 0 && !st.dev_slot_current() && !st.dev_a_current());
    double cert = -1.0;
    REQUIRE(!st.prepared());
    st.prepared(true, 0.25);
    REQUIRE(st.prepared() && st.take_prepared(&cert) && cert == 0.25 && !st.prepared());
    st.prepared(false, 0.5);
    REQUIRE(!st.take_prepared(&cert) && cert == 0.5);
    st.prepared(true, 0.75); st.prepared_no_go();
    REQUIRE(!st.take_prepared(&cert) && cert == 0.75);
    st.prepared(true, 1.0); st.unprepared();
    REQUIRE(!st.prepared());
    st.forced_marks_set();
    REQUIRE(st.forced_marks_dirty());
    st.forced_marks_wiped();
    REQUIRE(!st.forced_marks_dirty());
    st.forced_marks_set(); st.mirrors_allocated();
    REQUIRE(!st.forced_marks_dirty());
    REQUIRE(!st.stalled_twice(true) && st.stalled_twice(true) && !st.stalled_twice(true) && !st.stalled_twice(false) && !st.stalled_twice(true));
    std::printf("CACHE_STATE_OK\n");
    return 0;
}
