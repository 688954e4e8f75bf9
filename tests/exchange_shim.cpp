// Test-only C shim over csrc/exchange_state.hpp (the row-shard exchange's state), compiled with g++ and driven on
// the CPU by tests/test_exchange_state.py.  The handle's part is played by two facts: whether the inbox exists and
// whether the pinned timeout flag is set.  xs_comm_init ... xs_host set, xs_allreduce and xs_chunk call the
// transitions in the order the exports, allreduce and run_chunk (csrc/cdhip.hip) call them; the rest is one method each.
#include <cstdint>
#include "../coordinatedescent.jl_amd/csrc/exchange_state.hpp"

using cdh::ExchangeState;
using cdh::Refusal;
using cdh::Route;

namespace {
struct State { ExchangeState xs; bool inbox = false, flag = false; const char* msg = ""; };
int32_t said(State* s, const Refusal& r) { s->msg = r.msg; return r.status; }
int32_t host_cb(void*, double*, int64_t) { return 0; }
char a_comm;      // stands for a communicator
int32_t p2p_check(State* s) {
    if (s->xs.direct_on() && s->flag) return said(s, s->xs.p2p_timed_out());
    return CDH_OK;
}
// allreduce(): *issued counts the direct exchange's pieces, each epoch is passed to `each`
template <class F> int32_t allreduce(State* s, uint64_t count, F&& each) {
    ExchangeState& xs = s->xs;
    const cdh::Routing to = xs.route((size_t)count);
    switch (to.route) {
    case Route::Refuse: return said(s, to.why);
    case Route::Nothing: return CDH_OK;
    case Route::Direct:
        if (p2p_check(s) != CDH_OK) return CDH_RCCL_ERROR;
        for (uint64_t o = 0; o < count; o += cdk::kP2PMaxCount) { each(xs.next_epoch()); xs.issued(to.route); }
        return CDH_OK;
    default: break;
    }
    xs.issued(to.route);
    return CDH_OK;
}
}  // namespace

extern "C" {
void* xs_new() { return new State(); }
void xs_free(void* s) { delete (State*)s; }
const char* xs_msg(void* s) { return ((State*)s)->msg; }
int xs_max_count() { return cdk::kP2PMaxCount; }
int xs_max_ranks() { return cdk::kP2PMaxRanks; }
uint32_t xs_epoch_wrap() { return cdh::kEpochWrap; }
uint32_t xs_epoch_soft_wrap() { return cdh::kEpochSoftWrap; }
#define S ((State*)s)
#define XS (((State*)s)->xs)
// ---- the exports' decisions and state changes (the HIP / RCCL work between them always succeeds here) ----
int32_t xs_comm_init(void* s, int rank, int nranks, int force_rccl) {
    const int32_t rc = said(S, XS.comm_refused(rank, nranks));
    if (rc != CDH_OK) return rc;
    if (nranks == 1 && !force_rccl) { XS.comm_not_needed(); return CDH_OK; }
    XS.comm_installed(&a_comm, rank, nranks);
    return CDH_OK;
}
int32_t xs_comm_drop(void* s) {
    if (!XS.communicator()) return CDH_OK;
    XS.comm_dropped();
    return CDH_OK;
}
int32_t xs_p2p_local_handle(void* s) { S->inbox = true; return CDH_OK; }
int32_t xs_p2p_connect(void* s, int rank, int nranks) {
    const int32_t rc = said(S, XS.p2p_connect_refused(rank, nranks, S->inbox));
    if (rc == CDH_OK) XS.p2p_connected(rank, nranks);
    return rc;
}
int32_t xs_p2p_enable(void* s, int on) {
    if (!on) { XS.p2p_disabled(); return CDH_OK; }
    return said(S, XS.p2p_enabled(XS.direct_ranks() && S->flag));
}
// a kernel of the direct exchange ran out of its spin (only a running direct exchange can) ...
void xs_raise_timeout_flag(void* s) { if (XS.direct_on()) S->flag = true; }
int32_t xs_p2p_check(void* s) { return p2p_check(S); }     // ... and the host looks
int32_t xs_host_set(void* s, int install, int rank, int nranks) {
    if (!install) { XS.host_removed(); return CDH_OK; }
    const int32_t rc = said(S, XS.host_refused(rank, nranks));
    if (rc == CDH_OK) XS.host_installed(host_cb, S, rank, nranks);
    return rc;
}
void xs_capture_begins(void* s) { XS.capture_begins(); }
// run_chunk after a capture: the graph is replayed at once
void xs_capture_ends_and_replays(void* s, uint32_t* out2) {
    const cdh::Captured c = XS.capture_ends();
    out2[0] = c.exchanges; out2[1] = c.rccl;
    if (c.exchanges) (void)XS.reserve_epochs(c.exchanges);
    XS.replay_counted(c);
}
int32_t xs_allreduce(void* s, uint64_t count) { return allreduce(S, count, [](unsigned) {}); }
// ---- what readers ask ----
int xs_sharded(void* s) { return XS.sharded(); }
int32_t xs_alive(void* s) { return said(S, XS.alive()); }
int xs_route(void* s, uint64_t count) {      // 0 host, 1 direct, 2 RCCL, 3 nothing, 4 refuse (status and message: xs_route_status, xs_msg)
    const cdh::Routing to = XS.route((size_t)count);
    if (to.route == Route::Refuse) (void)said(S, to.why);
    return (int)to.route;
}
int32_t xs_route_status(void* s, uint64_t count) { return XS.route((size_t)count).why.status; }
int xs_route_hands_back_what_was_installed(void* s) {
    return (XS.communicator() == nullptr || XS.communicator() == (void*)&a_comm) &&
           (XS.host_callback() == nullptr || (XS.host_callback() == host_cb && XS.host_context() == s));
}
int xs_may_capture(void* s) { return XS.may_capture(); }
uint32_t xs_graph_key_bits(void* s) { return XS.graph_key_bits(); }
int xs_reported_ranks(void* s) { return XS.reported_ranks(); }
int xs_rank(void* s) { return XS.rank(); }
int xs_nranks(void* s) { return XS.nranks(); }
void xs_counters(void* s, int64_t* out3) { out3[0] = XS.rccl_calls(); out3[1] = XS.direct_calls(); out3[2] = XS.host_calls(); }
// ---- epochs ----
void xs_seed_epoch(void* s, uint32_t e) { XS.seed_epoch(e); }
uint32_t xs_last_epoch(void* s) { return XS.last_epoch(); }
// One chunk of k direct exchanges (records of 4 doubles), as run_chunk issues them: how = 0 node by node, 1 recorded in
// a graph (the epochs are positions), 2 a graph of k exchanges replayed.  prev: the epoch issued last before the chunk
// (0: none).  out: [0] status, [1] first epoch, [2] last epoch, [3] epochs issued, [4] epochs that are not their
// predecessor + 1 (inside the chunk), [5] epochs equal to 0, [6] epochs that share their predecessor's parity (prev
// included), [7] for how = 1: exchanges the capture says it recorded, for how = 2: the base.
void xs_chunk(void* s, uint32_t k, int how, uint32_t prev, uint64_t* out) {
    for (int i = 0; i < 8; ++i) out[i] = 0;
    bool have_prev = prev != 0;
    auto each = [&](unsigned e) {
        if (!out[3]) out[1] = e;
        else if (e != (unsigned)out[2] + 1u) out[4] += 1;
        if (e == 0) out[5] += 1;
        if (have_prev && ((e ^ prev) & 1u) == 0) out[6] += 1;
        out[2] = e; out[3] += 1; prev = e; have_prev = true;
    };
    if (how == 2) {
        XS.chunk_begins();
        const uint32_t base = XS.reserve_epochs(k);
        XS.replay_counted({k, 0});
        out[7] = base;
        for (uint32_t i = 1; i <= k; ++i) each(base + i);       // what k_p2p_allreduce computes: *epoch_base + position
        return;
    }
    if (how == 1) XS.capture_begins(); else XS.chunk_begins();
    for (uint32_t i = 0; i < k && out[0] == CDH_OK; ++i) out[0] = (uint64_t)allreduce(S, 4, each);
    if (how == 1) out[7] = XS.capture_ends().exchanges;
}
}
