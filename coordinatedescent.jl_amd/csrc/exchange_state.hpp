// exchange_state.hpp -- what the host knows about the row-shard exchange: which transport serves the shard, where
// an all-reduce goes, the epochs of the direct exchange, and what a graph capture has recorded.  Host only,
// standard library only (tests/exchange_shim.cpp drives it on the CPU).  Every fact changes through one of
// ExchangeState's named transitions; LAB_NOTES.md "Exchange state" has the table.  The HIP resources behind the
// facts (the IPC mappings, the inbox, the pinned timeout flag, the staging buffer) stay on the handle; the
// communicator and the callback are kept here as opaque pointers, for route()'s caller to hand on.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/cdhip.h"
#include "p2p_limits.hpp"

namespace cdh {

// Epochs count direct exchanges; 0 means "never written".  Consecutive epochs must alternate the
// inbox slot (parity), also across the 32-bit wrap.
constexpr unsigned kEpochWrap = 0xfffffff0u;
// Chunks start below this: every rank passes a chunk boundary with the same epoch count whether it replays a
// graph or launches node by node, so wrapping THERE keeps ranks on different paths in step.  That holds for a
// chunk of fewer than kEpochWrap - kEpochSoftWrap = 2^28 - 16 exchanges: the hard wrap is then never reached inside one.
constexpr unsigned kEpochSoftWrap = 0xf0000000u;

enum class Route { Host, Direct, Rccl, Nothing, Refuse };
// a transition or a query says no: the status and the message the export returns (CDH_OK: go ahead)
struct Refusal { int32_t status; const char* msg; };
struct Routing { Route route; Refusal why; };          // why: of Route::Refuse
struct Captured { unsigned exchanges, rccl; };         // what one graph holds: direct exchanges, RCCL all-reduces

class ExchangeState {
public:
    // ---- what readers ask ----
    int rank() const { return rank_; }
    int nranks() const { return nranks_; }
    int direct_ranks() const { return p2p_ranks_; }     // 0: not connected
    bool direct_on() const { return p2p_on_; }
    void* communicator() const { return comm_; }
    cdh_host_allreduce_fn host_callback() const { return host_fn_; }
    void* host_context() const { return host_user_; }
    bool in_capture() const { return capturing_; }
    int64_t rccl_calls() const { return n_rccl_calls_; }
    int64_t direct_calls() const { return n_p2p_calls_; }
    int64_t host_calls() const { return n_host_calls_; }
    // Is this handle one shard of several?  The dead and the lost count: a shard that lost its exchange must never fall
    // into the single-process (fused) finalize kernels on its local rows -- every path then reaches route(), which refuses.
    // ODDITY: a shard connected for the direct exchange alone (nranks > 1, no communicator) is NOT sharded while that
    // exchange is off -- between connect and the first enable, and after a disable -- and nothing marks it lost
    bool sharded() const { return comm_ != nullptr || p2p_on_ || p2p_dead_ || lost_exchange_ || host_fn_ != nullptr; }
    // A shard that has lost its exchange refuses to sweep at all -- also where a pass could be served from sums exchanged
    // earlier (the gradient cache): the ranks of one problem must fail together, not one by one as they come to need an exchange.
    Refusal alive() const {
        if (p2p_dead_) return {CDH_RCCL_ERROR, "the shard lost its exchange (p2p timed out earlier); rebuild the handle"};
        if (lost_exchange_) return {CDH_RCCL_ERROR, "the shard's host exchange was removed and nothing replaced it: its sums would cover local rows only"};
        return ok();
    }
    // Where an all-reduce of `count` doubles goes.  Direct: the caller still looks at the timeout flag (p2p_timed_out).
    // ODDITY: the direct route takes records longer than kP2PMaxCount (in pieces) only when there is no communicator
    Routing route(std::size_t count) const {
        if (host_fn_) {
            if (capturing_) return {Route::Refuse, {CDH_BAD_ARG, "the host-staged exchange cannot be recorded in a graph"}};
            return {Route::Host, ok()};
        }
        if (p2p_on_ && (count <= (std::size_t)cdk::kP2PMaxCount || !comm_)) return {Route::Direct, ok()};
        const Refusal a = alive();
        if (a.status != CDH_OK) return {Route::Refuse, a};
        return {comm_ ? Route::Rccl : Route::Nothing, ok()};
    }
    // may a chunk's launches be recorded in a graph?  (the host-staged exchange cannot; a dead one is not worth it)
    bool may_capture() const { return !host_fn_ && !p2p_dead_; }
    // the exchange's share of a captured chunk's key: graphs recorded under one transport are not replayed under another
    unsigned graph_key_bits() const { return (comm_ ? 32u : 0u) | (p2p_on_ ? 16u : 0u); }
    // the rank count cdh_exchange_stats reports (with a communicator the export asks ncclCommCount, and this is its fallback)
    int reported_ranks() const { return comm_ ? nranks_ : p2p_on_ ? p2p_ranks_ : host_fn_ ? nranks_ : 1; }

    // ---- who serves the shard: each install says first whether it may, then (the HIP / RCCL work done) that it has ----
    Refusal comm_refused(int rank, int nranks) const {
        if (host_fn_) return {CDH_BAD_ARG, "the handle already exchanges through a host transport"};
        return bad_ranks(rank, nranks) ? Refusal{CDH_BAD_ARG, "bad rank / nranks"} : ok();
    }
    // one rank and no communicator asked for.  ODDITY: leaves lost_exchange_ alone
    void comm_not_needed() { rank_ = 0; nranks_ = 1; }
    void comm_installed(void* comm, int rank, int nranks) { comm_ = comm; rank_ = rank; nranks_ = nranks; lost_exchange_ = false; }
    // ODDITY: tests the direct exchange being ON, host_removed() its being CONNECTED
    void comm_dropped() {
        comm_ = nullptr;
        if (nranks_ > 1 && !p2p_on_ && !host_fn_) lost_exchange_ = true;
    }
    Refusal p2p_connect_refused(int rank, int nranks, bool have_inbox) const {
        if (host_fn_) return {CDH_BAD_ARG, "the handle already exchanges through a host transport"};
        if (bad_ranks(rank, nranks) || nranks > cdk::kP2PMaxRanks) return {CDH_BAD_ARG, "p2p exchange: bad rank / nranks (at most 8 ranks)"};
        if (!have_inbox) return {CDH_BAD_ARG, "cdh_p2p_local_handle must be called first"};
        if (comm_ && (rank != rank_ || nranks != nranks_)) return {CDH_BAD_ARG, "p2p exchange: rank / nranks differ from the RCCL communicator's"};
        if (p2p_ranks_) return {CDH_BAD_ARG, "p2p exchange is already connected"};
        return ok();
    }
    void p2p_connected(int rank, int nranks) { rank_ = rank; nranks_ = nranks; p2p_ranks_ = nranks; }
    // timed_out: the pinned flag, looked at by the caller only when there is one (connected)
    Refusal p2p_enabled(bool timed_out) {
        if (!p2p_ranks_) return {CDH_BAD_ARG, "p2p exchange is not connected"};
        if (timed_out) return {CDH_RCCL_ERROR, "p2p exchange timed out earlier on this handle; it stays off"};
        p2p_on_ = true;
        lost_exchange_ = false;      // the direct exchange serves the shard again
        return ok();
    }
    void p2p_disabled() { p2p_on_ = false; }
    // the timeout flag was found set while the direct exchange was on.  After a timeout the ranks no longer agree on what
    // has been exchanged: the handle refuses every later exchange (falling back to RCCL here could pair mismatched
    // all-reduces and hang)
    Refusal p2p_timed_out() {
        p2p_on_ = false;
        p2p_dead_ = true;
        return {CDH_RCCL_ERROR, "p2p exchange timed out waiting for a peer (rank died, or ranks ran different sweeps)"};
    }
    Refusal host_refused(int rank, int nranks) const {
        if (bad_ranks(rank, nranks)) return {CDH_BAD_ARG, "bad rank / nranks"};
        if (comm_ || p2p_ranks_) return {CDH_BAD_ARG, "the handle already has an exchange (RCCL / direct)"};
        return ok();
    }
    void host_installed(cdh_host_allreduce_fn fn, void* user, int rank, int nranks) {
        host_fn_ = fn; host_user_ = user; rank_ = rank; nranks_ = nranks;
        lost_exchange_ = false;
    }
    // a shard of a multi-rank problem must not quietly fall into the single-process kernels on its local rows
    // (!comm_ cannot be otherwise here: host_refused)
    void host_removed() {
        if (host_fn_ && nranks_ > 1 && !comm_ && !p2p_ranks_) lost_exchange_ = true;
        host_fn_ = nullptr; host_user_ = nullptr;
    }

    // ---- epochs of the direct exchange ----
    // The epoch the next exchange runs under.  While a graph is being recorded: the position of the exchange in the
    // graph instead (from 1), to which the kernel adds the base of the replay.
    unsigned next_epoch() {
        if (capturing_) return ++cap_exchanges_;
        rewind_if(epoch_ >= kEpochWrap);
        return ++epoch_;
    }
    // a chunk begins: the soft wrap
    void chunk_begins() { rewind_if(epoch_ >= kEpochSoftWrap); }
    // A graph with k > 0 direct exchanges is about to be replayed: they run under base + 1 .. base + k.  Returns the
    // base, for the host to put where the graph's kernels read it.
    unsigned reserve_epochs(unsigned k) {
        rewind_if((uint64_t)epoch_ + k >= (uint64_t)kEpochWrap);
        const unsigned base = epoch_;
        epoch_ += k;
        return base;
    }
    void seed_epoch(unsigned e) { epoch_ = e; }           // tests only: the wraps are 2^28 exchanges away otherwise
    unsigned last_epoch() const { return epoch_; }

    // ---- capture bookkeeping and counters ----
    void capture_begins() { capturing_ = true; cap_exchanges_ = 0; cap_rccl_ = 0; }
    Captured capture_ends() { capturing_ = false; return {cap_exchanges_, cap_rccl_}; }
    // what a graph recorded is counted each time it is replayed, not when it was captured
    void replay_counted(const Captured& c) { n_p2p_calls_ += c.exchanges; n_rccl_calls_ += c.rccl; }
    // an all-reduce went out through r (the direct exchange: one piece of it, of at most kP2PMaxCount doubles).  While
    // capturing, RCCL's are recorded for the replays to count; the direct exchange's are, by next_epoch
    void issued(Route r) {
        if (r == Route::Host) n_host_calls_ += 1;
        else if (r == Route::Direct) { if (!capturing_) n_p2p_calls_ += 1; }
        else if (r == Route::Rccl) { if (capturing_) cap_rccl_ += 1; else n_rccl_calls_ += 1; }
    }

private:
    static Refusal ok() { return {CDH_OK, ""}; }
    static bool bad_ranks(int rank, int nranks) { return nranks < 1 || rank < 0 || rank >= nranks; }
    // The one wrap rule: the last epoch used goes back to 1 or 2, whichever has ITS parity, so that the epoch after it
    // (2 or 3, never 0) lands in the other inbox slot as if nothing had happened.
    void rewind_if(bool due) { if (due) epoch_ = (epoch_ & 1u) ? 1u : 2u; }

    void* comm_ = nullptr;
    int rank_ = 0, nranks_ = 1;
    int p2p_ranks_ = 0;
    bool p2p_on_ = false, p2p_dead_ = false;
    bool lost_exchange_ = false;       // a multi-rank shard whose transport was taken away: route() refuses
    cdh_host_allreduce_fn host_fn_ = nullptr;
    void* host_user_ = nullptr;
    unsigned epoch_ = 0;               // the last epoch used
    bool capturing_ = false;           // a graph is being recorded: exchanges take base + position epochs
    unsigned cap_exchanges_ = 0, cap_rccl_ = 0;   // exchanges recorded in the graph being captured
    int64_t n_rccl_calls_ = 0, n_p2p_calls_ = 0, n_host_calls_ = 0;
};

}  // namespace cdh
