// cache_state.hpp -- what the gradient cache knows ABOUT its data: which copy of g is current, whether g and beta_ref
// describe r, what the device mirrors and the device loop's table still hold.  Host only, standard library only
// (tests/cache_shim.cpp drives it on the CPU).  The data itself (g, a, slot, G, the device buffers) and the counters stay
// in GradCache (cdhip.hip); every fact about them changes through one of CacheState's named transitions, none of which
// touches the device: code that must do both asks first and then acts.  LAB_NOTES.md "Gradient cache state" has the table.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "resid_state.hpp"

namespace cdh {

// how a move of the iterate reaches the cache (CacheState::moved)
enum class MoveKind {
    streamed,      // a streamed visit has rewritten r: g owes the move, the carried r'r is void
    carried,       // a covariance-form visit: g on the device has the move already, r is left alone
    off_stream     // the one-launch solve from r: r is left alone, g owes the move
};

class CacheState {
public:
    // ---- what readers ask ----
    bool sized() const { return !beta_ref_.empty(); }
    bool valid() const { return valid_; }                       // g (with the pending moves) describes X'r of the current r
    bool beta_known() const { return beta_ok_; }                // r == y - X beta_ref up to rounding
    bool tracks_r() const { return valid_ || beta_ok_; }        // a move of r or beta means something to the cache
    const std::vector<double>& beta_ref() const { return beta_ref_; }
    const MoveLedger& moved() const { return moved_; }          // what the coordinates have moved by since g was last folded
    int64_t cov_since_ref() const { return cov_since_ref_; }    // covariance-form visits since g was last taken from X itself
    bool host_g_current() const { return g_host_ok_; }
    bool dev_g_current() const { return g_dev_ok_; }
    bool dev_a_current() const { return a_dev_ok_; }
    bool dev_slot_current() const { return slot_dev_ok_; }
    bool yy_current() const { return yy_ok_; }
    double yy() const { return yy_; }                           // y'y over all shards, good while yy_current()
    bool q_usable() const { return q_valid_; }
    double q() const { return q_; }                             // r'r of the residual g describes, carried through the visits
    double q_exact() const { return q_exact_; }                 // ... as last summed from r itself
    bool table_void() const { return cs_table_reset_; }
    int32_t table_entries() const { return cs_table_reset_ ? 0 : cs_ncid_; }   // coordinates the device loop's Gram table holds
    bool prepared() const { return prep_state_ != 0; }          // gc_prepare_full has run for the pass about to be walked
    bool forced_marks_dirty() const { return forced_dirty_; }

    // ---- sizing ----
    // first use on a handle of p coordinates; the reference follows the iterate x if r is its residual right now
    void size(int64_t p, bool consistent, const SupportList& x) {
        moved_.resize(p);
        beta_ref_.assign((std::size_t)p, 0.0);
        beta_ok_ = consistent;
        if (beta_ok_)
            for (int64_t s = 0; s < x.nnz(); ++s) beta_ref_[(std::size_t)x.coord(s)] = x.slot_value(s);
    }
    // the device mirrors of g and a were just allocated: they hold nothing, no forced mark is set
    void mirrors_allocated() { forced_dirty_ = false; g_dev_ok_ = false; a_dev_ok_ = false; }

    // ---- invalidation ----
    // g no longer describes r: whatever g held is void, the next reference pass fills the host copy.  Keeps a's mirror, yy,
    // the prepared verdict and the stall mark: none of them is taken from r.  columns: X changed -- a's mirror, the slot map
    // on the device and the device loop's table are void too (the table keeps its count until it is reset on the device)
    void invalidated(bool columns) {
        valid_ = false; beta_ok_ = false; q_valid_ = false;
        g_host_ok_ = true; g_dev_ok_ = false;
        moved_.clear();
        if (columns) { a_dev_ok_ = false; slot_dev_ok_ = false; cs_table_reset_ = true; }
    }

    // ---- a new reference point ----
    // g and a were just taken from X itself, on the host; nothing is pending.  beta_known: what was known about beta before
    // the invalidate that made room for this reference holds again (g describes the same residual, only freshly summed;
    // beta_ref itself was never touched)
    void referenced(bool beta_known) {
        moved_.clear();
        valid_ = true;
        g_host_ok_ = true; g_dev_ok_ = false; a_dev_ok_ = false;
        cov_since_ref_ = 0;
        beta_ok_ = beta_known;
    }

    // ---- the copies of g, a, slot; y'y ----
    void host_g_fetched() { g_host_ok_ = true; }                // d_g was copied into g (or the chunk's g_new swapped in)
    void dev_g_uploaded() { g_dev_ok_ = true; }
    void dev_a_uploaded() { a_dev_ok_ = true; }
    void dev_slot_uploaded() { slot_dev_ok_ = true; }
    // a kernel has moved d_g along; keeps g_dev_ok: the device copy is the current one
    void dev_g_moved_on() { g_host_ok_ = false; }
    // the device copy is void; keeps g_host_ok as it is (the host copy is the truth if there is one: the caller has asked)
    void dev_g_dropped() { g_dev_ok_ = false; }
    // the chunk d_g has seen never happened: the host copy, the gradient from before the chunk, is the one truth again
    void dev_g_rejected() { g_host_ok_ = true; g_dev_ok_ = false; }
    // d_g was restored from the pass's snapshot: the host copy is worth what it was worth when the pass began
    void dev_g_rolled_back(bool host_was_current) { g_host_ok_ = host_was_current; }
    void yy_summed(double yy) { yy_ = yy; yy_ok_ = true; }
    void yy_void() { yy_ok_ = false; }                          // a new y

    // ---- moves ----
    // Coordinate k of the iterate moved by d != 0.  The reference follows where it is known (a NaN only with ref_takes_nan:
    // the device loop's moves, as they always have); a move g owes joins the ledger, in the order the moves come (the bits
    // of the fold depend on it).  A NaN move that g owes voids the cache.  false: a streamed chunk has nothing more to tell
    // (the cache tracks nothing, or this NaN has just voided it); the one-launch solve goes on regardless.
    bool moved(int64_t k, double d, MoveKind kind, bool ref_takes_nan = false) {
        if (kind == MoveKind::streamed) {
            if (!tracks_r()) return false;
            if (d != d) { invalidated(false); return false; }
            if (beta_ok_) beta_ref_[(std::size_t)k] += d;
            q_valid_ = false;
            if (valid_) moved_.add(k, d);
            return true;
        }
        if (beta_ok_ && (ref_takes_nan || d == d)) beta_ref_[(std::size_t)k] += d;
        if (kind == MoveKind::carried) return true;
        if (d != d) { if (tracks_r()) invalidated(false); return true; }
        if (valid_) moved_.add(k, d);
        return true;
    }
    // r was just set to y - X x by a kernel: beta_ref follows; what changed against the previous reference becomes pending
    // moves, in ascending k (a warm start from another x is a move like any other).  A g whose reference was unknown is void
    void rebuilt(const SupportList& x, int64_t p) {
        if (!sized()) return;
        if (valid_ && !beta_ok_) invalidated(false);
        std::vector<double> nb((std::size_t)p, 0.0);
        for (int64_t s = 0; s < x.nnz(); ++s) nb[(std::size_t)x.coord(s)] = x.slot_value(s);
        if (valid_)
            for (int64_t k = 0; k < p; ++k) {
                const double d = nb[(std::size_t)k] - beta_ref_[(std::size_t)k];
                if (d != 0.0) moved_.add(k, d);
            }
        beta_ref_.swap(nb);
        beta_ok_ = true;
        q_valid_ = false;
    }
    void folded() { moved_.clear(); }                           // g has taken the pending moves
    // the device loop took the pending moves in and hands back those still pending when it stopped (zeros are none)
    void pending_replaced(const int32_t* idx, const double* val, int32_t n) {
        moved_.clear();
        for (int32_t m = 0; m < n; ++m) if (val[m] != 0.0) moved_.set(idx[m], val[m]);
    }
    void cov_visited(int64_t visits) { cov_since_ref_ += visits; }   // g was carried through this many more updates

    // ---- r'r ----
    void q_summed(double q) { q_ = q; q_exact_ = q; q_valid_ = true; }   // one pass over r itself
    void q_carried(double q) { q_ = q; }                        // the visits' recurrence; keeps q_exact and the flag
    // the carried value has fallen to `factor` of the last exact sum: it is summed afresh before the next pass
    void q_guard(double factor) { if (q_valid_ && q_ < factor * q_exact_) q_valid_ = false; }
    void q_void() { q_valid_ = false; }                         // r changed behind its back (or the kernel asks for a fresh sum)

    // ---- the device loop ----
    void table_allocated() { cs_ncid_ = 0; cs_table_reset_ = true; }
    void table_reset_done() { cs_ncid_ = 0; cs_table_reset_ = false; }   // its entries were wiped on the device
    void table_holds(int32_t ncid) { cs_ncid_ = ncid; }
    // gc_prepare_full has run for the next pass with this verdict: gc_full_pass, if it comes to that, does not prepare twice
    void prepared(bool go, double cert_abs) { prep_state_ = go ? 1 : 2; prep_cert_abs_ = cert_abs; }
    void prepared_no_go() { prep_state_ = 2; }                  // the loop backed off; keeps the certificate margin
    bool take_prepared(double* cert_abs) { const bool go = prep_state_ == 1; *cert_abs = prep_cert_abs_; prep_state_ = 0; return go; }
    void unprepared() { prep_state_ = 0; }                      // the state moves from here on: a later pass prepares afresh
    void forced_marks_set() { forced_dirty_ = true; }
    void forced_marks_wiped() { forced_dirty_ = false; }
    // the loop came back for columns, with or without a pass done.  true: the second time in a row without one (the host's
    // passes take over, and the count starts again)
    bool stalled_twice(bool no_progress) {
        if (no_progress && cs_stalled_) { cs_stalled_ = false; return true; }
        cs_stalled_ = no_progress;
        return false;
    }

private:
    bool valid_ = false, beta_ok_ = false;
    bool g_host_ok_ = true, g_dev_ok_ = false;       // at least one is current while valid_ (gc_fold's fallback aside: LAB_NOTES.md)
    bool a_dev_ok_ = false, slot_dev_ok_ = false, yy_ok_ = false, q_valid_ = false;
    bool cs_table_reset_ = true, forced_dirty_ = false, cs_stalled_ = false;
    int prep_state_ = 0;                             // 1 go, 2 no-go (0: not prepared)
    int32_t cs_ncid_ = 0;
    int64_t cov_since_ref_ = 0;
    double yy_ = 0.0, q_ = 0.0, q_exact_ = 0.0, prep_cert_abs_ = 0.0;
    std::vector<double> beta_ref_;
    MoveLedger moved_;
};

}  // namespace cdh
