// resid_state.hpp -- what the host knows about the residual buffer r, and the ledger of coordinate moves
// that both r and the gradient cache keep.  Host only, standard library only (tests/resid_shim.cpp drives it
// on the CPU).  Every fact about r changes through one of ResidState's named transitions; LAB_NOTES.md
// "Residual state" has the table.  Coordinates are 0-based.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "sparse_iterate.hpp"

namespace cdh {

// Moves of coordinates that somebody still owes somebody: a dense value per coordinate, and the members in
// the order they were FIRST added (the catch-up of r and the cache's fold walk that order: the bits of
// their sums depend on it).  Membership is the byte, never the value: moves that cancel to 0.0 keep their
// member, a NaN is a value like any other.  Sized once; nothing here allocates afterwards.
class MoveLedger {
public:
    void resize(int64_t p) {
        val_.assign((std::size_t)p, 0.0); in_.assign((std::size_t)p, 0);
        list_.clear(); list_.reserve((std::size_t)p);
    }
    void add(int64_t k, double d) { join(k); val_[(std::size_t)k] += d; }
    void set(int64_t k, double v) { join(k); val_[(std::size_t)k] = v; }
    double value(int64_t k) const { return val_[(std::size_t)k]; }
    bool contains(int64_t k) const { return in_[(std::size_t)k] != 0; }
    bool empty() const { return list_.empty(); }
    std::size_t size() const { return list_.size(); }
    int64_t operator[](std::size_t i) const { return list_[i]; }       // the i-th member
    std::vector<int64_t>::const_iterator begin() const { return list_.begin(); }
    std::vector<int64_t>::const_iterator end() const { return list_.end(); }
    void clear() {       // touches the members only
        for (int64_t k : list_) { val_[(std::size_t)k] = 0.0; in_[(std::size_t)k] = 0; }
        list_.clear();
    }

private:
    void join(int64_t k) {
        if (!in_[(std::size_t)k]) { in_[(std::size_t)k] = 1; list_.push_back(k); }
    }
    std::vector<double> val_;
    std::vector<uint8_t> in_;
    std::vector<int64_t> list_;
};

inline bool same_iterate(const SupportList& a, const SupportList& b) {
    if (a.size() != b.size() || a.nnz() != b.nnz()) return false;
    for (int64_t s = 0; s < a.nnz(); ++s) if (a.coord(s) != b.coord(s) || !(a.slot_value(s) == b.slot_value(s))) return false;
    return true;
}

// The buffer r on the device and the residual the handle STANDS FOR are two things:
//   stands for = buffer - X * pending        (covariance-form visits move beta and leave r to catch up), or
//   stands for = y - X * lazy_iterate()      (lazy: the one-launch solve never touches r; whatever the buffer holds is stale).
// On top of that: `consistent` -- the residual stood for is y - X beta of the handle's current iterate; `pristine` -- the
// BUFFER is bit for bit what initialize! makes of one known iterate and nothing has written it since; the stash -- dots of
// all p columns with the residual stood for; `roundings` -- launches that have rewritten the buffer since its last rebuild.
class ResidState {
public:
    void resize(int64_t p) { pending_.resize(p); }

    // ---- what readers ask ----
    bool consistent() const { return consistent_; }
    bool lazy() const { return lazy_; }
    const MoveLedger& pending() const { return pending_; }
    bool owes_catchup() const { return lazy_ || !pending_.empty(); }     // the buffer is not the residual stood for
    int64_t roundings() const { return roundings_; }
    int64_t rebuilds_skipped() const { return n_rebuild_skipped_; }
    int64_t dots_adopted() const { return n_dots_adopted_; }
    // would initialize! of x write the very bits the buffer holds?  (k_init_resid is deterministic)
    bool rebuild_is_noop(const SupportList& x) const {
        return pristine_ && !lazy_ && pending_.empty() && same_iterate(x, x_pristine_);
    }
    // may a reference pass of the gradient cache take the stash instead of reading X?  (weighted: the dots it would take)
    bool can_adopt_dots(bool weighted, int64_t p) const {
        return dots_valid_ && dots_w_ == weighted && (int64_t)stash_.size() == 2 * p;
    }

    // ---- the buffer is written ----
    // a streamed chunk is about to read and rewrite r: the buffer is no rebuild's any more, the residual stood for moves
    void stream_begins() { written(); }
    // ... and has been enqueued: each launch that applied updates rounded r to the storage type once
    void stream_enqueued(int64_t launches) { roundings_ += launches; }
    // the catch-up is about to apply the pending moves to the buffer; keeps the stash: the residual stood for stays the same
    void catchup_begins() { pristine_ = false; }
    void catchup_batch_applied() { roundings_ += 1; }                   // one k_multi_axpy launch
    void catchup_done() { pending_.clear(); }
    // somebody wants the residual the one-launch solve left unformed: the caller rebuilds from the iterate returned.  Not
    // lazy from here on, so that the rebuild may find the buffer already holds it (a solve that moved nothing)
    const SupportList& take_lazy() { lazy_ = false; return x_lazy_; }
    // initialize! is about to overwrite r: nothing to catch up with, and it rounds once
    void rebuild_begins() { overwritten(); roundings_ = 1; }
    // ... and has: r = y - X x, bit for bit
    void rebuilt_from(const SupportList& x) { consistent_ = true; pristine_ = true; x_pristine_ = x; }
    // the buffer already held what initialize!(x) writes (rebuild_is_noop): keeps the stash, the residual stood for is the same
    void rebuild_skipped() { roundings_ = 1; consistent_ = true; n_rebuild_skipped_ += 1; }
    // a kernel has just written y, W and r together so that r IS y - X x of the current iterate (cdh_glm_irls: r = d / w under
    // the new working response), after r had caught up: consistent, but NOT the bits initialize! would write -- a later
    // rebuild must run -- and nothing taken of the old r, y or W holds
    void rewritten_as_residual() { overwritten(); roundings_ = 1; consistent_ = true; }
    // r = copy(y) under a new y: whatever the iterate is, r is not its residual
    void overwritten_with_y() { consistent_ = false; overwritten(); }
    // X and y regenerated with r = y; keeps `consistent`: the generator zeroes the iterate, so r IS its residual -- a
    // carried `false` only costs the next warm start its shortcut
    void regenerated() { overwritten(); }

    // ---- the buffer stays, what it means changes ----
    // X, W or the loss changed: nothing taken from them holds.  Keeps pending and lazy: what r owes is owed in columns of
    // X, which W and the loss leave alone (a change of X applies it first: design_changes)
    void design_or_loss_changed() { consistent_ = false; written(); }
    // the caller loaded another iterate without initialize!: r is left alone, as the reference's x[k] = ... leaves it
    void iterate_loaded() { consistent_ = false; }
    // the iterate moved in a kernel that does not write r: the residual stood for moves with it ...
    void iterate_moved() { dots_valid_ = false; }
    // ... by d at coordinate k: r owes -d X_k
    void moved(int64_t k, double d) { iterate_moved(); pending_.add(k, d); }
    // the one-launch solve ended at x without reading or writing r: r stands for y - X x, formed when somebody asks
    void left_lazy(const SupportList& x) { dots_valid_ = false; pending_.clear(); lazy_ = true; x_lazy_ = x; consistent_ = true; }

    // ---- the stash ----
    // (X_k'W r, X_k'W X_k) for all k were just taken of the residual stood for (the catch-up has run)
    void dots_taken(const std::vector<double>& cd, bool weighted) { stash_ = cd; dots_valid_ = true; dots_w_ = weighted; }
    void dots_taken(std::vector<double>&& cd, bool weighted) { stash_.swap(cd); dots_valid_ = true; dots_w_ = weighted; }   // cd is done with
    const std::vector<double>& adopt_dots() { n_dots_adopted_ += 1; return stash_; }

private:
    void written() { pristine_ = false; dots_valid_ = false; }
    void overwritten() { written(); pending_.clear(); lazy_ = false; }   // from scratch: what r owed is void
    bool consistent_ = false, lazy_ = false, pristine_ = false, dots_valid_ = false, dots_w_ = false;
    SupportList x_lazy_, x_pristine_;
    MoveLedger pending_;
    std::vector<double> stash_;
    int64_t roundings_ = 0, n_rebuild_skipped_ = 0, n_dots_adopted_ = 0;
};

}  // namespace cdh
