// The wait between the retirement of a registered key and the reuse of what a keyed launch may still read of it - a device table, a
// slot, a snapshot array (pure C++, no HIP; fabgpu_api.hip is the user, once per curve, hosttest_keyed_fence.cpp runs it on the CPU
// over a model of streams and events).
//
// The protocol, the same for every kind of registered key:
//   1. A launcher takes its view of the key table under the BOOK'S LOCK (the caller's mutex over the table; kmu, k384_mu) and, still
//      under it, calls enter() with the streams it will queue keyed launches on.  It is counted from then until its ticket dies, which
//      must be after its last keyed enqueue.  Nothing between the two may take the book's lock: a waiter holds it.
//   2. Memory such a launch may read is reused only behind a wait: at a moment when no launcher is counted (quiet(); the book's lock is
//      held, so nobody takes a new view meanwhile) events are recorded on every stream that has ever carried a keyed launch
//      (record()), and those events have completed (done()).  Whoever took a view earlier has enqueued - the events cover it; whoever
//      takes one later sees what the caller published before the wait.
//   3. A stream that refuses the record is one the caller has destroyed since (it must have been idle by then) and is forgotten -
//      unless it is one of the owner's OWN streams, which live as long as the fence: such a stream is synchronised instead and kept.
//   4. Nobody has to block: done(evs, false) and quiet(false) only ask, so drains can advance on the paths that change the book
//      (advance()), and only a registration that needs one particular slot waits, for exactly that slot's drain (wait_for()).
//
// Locking: the launcher count has a leaf mutex of its own (taken under the book's lock or alone).  EVERYTHING ELSE here - the remembered
// streams, the event pool, the event lists handed to record() and done() - is guarded by the book's lock, which the caller holds
// around every call but a ticket's death.
//
// Dev: static functions over two handle types, a value-initialised Event meaning "none":
//     Event make_event()            Event{}: it could not be made
//     void  destroy_event(Event)
//     bool  record(Event, Stream)   false: the stream refused
//     FenceQuery query(Event)       without blocking
//     void  wait(Event)             until the event has completed (or its device has failed)
//     bool  sync(Stream)            false: the stream could not be waited for
#pragma once
#include <algorithm>
#include <condition_variable>
#include <initializer_list>
#include <mutex>
#include <vector>

namespace fab {

enum class FenceQuery { DONE, NOT_READY, FAILED };

template <class Dev>
class KeyedFence {
public:
    using Event = typename Dev::Event;
    using Stream = typename Dev::Stream;

    // A launcher's place in the count.  Move-only; its death (or release()) uncounts and wakes the waiters.
    class Ticket {
    public:
        Ticket() = default;
        Ticket(Ticket&& o) noexcept : f_(o.f_) { o.f_ = nullptr; }
        Ticket& operator=(Ticket&& o) noexcept {
            if (this != &o) {
                release();
                f_ = o.f_;
                o.f_ = nullptr;
            }
            return *this;
        }
        Ticket(const Ticket&) = delete;
        Ticket& operator=(const Ticket&) = delete;
        ~Ticket() { release(); }
        void release() {
            if (!f_) return;
            std::lock_guard<std::mutex> ll(f_->lm_);
            if (--f_->launchers_ == 0) f_->cv_.notify_all();
            f_ = nullptr;
        }

    private:
        friend class KeyedFence;
        explicit Ticket(KeyedFence* f) : f_(f) {}
        KeyedFence* f_ = nullptr;
    };

    KeyedFence() = default;
    KeyedFence(const KeyedFence&) = delete;
    KeyedFence& operator=(const KeyedFence&) = delete;

    // (the book's lock held) the streams are remembered, the launcher is counted
    Ticket enter(std::initializer_list<Stream> streams) {
        for (Stream s : streams)
            if (std::find(streams_.begin(), streams_.end(), s) == streams_.end()) streams_.push_back(s);
        std::lock_guard<std::mutex> ll(lm_);
        launchers_++;
        return Ticket(this);
    }

    // no launcher is counted.  wait: sleeps until that is so (launchers never take the book's lock while counted, so they finish)
    bool quiet(bool wait) {
        std::unique_lock<std::mutex> ll(lm_);
        if (launchers_ != 0 && !wait) return false;
        cv_.wait(ll, [&] { return launchers_ == 0; });
        return true;
    }

    // One event into evs behind everything queued so far on every remembered stream, and on every stream of `extra` (the owner's own
    // by definition).  owned(s): s is one of the owner's own streams (rule 3).  false: an own stream could neither be recorded on nor
    // synchronised - its device has failed.
    template <class Owned>
    bool record(std::vector<Event>& evs, Owned owned, const std::vector<Stream>& extra = {}) {
        bool ok = true;
        auto one = [&](Stream s, bool own) {      // false: forget the stream
            const Event e = get();
            if (e != Event{} && Dev::record(e, s)) {
                evs.push_back(e);
                return true;
            }
            if (e != Event{}) put(e);
            if (own) ok = Dev::sync(s) && ok;
            return own;
        };
        for (size_t i = 0; i < streams_.size();) {
            if (one(streams_[i], owned(streams_[i]))) i++;
            else streams_.erase(streams_.begin() + (long)i);
        }
        for (Stream s : extra) one(s, true);
        return ok;
    }

    // The events of evs have completed, asked (or with wait: waited for) from the back; those that have - or whose device has failed:
    // nothing of it runs any more - return to the pool.  false: the first one that is not ready, which stays in evs with those before it.
    bool done(std::vector<Event>& evs, bool wait) {
        while (!evs.empty()) {
            if (wait) Dev::wait(evs.back());
            else if (Dev::query(evs.back()) == FenceQuery::NOT_READY) return false;
            put(evs.back());
            evs.pop_back();
        }
        return true;
    }

    // The event pool: every event of a drain, and of whatever else may end up in one, comes from here and returns here.
    Event get() {
        if (pool_.empty()) return Dev::make_event();
        const Event e = pool_.back();
        pool_.pop_back();
        return e;
    }
    void put(Event e) { pool_.push_back(e); }
    void destroy_all() {      // shutdown: the events at rest (those in unfinished lists are their holder's to destroy)
        for (Event e : pool_) Dev::destroy_event(e);
        pool_.clear();
    }

    // Lists of drains, oldest first.  step(d, wait): one drain as far as it goes without blocking (wait: all the way); true: finished.
    // Every drain that finishes without waiting is erased; the others keep their order.
    template <class D, class Step>
    static void advance(std::vector<D>& drains, Step step) {
        for (size_t i = 0; i < drains.size();) {
            if (step(drains[i], false)) drains.erase(drains.begin() + (long)i);
            else i++;
        }
    }
    // The first drain that matches pred, all the way, and erased; the others are not touched.  false: it did not finish (and stays).
    // true also when nothing matches - whether that is good news is the caller's to say.
    template <class D, class Pred, class Step>
    static bool wait_for(std::vector<D>& drains, Pred pred, Step step) {
        for (size_t i = 0; i < drains.size(); i++)
            if (pred(drains[i])) {
                if (!step(drains[i], true)) return false;
                drains.erase(drains.begin() + (long)i);
                return true;
            }
        return true;
    }

private:
    std::vector<Stream> streams_;      // every stream ever passed to enter() that has not refused a record since
    std::vector<Event> pool_;
    std::mutex lm_;                    // launchers_ only (a leaf)
    std::condition_variable cv_;
    int launchers_ = 0;
};

}  // namespace fab
