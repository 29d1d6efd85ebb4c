// Stand-alone host program over KeyedFence (keyed_fence.h; its own main; built by the Makefile as ../lib/hosttest_keyed_fence, as
// ../lib/hosttest_keyed_fence_san with -fsanitize=address,undefined by `make sanitize-keyed-fence` and as ../lib/hosttest_keyed_fence_tsan
// with -fsanitize=thread by `make sanitize-keyed-fence-thread`).  The fence is pure C++ over a `Dev` of streams and events, so it runs
// here over a model of them, without a device.
//
// The model: a stream is two counters, enqueued and completed, and the queue of what lies between them; an event holds the enqueued
// count at its record and has completed once the stream's completed count reaches it.  A stream can be marked destroyed (a record on
// it fails) or stuck (it cannot be synchronised).  Nothing completes by itself: a case completes streams where it wants to, or runs a
// completer thread.
//
// Each case prints one line, "NAME ok" or "NAME FAILED"; the last line is "N failures", the exit status 0 when N is 0.
// tests/test_keyed_fence_host.py checks every line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "keyed_fence.h"

namespace {

// what a keyed launch reads: live until the retirer has drained it, poisoned from then on.  `poisoned` is a plain int on purpose: the
// fence's waits are all that orders the retirer's write behind the readers' reads, so the thread sanitizer sees a broken protocol as a race.
struct Table {
    int poisoned = 0;
};
struct FakeStream {
    std::mutex m;
    std::deque<const Table*> queued;      // launches between `completed` and `enqueued`, each with the table it will read
    uint64_t enqueued = 0;
    std::atomic<uint64_t> completed{0};
    bool destroyed = false, stuck = false;
    int records = 0, syncs = 0;           // what the fence asked of it
    std::atomic<int>* bad_reads = nullptr;
    void enqueue(const Table* t = nullptr) {
        std::lock_guard<std::mutex> lk(m);
        queued.push_back(t);
        enqueued++;
    }
    // the launches run, in order: each reads its table
    void complete_all() {
        std::lock_guard<std::mutex> lk(m);
        while (!queued.empty()) {
            if (queued.front() && queued.front()->poisoned && bad_reads) bad_reads->fetch_add(1);
            queued.pop_front();
            completed.fetch_add(1, std::memory_order_release);
        }
    }
};
struct FakeEvent {
    FakeStream* s = nullptr;
    uint64_t at = 0;
};
struct FakeDev {
    using Event = FakeEvent*;
    using Stream = FakeStream*;
    static int made, alive;
    static Event make_event() {
        made++;
        alive++;
        return new FakeEvent;
    }
    static void destroy_event(Event e) {
        alive--;
        delete e;
    }
    static bool record(Event e, Stream s) {
        std::lock_guard<std::mutex> lk(s->m);
        s->records++;
        if (s->destroyed) return false;
        e->s = s;
        e->at = s->enqueued;
        return true;
    }
    static fab::FenceQuery query(Event e) {
        return e->s->completed.load(std::memory_order_acquire) >= e->at ? fab::FenceQuery::DONE : fab::FenceQuery::NOT_READY;
    }
    static void wait(Event e) {
        const auto t0 = std::chrono::steady_clock::now();
        while (query(e) != fab::FenceQuery::DONE) {
            std::this_thread::yield();
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {      // (a case that waits for what nobody completes)
                fprintf(stderr, "FAILED: an event was waited for and never completed\n");
                exit(3);
            }
        }
    }
    static bool sync(Stream s) {
        {
            std::lock_guard<std::mutex> lk(s->m);
            s->syncs++;
            if (s->stuck) return false;
        }
        s->complete_all();
        return true;
    }
};
int FakeDev::made = 0;
int FakeDev::alive = 0;
using Fence = fab::KeyedFence<FakeDev>;

int g_bad = 0;
bool g_case_ok = true;
void expect(bool ok, const char* what, long i = 0) {
    if (ok) return;
    fprintf(stderr, "FAILED: %s (%ld)\n", what, i);
    g_case_ok = false;
}
void end_case(const char* name) {
    printf("%s %s\n", name, g_case_ok ? "ok" : "FAILED");
    if (!g_case_ok) g_bad++;
    g_case_ok = true;
}

void case_quiet() {
    Fence f;
    FakeStream s;
    expect(f.quiet(false) && f.quiet(true), "a fence nobody entered is quiet");
    {
        Fence::Ticket t = f.enter({&s});
        expect(!f.quiet(false), "not quiet while a ticket is alive");
        Fence::Ticket u = std::move(t);
        expect(!f.quiet(false), "a moved ticket still counts, once");
        Fence::Ticket t2 = f.enter({&s});
        u.release();
        expect(!f.quiet(false), "the second launcher is still counted");
        u.release();                      // (twice: nothing)
        expect(!f.quiet(false), "a ticket uncounts once");
    }
    expect(f.quiet(false), "quiet after the last ticket");
    // quiet(true) returns only after another thread has dropped its ticket
    std::atomic<bool> dropped{false};
    std::atomic<bool> entered{false};
    std::thread other([&] {
        Fence::Ticket t = f.enter({&s});
        entered.store(true);
        std::this_thread::sleep_for(std::chrono::milliseconds(30));
        dropped.store(true);
    });
    while (!entered.load()) std::this_thread::yield();
    const bool q = f.quiet(true);
    expect(q && dropped.load(), "quiet(true) outlasts the other thread's ticket");
    other.join();
    end_case("quiet");
}

void case_record() {
    Fence f;
    FakeStream own1, own2, foreign1, foreign2, extra, never;
    auto owned = [&](FakeStream* s) { return s == &own1 || s == &own2; };
    for (int k = 0; k < 5; k++) f.enter({&own1, &foreign1});      // (the tickets die at once)
    f.enter({&foreign1, &own2, &foreign2, &own1});
    std::vector<FakeEvent*> evs;
    expect(f.record(evs, owned, {&extra}), "record");
    expect(evs.size() == 5 && own1.records == 1 && own2.records == 1 && foreign1.records == 1 && foreign2.records == 1 && extra.records == 1 && never.records == 0,
           "one event per stream ever entered, each once, and one per extra stream");
    expect(f.record(evs, owned), "record without extra");
    expect(evs.size() == 9 && extra.records == 1 && own1.records == 2, "extra streams are not remembered");
    for (FakeStream* s : {&own1, &own2, &foreign1, &foreign2, &extra}) s->complete_all();
    expect(f.done(evs, false) && evs.empty(), "nothing was queued: done");
    // a destroyed foreign stream is forgotten, a destroyed own one is synchronised and kept
    foreign1.destroyed = true;
    own2.destroyed = true;
    own2.enqueue();
    expect(f.record(evs, owned) && evs.size() == 2, "two streams refuse");
    expect(foreign1.records == 3 && foreign1.syncs == 0, "the foreign one is not synchronised");
    expect(own2.records == 3 && own2.syncs == 1 && own2.completed.load() == 1, "the own one is synchronised: what it carried has run");
    expect(f.done(evs, false), "done");
    expect(f.record(evs, owned) && evs.size() == 2, "again");
    expect(foreign1.records == 3, "a forgotten stream is not asked again");
    expect(own2.records == 4 && own2.syncs == 2, "a kept one is");
    expect(f.done(evs, false), "done");
    f.enter({&foreign1});
    foreign1.destroyed = false;
    expect(f.record(evs, owned) && evs.size() == 3 && foreign1.records == 4, "a forgotten stream that is entered again is remembered again");
    expect(f.done(evs, false), "done");
    // a stuck own stream: false, and the others are recorded all the same
    own2.stuck = true;
    expect(!f.record(evs, owned) && evs.size() == 3, "an own stream that can neither be recorded on nor synchronised");
    expect(f.done(evs, false), "done");
    own2.stuck = false;
    extra.destroyed = extra.stuck = true;
    expect(!f.record(evs, owned, {&extra}), "an extra stream is an own one");
    expect(f.done(evs, false), "done");
    f.destroy_all();
    expect(FakeDev::alive == 0, "every event went back to the pool");
    end_case("record");
}

void case_done() {
    Fence f;
    FakeStream a, b, c;
    auto owned = [](FakeStream*) { return false; };
    f.enter({&a, &b, &c});
    a.enqueue();
    a.enqueue();
    b.enqueue();
    std::vector<FakeEvent*> evs;
    f.record(evs, owned);
    a.enqueue();                           // (behind the record: not waited for)
    expect(evs.size() == 3 && !f.done(evs, false), "two streams have work in front of the record");
    b.complete_all();
    expect(!f.done(evs, false), "one of them still has");
    {
        std::lock_guard<std::mutex> lk(a.m);      // one of the two launches in front of the record
        a.queued.pop_front();
        a.completed.fetch_add(1);
    }
    expect(!f.done(evs, false) && !evs.empty(), "up to the recorded point, not short of it");
    {
        std::lock_guard<std::mutex> lk(a.m);
        a.queued.pop_front();
        a.completed.fetch_add(1);
    }
    expect(f.done(evs, false) && evs.empty(), "done at the recorded point, whatever was queued behind it");
    expect(a.queued.size() == 1, "the launch behind the record has not run");
    expect(f.done(evs, true), "an empty list is done");
    f.destroy_all();
    expect(FakeDev::alive == 0, "every event went back to the pool");
    end_case("done");
}

void case_pooling() {
    Fence f;
    FakeStream s[3];
    auto owned = [](FakeStream*) { return false; };
    f.enter({&s[0], &s[1], &s[2]});
    const int made0 = FakeDev::made;
    int outstanding_max = 0;
    std::vector<FakeEvent*> a, b;
    for (int round = 0; round < 200; round++) {
        for (auto& x : s) x.enqueue();
        f.record(a, owned);
        if (round % 3 == 0) f.record(b, owned, {&s[0]});      // two lists at once, every third round
        outstanding_max = std::max(outstanding_max, (int)(a.size() + b.size()));
        expect(!f.done(a, false), "not done", round);
        for (auto& x : s) x.complete_all();
        expect(f.done(a, false) && f.done(b, round % 2 == 0), "done", round);
    }
    FakeEvent* e = f.get();                                   // (an event for a pending list comes from the same pool)
    expect(e != nullptr && FakeDev::made - made0 == outstanding_max, "get() hands out a pooled event");
    f.put(e);
    expect(outstanding_max == 7 && FakeDev::made - made0 == outstanding_max, "as many events ever made as were ever outstanding at once");
    f.destroy_all();
    expect(FakeDev::alive == 0, "destroy_all");
    end_case("pooling");
}

// a list of drains the way the product keeps them: a slot, its events, whether they were recorded yet
struct Drain {
    int slot;
    bool recorded = false;
    std::vector<FakeEvent*> evs;
};
void case_drain_loops() {
    Fence f;
    FakeStream s0, s1;
    auto owned = [](FakeStream*) { return false; };
    std::vector<bool> draining(8, false);
    int stepped_with_wait = 0;
    auto step = [&](Drain& d, bool wait) {
        if (wait) {
            stepped_with_wait++;
            s0.complete_all();             // (what a device does by itself)
            s1.complete_all();
        }
        if (!d.recorded) {
            if (!f.quiet(wait)) return false;
            f.record(d.evs, owned);
            d.recorded = true;
        }
        if (!f.done(d.evs, wait)) return false;
        draining[(size_t)d.slot] = false;
        return true;
    };
    // what the product's two "wait for the drain of slot k" functions answer
    std::vector<Drain> drains;
    auto wait_slot = [&](int slot) { return Fence::wait_for(drains, [&](const Drain& d) { return d.slot == slot; }, step) && !draining[(size_t)slot]; };
    auto slots = [&] {
        std::vector<int> v;
        for (auto& d : drains) v.push_back(d.slot);
        return v;
    };
    f.enter({&s0, &s1});
    for (int k = 0; k < 5; k++) {
        drains.push_back(Drain{k});
        draining[(size_t)k] = true;
    }
    // drains 0 and 1 record now, behind one launch on s0; 2 .. 4 cannot: a launcher is under way
    s0.enqueue();
    Fence::advance(drains, [&](Drain& d, bool wait) { return d.slot < 2 ? step(d, wait) : false; });
    expect(slots() == std::vector<int>({0, 1, 2, 3, 4}) && drains[0].recorded && drains[1].recorded && !drains[2].recorded, "nothing finished, two recorded");
    {
        Fence::Ticket t = f.enter({&s0});
        s0.complete_all();
        Fence::advance(drains, step);
        expect(slots() == std::vector<int>({2, 3, 4}), "advance erases the finished drains and keeps the order of the rest");
        expect(!drains[0].recorded && !draining[0] && !draining[1] && draining[2], "a launcher postpones the others");
    }
    s1.enqueue();
    Fence::advance(drains, step);
    expect(slots() == std::vector<int>({2, 3, 4}) && drains[0].recorded && drains[2].recorded, "recorded behind a launch that has not run");
    expect(stepped_with_wait == 0, "advance never waits");
    // wait_for: the matching drain all the way, the others as they were
    const size_t n3 = drains[1].evs.size();
    expect(wait_slot(3) && stepped_with_wait == 1, "wait_for runs the matching drain with wait");
    expect(slots() == std::vector<int>({2, 4}) && !draining[3] && draining[2] && draining[4], "and erases it alone");
    expect(drains[0].evs.size() == n3 && drains[1].evs.size() == n3 && n3 == 2, "the others' events were not asked");
    // nothing matches: true if the slot is not draining, false if it is (its drain is lost: the product answers FABGPU_ELAUNCH)
    expect(wait_slot(3) && wait_slot(7), "no drain and not draining");
    draining[6] = true;
    expect(!wait_slot(6) && stepped_with_wait == 1, "no drain, but draining");
    // a step that does not finish even with wait (the P-256 generation write can fail): false, and the drain stays
    expect(!Fence::wait_for(drains, [](const Drain& d) { return d.slot == 4; }, [](Drain&, bool) { return false; }), "a drain that cannot finish");
    expect(slots() == std::vector<int>({2, 4}), "stays in the list");
    s0.complete_all();
    s1.complete_all();
    Fence::advance(drains, step);
    expect(drains.empty(), "everything drains in the end");
    f.destroy_all();
    expect(FakeDev::alive == 0, "every event went back to the pool");
    end_case("drain_loops");
}

// 8 launchers on 4 streams read the table a shared cell names, under the rules of keyed_fence.h; one retirer swaps the cell and drains
// the old table through quiet / record / done - waiting all the way on even rounds, asking and letting go of the book's lock on odd
// ones - while a completer runs what the launchers queued.  Neither a launcher nor a queued launch may ever read a poisoned table.
void case_protocol() {
    constexpr int LAUNCHERS = 8, STREAMS = 4, ROUNDS = 3000;
    Fence f;
    FakeStream st[STREAMS];
    std::atomic<int> bad_reads{0};
    for (auto& s : st) s.bad_reads = &bad_reads;
    auto owned = [](FakeStream*) { return true; };
    std::mutex book;
    std::vector<std::unique_ptr<Table>> tables;      // (kept to the end: a poisoned table must stay readable to be caught)
    tables.emplace_back(new Table);
    Table* cell = tables.back().get();               // guarded by `book`
    std::atomic<bool> stop{false};
    std::atomic<long> launches{0};
    std::vector<std::thread> threads;
    for (int l = 0; l < LAUNCHERS; l++)
        threads.emplace_back([&, l] {
            for (long k = 0; !stop.load(std::memory_order_relaxed); k++) {
                FakeStream* s = &st[(l + k) % STREAMS];
                const Table* view;
                Fence::Ticket t;
                {
                    std::lock_guard<std::mutex> lk(book);
                    view = cell;
                    t = f.enter({s});
                }
                if (view->poisoned) bad_reads.fetch_add(1);
                s->enqueue(view);
                launches.fetch_add(1, std::memory_order_relaxed);
            }      // (the ticket dies behind the enqueue)
        });
    std::thread completer([&] {
        while (!stop.load(std::memory_order_relaxed)) {
            for (auto& s : st) s.complete_all();
            std::this_thread::yield();
        }
        for (auto& s : st) s.complete_all();
    });
    long seen = 0;
    for (int r = 0; r < ROUNDS; r++) {
        std::vector<FakeEvent*> evs;
        Table* old;
        while (launches.load(std::memory_order_relaxed) == seen) std::this_thread::yield();      // every table is retired under traffic
        seen = launches.load(std::memory_order_relaxed);
        if (r % 2 == 0) {
            std::lock_guard<std::mutex> lk(book);
            old = cell;
            tables.emplace_back(new Table);
            cell = tables.back().get();
            f.quiet(true);
            expect(f.record(evs, owned), "record", r);
            expect(f.done(evs, true), "done", r);
        } else {
            {
                std::lock_guard<std::mutex> lk(book);
                old = cell;
                tables.emplace_back(new Table);
                cell = tables.back().get();
            }
            for (bool recorded = false;;) {
                {
                    std::lock_guard<std::mutex> lk(book);
                    if (!recorded && f.quiet(false)) {
                        expect(f.record(evs, owned), "record", r);
                        recorded = true;
                    }
                    if (recorded && f.done(evs, false)) break;
                }
                std::this_thread::yield();
            }
        }
        old->poisoned = 1;
    }
    stop.store(true);
    for (auto& t : threads) t.join();
    completer.join();
    expect(bad_reads.load() == 0, "a poisoned table was read", bad_reads.load());
    expect(launches.load() > 0, "the launchers ran");
    {
        std::lock_guard<std::mutex> lk(book);
        f.destroy_all();
    }
    expect(FakeDev::alive == 0, "every event went back to the pool");
    end_case("protocol");
}

}  // namespace

int main() {
    case_quiet();
    case_record();
    case_done();
    case_pooling();
    case_drain_loops();
    case_protocol();
    printf("%d failures\n", g_bad);
    return g_bad ? 1 : 0;
}
