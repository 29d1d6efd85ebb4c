// Stand-alone host program over P384Memo (p384_memo.h; its own main; built by the Makefile as ../lib/hosttest_p384_memo, and as
// ../lib/hosttest_p384_memo_san with -fsanitize=address,undefined by `make sanitize-p384-memo`).  The table is a pure function of bytes,
// so it runs here without a provider and without a device.
//
// With a file name: the file is a script, one command per line, binary values in hex; one answer line per command on stdout.
//     cap N                        -> ok
//     begin SEQ N                  -> ok                      (a new record for block SEQ, N entries expected)
//     add QX QY SIG DIGEST STATUS  -> ok | refused
//     publish                      -> published N | refused   (N: entries of the record)
//     lookup QX QY SIG DIGEST      -> hit STATUS SEQ | miss
//     has SEQ                      -> has N
//     evict SEQ                    -> evicted N
//     stats                        -> stats ENTRIES HITS MISSES EVICTED
// tests/test_p384_memo_host.py writes such scripts and checks every answer.  Each looked-up part lives in a heap buffer of exactly its
// length, so that a read past its end is the sanitizer's to see.
// Without arguments: the same cases made here from a seeded generator (hits over the DER range of signature lengths, single-bit and
// length near misses, the framing pair, duplicates, capacity, evicting what is not held) and, last, lookups from four threads while a
// fifth publishes and evicts.  Exit status 0 and "0 failures": everything answered as it must.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "p384_memo.h"

using fab::P384Memo;

namespace {
typedef std::vector<uint8_t> Bytes;

bool unhex(const std::string& s, Bytes& out) {
    out.clear();
    if (s == "-") return true;                              // (an empty value)
    if (s.size() % 2) return false;
    auto nib = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
    for (size_t i = 0; i < s.size(); i += 2) {
        const int a = nib(s[i]), b = nib(s[i + 1]);
        if (a < 0 || b < 0) return false;
        out.push_back((uint8_t)(a << 4 | b));
    }
    return true;
}
// exactly these bytes on the heap, nothing behind them
struct Exact {
    uint8_t* p;
    size_t n;
    explicit Exact(const Bytes& b) : p((uint8_t*)malloc(b.size() ? b.size() : 1)), n(b.size()) {
        if (n) memcpy(p, b.data(), n);
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};
int lookup(const P384Memo& m, const Bytes& qx, const Bytes& qy, const Bytes& sig, const Bytes& dg, uint8_t* st, uint64_t* seq) {
    if (qx.size() != 48 || qy.size() != 48) return 1;
    Exact x(qx), y(qy), s(sig), d(dg);
    return m.Lookup(x.p, y.p, s.p, s.n, d.p, d.n, st, seq);
}

int run_script(const char* path) {
    std::ifstream in(path);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    P384Memo memo;
    std::shared_ptr<P384Memo::Record> rec;
    std::string line;
    size_t ln = 0;
    while (std::getline(in, line)) {
        ln++;
        std::istringstream ss(line);
        std::string cmd;
        if (!(ss >> cmd) || cmd[0] == '#') continue;
        if (cmd == "cap") {
            unsigned long long n = 0;
            ss >> n;
            memo.SetCapacity((size_t)n);
            puts("ok");
        } else if (cmd == "begin") {
            unsigned long long seq = 0, n = 0;
            ss >> seq >> n;
            rec = std::make_shared<P384Memo::Record>((uint64_t)seq, (size_t)n);
            puts("ok");
        } else if (cmd == "add" || cmd == "lookup") {
            std::string f[4];
            Bytes b[4];
            unsigned status = 0;
            ss >> f[0] >> f[1] >> f[2] >> f[3];
            if (cmd == "add") ss >> status;
            bool ok = !ss.fail();
            for (int k = 0; k < 4 && ok; k++) ok = unhex(f[k], b[k]);
            if (!ok || (cmd == "add" && !rec)) {
                fprintf(stderr, "line %zu: malformed\n", ln);
                return 2;
            }
            if (cmd == "add") {
                Exact x(b[0]), y(b[1]), s(b[2]), d(b[3]);
                puts(b[0].size() == 48 && b[1].size() == 48 && rec->Add(x.p, y.p, s.p, s.n, d.p, d.n, (uint8_t)status) ? "ok" : "refused");
            } else {
                uint8_t st = 0xFF;
                uint64_t seq = 0;
                if (lookup(memo, b[0], b[1], b[2], b[3], &st, &seq) == 0) printf("hit %u %llu\n", (unsigned)st, (unsigned long long)seq);
                else puts("miss");
            }
        } else if (cmd == "publish") {
            const uint32_t n = rec ? rec->size() : 0;
            if (rec && memo.Publish(rec)) printf("published %u\n", n);
            else puts("refused");
            rec.reset();
        } else if (cmd == "has" || cmd == "evict") {
            unsigned long long seq = 0;
            ss >> seq;
            if (cmd == "has") printf("has %zu\n", memo.HasBlock(seq));
            else printf("evicted %zu\n", memo.EvictBlock(seq));
        } else if (cmd == "stats") {
            uint64_t v[4];
            memo.Stats(&v[0], &v[1], &v[2], &v[3]);
            printf("stats %llu %llu %llu %llu\n", (unsigned long long)v[0], (unsigned long long)v[1], (unsigned long long)v[2], (unsigned long long)v[3]);
        } else {
            fprintf(stderr, "line %zu: unknown command %s\n", ln, cmd.c_str());
            return 2;
        }
    }
    return 0;
}

// ---- the cases made here ----
struct Rng {
    uint64_t s;
    uint64_t next() {                                      // splitmix64
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    Bytes bytes(size_t n) {
        Bytes b(n);
        for (auto& v : b) v = (uint8_t)next();
        return b;
    }
};
struct Entry {
    Bytes qx, qy, sig, dg;
    uint8_t status;
};
int g_bad = 0;
void expect(bool ok, const char* what, size_t i) {
    if (ok) return;
    fprintf(stderr, "FAILED: %s (entry %zu)\n", what, i);
    g_bad++;
}
bool add(P384Memo::Record& r, const Entry& e) { return r.Add(e.qx.data(), e.qy.data(), e.sig.data(), e.sig.size(), e.dg.data(), e.dg.size(), e.status); }
bool hits(const P384Memo& m, const Entry& e, uint8_t want, uint64_t want_seq) {
    uint8_t st = 0xFF;
    uint64_t seq = ~0ull;
    return lookup(m, e.qx, e.qy, e.sig, e.dg, &st, &seq) == 0 && st == want && seq == want_seq;
}
bool misses(const P384Memo& m, const Bytes& qx, const Bytes& qy, const Bytes& sig, const Bytes& dg) {
    uint8_t st = 0xFF;
    return lookup(m, qx, qy, sig, dg, &st, nullptr) == 1 && st == 0xFF;
}
std::vector<Entry> make_entries(Rng& g, size_t n) {
    std::vector<Entry> v(n);
    for (size_t i = 0; i < n; i++) v[i] = {g.bytes(48), g.bytes(48), g.bytes(8 + i % 97), g.bytes(i & 1 ? 48 : 32), (uint8_t)(i % 4)};
    return v;
}

int self_test() {
    Rng g{384};
    size_t asked = 0;
    {   // hits and near misses: 257 entries, signatures of 8 .. 104 bytes, digests of 32 and 48
        P384Memo m;
        const std::vector<Entry> es = make_entries(g, 257);
        auto rec = std::make_shared<P384Memo::Record>(7, es.size());
        for (size_t i = 0; i < es.size(); i++) expect(add(*rec, es[i]), "an entry is taken", i);
        expect(m.Publish(rec), "the record is published", 0);
        for (size_t i = 0; i < es.size(); i++) {
            const Entry& e = es[i];
            expect(hits(m, e, e.status, 7), "an entry hits with its own status", i);
            for (int part = 0; part < 4; part++) {
                Entry f = e;
                Bytes& b = part == 0 ? f.qx : part == 1 ? f.qy : part == 2 ? f.sig : f.dg;
                b[g.next() % b.size()] ^= (uint8_t)(1u << (g.next() & 7));
                expect(misses(m, f.qx, f.qy, f.sig, f.dg), "a flipped bit misses", i);
            }
            Bytes shorter(e.sig.begin(), e.sig.end() - 1), longer = e.sig;
            longer.push_back(0);
            expect(misses(m, e.qx, e.qy, shorter, e.dg), "siglen - 1 misses", i);
            expect(misses(m, e.qx, e.qy, longer, e.dg), "siglen + 1 misses", i);
            asked += 7;
        }
        uint64_t v[4];
        m.Stats(&v[0], &v[1], &v[2], &v[3]);
        expect(v[0] == 257 && v[1] == 257 && v[2] == 6 * 257 && v[3] == 0, "the counters add up", 0);
        expect(misses(m, es[0].qx, es[0].qy, Bytes(), es[0].dg) && misses(m, es[0].qx, es[0].qy, es[0].sig, Bytes()), "an empty part misses", 0);
        expect(misses(m, es[0].qx, es[0].qy, Bytes(1025, 1), es[0].dg), "an oversized part misses", 0);
    }
    {   // framing: sig || digest equal, split differently
        P384Memo m;
        const Bytes qx = g.bytes(48), qy = g.bytes(48), all = g.bytes(72);
        const Entry a = {qx, qy, Bytes(all.begin(), all.begin() + 40), Bytes(all.begin() + 40, all.end()), 0};
        const Entry b = {qx, qy, Bytes(all.begin(), all.begin() + 24), Bytes(all.begin() + 24, all.end()), 1};
        auto rec = std::make_shared<P384Memo::Record>(1, 1);
        add(*rec, a);
        m.Publish(rec);
        expect(hits(m, a, 0, 1) && misses(m, b.qx, b.qy, b.sig, b.dg), "the other split of the same bytes misses", 0);
        rec = std::make_shared<P384Memo::Record>(2, 1);
        add(*rec, b);
        m.Publish(rec);
        expect(hits(m, a, 0, 1) && hits(m, b, 1, 2), "the two splits do not alias", 0);
    }
    {   // duplicates keep the first
        P384Memo m;
        Entry e = make_entries(g, 1)[0];
        auto rec = std::make_shared<P384Memo::Record>(3, 2);
        e.status = 1;
        add(*rec, e);
        Entry again = e;
        again.status = 0;
        add(*rec, again);
        m.Publish(rec);
        expect(hits(m, e, 1, 3) && m.HasBlock(3) == 2, "a key seeded twice answers with the first status", 0);
    }
    {   // capacity: four blocks of 100 with room for 250; evicting what is not held
        P384Memo m;
        m.SetCapacity(250);
        std::vector<std::vector<Entry>> blocks;
        for (uint64_t b = 0; b < 4; b++) {
            blocks.push_back(make_entries(g, 100));
            auto rec = std::make_shared<P384Memo::Record>(10 + b, 100);
            for (const Entry& e : blocks.back()) add(*rec, e);
            m.Publish(rec);
        }
        uint64_t v[4];
        m.Stats(&v[0], nullptr, nullptr, &v[3]);
        expect(v[0] == 200 && v[3] == 200, "200 entries stay, 200 were evicted", 0);
        for (uint64_t b = 0; b < 4; b++) {
            expect(m.HasBlock(10 + b) == (b < 2 ? 0u : 100u), "only the newest two blocks stay, whole", (size_t)b);
            for (size_t i = 0; i < 100; i++) {
                const Entry& e = blocks[b][i];
                expect(b < 2 ? misses(m, e.qx, e.qy, e.sig, e.dg) : hits(m, e, e.status, 10 + b), "entries of a block leave together", i);
            }
        }
        expect(m.EvictBlock(99) == 0, "evicting a block that is not held returns 0", 0);
        expect(m.EvictBlock(12) == 100 && m.HasBlock(12) == 0 && m.HasBlock(13) == 100, "evicting a held block drops it alone", 0);
        expect(!m.Publish(std::make_shared<P384Memo::Record>(50, 0)), "an empty record is not published", 0);
        std::atomic<bool> refuse{true};
        auto rec = std::make_shared<P384Memo::Record>(51, 1);
        add(*rec, blocks[0][0]);
        expect(!m.Publish(rec, &refuse) && m.HasBlock(51) == 0, "a refused record is not published", 0);
    }
    {   // four readers while a writer publishes and evicts: block 1 stays throughout and always hits
        P384Memo m;
        m.SetCapacity(64);
        const std::vector<Entry> keep = make_entries(g, 16), churn = make_entries(g, 16);
        auto rec = std::make_shared<P384Memo::Record>(1, keep.size());
        for (const Entry& e : keep) add(*rec, e);
        m.Publish(rec);
        std::atomic<bool> stop{false};
        std::atomic<int> wrong{0};
        std::vector<std::thread> readers;
        for (int t = 0; t < 4; t++)
            readers.emplace_back([&] {
                while (!stop.load(std::memory_order_acquire))
                    for (const Entry& e : keep) {
                        if (!hits(m, e, e.status, 1)) wrong.fetch_add(1);
                        uint8_t st;
                        (void)m.Lookup(churn[0].qx.data(), churn[0].qy.data(), churn[0].sig.data(), churn[0].sig.size(), churn[0].dg.data(), churn[0].dg.size(), &st);
                    }
            });
        for (uint64_t round = 0; round < 200; round++) {
            auto r2 = std::make_shared<P384Memo::Record>(2, churn.size());
            for (const Entry& e : churn) add(*r2, e);
            m.Publish(r2);
            m.EvictBlock(2);
        }
        stop.store(true, std::memory_order_release);
        for (auto& t : readers) t.join();
        expect(wrong.load() == 0 && m.HasBlock(1) == 16 && m.HasBlock(2) == 0, "readers beside a writer see block 1 whole", 0);
    }
    printf("hosttest_p384_memo: %zu lookups of the first case and four more cases, %d failures\n", asked, g_bad);
    return g_bad ? 1 : 0;
}
}  // namespace

int main(int argc, char** argv) { return argc > 1 ? run_script(argv[1]) : self_test(); }
