// The verdict memo of the P-384 tuples of a block pass: a table of its own beside the P-256 memo (bccsp_host.h BlockMemo),
// seeded on the host by GPUCSP::P384PassStage and asked by bccsp.Verify(k, sig, digest) for a P-384 key (fabgpu_csp_memo_lookup_p384).
//
// One record per block: its entries' framed keys back to back with an offsets array, a status byte per entry and an open-addressed index
// (entry + 1; linear probing, at most half full) over a hash of (sig, digest).  A key is
//     X48 || Y48 || u32 siglen || sig || u32 dlen || digest
// - the lengths frame the two ragged parts, so (sig || d[:k], d[k:]) never reads as (sig, d).  A hit is decided by comparing the whole
// key; the hash only chooses where to look.  A key seeded twice keeps both entries and answers with the first (it sits nearer the hash's
// slot), as the P-256 host seeding does.
// The records live in a deque, oldest first, under a reader lock of their own (reader_lock.h: readers share no cache line); the table is
// bounded by a capacity in entries and the oldest BLOCK goes first while it is over.
//
// Pure host code over bytes: no provider state, no device, nothing of the P-256 memo.  csrc/hosttest_p384_memo.cpp drives it alone.
#pragma once
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "reader_lock.h"

namespace fab {
namespace bccsp {
struct TestAccess;   // testhooks.cpp (libfabgpu_testhooks.so): edits a stored status to show that the audit sees it
}

class P384Memo {
   public:
    static constexpr size_t kMaxPart = 1024;                 // longest signature / digest a lookup takes (as the P-256 memo)
    static constexpr size_t kDefaultCapacity = (size_t)1 << 16;
    static size_t KeyBytes(size_t siglen, size_t dlen) { return 96 + 4 + siglen + 4 + dlen; }
    static void KeyWrite(uint8_t* k, const uint8_t* qx48, const uint8_t* qy48, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen) {
        const uint32_t sl = (uint32_t)siglen, dl = (uint32_t)dlen;
        memcpy(k, qx48, 48);
        memcpy(k + 48, qy48, 48);
        memcpy(k + 96, &sl, 4);
        memcpy(k + 100, sig, siglen);
        memcpy(k + 100 + siglen, &dl, 4);
        memcpy(k + 104 + siglen, digest, dlen);
    }
    // slot choice only: the digest is SHA-256 output whatever the sender of the block does, mixed with the tail of the signature
    // (the mix of GPUCSP::MemoHash)
    static uint64_t Hash(const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen) {
        uint64_t a = 0, b = 0;
        memcpy(&a, digest, dlen < 8 ? dlen : 8);
        memcpy(&b, sig + (siglen > 8 ? siglen - 8 : 0), siglen < 8 ? siglen : 8);
        const uint64_t h = (a ^ (b * 0x9E3779B97F4A7C15ull)) * 0xD6E8FEB86659FD93ull;
        return h ^ (h >> 32);
    }
    static bool Askable(const uint8_t* qx48, const uint8_t* qy48, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen) {
        return qx48 && qy48 && sig && digest && siglen != 0 && dlen != 0 && siglen <= kMaxPart && dlen <= kMaxPart;
    }

    // The entries of one block.  Add() in tuple order, Seal() once, then Publish(); nothing is written after that.
    class Record {
       public:
        Record(uint64_t block_seq, size_t expect_entries) : seq_(block_seq) {
            key_off_.reserve(expect_entries + 1);
            status_.reserve(expect_entries);
            keys_.reserve(expect_entries * KeyBytes(104, 32));
            key_off_.push_back(0);
        }
        // false: not an entry a lookup could ask for (an empty or oversized part), or the record is full (4 GiB of keys)
        bool Add(const uint8_t* qx48, const uint8_t* qy48, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen, uint8_t status) {
            if (sealed_ || !Askable(qx48, qy48, sig, siglen, digest, dlen)) return false;
            const size_t kl = KeyBytes(siglen, dlen), at = keys_.size();
            if (at + kl > 0xFFFFFFF0ull) return false;
            keys_.resize(at + kl);
            KeyWrite(keys_.data() + at, qx48, qy48, sig, siglen, digest, dlen);
            key_off_.push_back((uint32_t)(at + kl));
            status_.push_back(status);
            return true;
        }
        void Seal() {
            if (sealed_) return;
            sealed_ = true;
            const uint32_t n = size();
            if (!n) return;
            uint32_t cap = 16;
            while (cap < 2 * (uint64_t)n) cap <<= 1;
            mask_ = cap - 1;
            slots_.assign(cap, 0u);
            for (uint32_t e = 0; e < n; e++) {
                uint32_t at = (uint32_t)HashOfEntry(e) & mask_;
                while (slots_[at]) at = (at + 1) & mask_;    // (at most half full: an empty slot comes)
                slots_[at] = e + 1;
            }
        }
        uint32_t size() const { return (uint32_t)status_.size(); }
        uint64_t seq() const { return seq_; }
        uint64_t gen() const { return gen_; }

       private:
        friend class P384Memo;
        friend struct bccsp::TestAccess;
        uint64_t HashOfEntry(uint32_t e) const {
            const uint8_t* k = keys_.data() + key_off_[e];
            uint32_t sl, dl;
            memcpy(&sl, k + 96, 4);
            memcpy(&dl, k + 100 + sl, 4);
            return Hash(k + 100, sl, k + 104 + sl, dl);
        }
        bool Same(uint32_t e, const uint8_t* key, size_t kl) const {
            const uint32_t o = key_off_[e];
            return key_off_[e + 1] - o == kl && memcmp(keys_.data() + o, key, kl) == 0;
        }
        // entry + 1 of the first entry that holds exactly this key, 0: none
        uint32_t Find(const uint8_t* key, size_t kl, uint64_t h) const {
            if (slots_.empty()) return 0;
            for (uint32_t probe = 0, at = (uint32_t)h & mask_; probe <= mask_; probe++, at = (at + 1) & mask_) {
                const uint32_t e = slots_[at];
                if (!e) return 0;
                if (Same(e - 1, key, kl)) return e;
            }
            return 0;
        }
        uint64_t seq_, gen_ = 0;
        bool sealed_ = false;
        std::vector<uint8_t> keys_, status_;
        std::vector<uint32_t> key_off_, slots_;
        uint32_t mask_ = 0;
    };

    // Pushes the record under the write lock and drops the oldest blocks while the table is over capacity (the newest always stays).
    // false: nothing was published - the record is empty, or `refuse` (the provider's poison flag), read under the lock, is set.
    bool Publish(std::shared_ptr<Record> rec, const std::atomic<bool>* refuse = nullptr) {
        if (!rec || !rec->size()) return false;
        rec->Seal();
        rec->gen_ = NextGen();
        std::unique_lock<BigReaderLock> lk(mu_);
        if (refuse && refuse->load(std::memory_order_acquire)) return false;
        blocks_.push_back(std::move(rec));
        size_t total = 0;
        for (const auto& b : blocks_) total += b->size();
        while (total > cap_ && blocks_.size() > 1) {
            total -= blocks_.front()->size();
            evicted_.fetch_add(blocks_.front()->size(), std::memory_order_relaxed);
            blocks_.pop_front();
        }
        return true;
    }
    // 0: hit (*status, *block_seq and *entry - the entry's place in its record - are set, each may be null); 1: miss
    int Lookup(const uint8_t* qx48, const uint8_t* qy48, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen, uint8_t* status,
               uint64_t* block_seq = nullptr, uint32_t* entry = nullptr) const {
        if (!Askable(qx48, qy48, sig, siglen, digest, dlen)) return 1;
        uint8_t key[96 + 8 + 2 * kMaxPart];
        const size_t kl = KeyBytes(siglen, dlen);
        KeyWrite(key, qx48, qy48, sig, siglen, digest, dlen);
        std::shared_lock<BigReaderLock> lk(mu_);
        auto hit = [&](const Record& r, uint32_t e) {
            if (status) *status = r.status_[e - 1];
            if (block_seq) *block_seq = r.seq_;
            if (entry) *entry = e - 1;
            last_gen() = r.gen_;
            hits_.add(1);
            return 0;
        };
        // A validator thread works through one block at a time: the record that answered its last lookup is asked first, whatever its
        // age.  A hint and nothing more - a thread that moved to another block falls through to the others, newest first.
        const uint64_t h = Hash(sig, siglen, digest, dlen);
        const Record* hinted = nullptr;
        if (const uint64_t g = last_gen())
            for (const auto& b : blocks_)
                if (b->gen_ == g) hinted = b.get();
        if (hinted)
            if (const uint32_t e = hinted->Find(key, kl, h)) return hit(*hinted, e);
        for (auto it = blocks_.rbegin(); it != blocks_.rend(); ++it) {   // newest block first
            if (it->get() == hinted) continue;
            if (const uint32_t e = (*it)->Find(key, kl, h)) return hit(**it, e);
        }
        misses_.add(1);
        return 1;
    }
    size_t HasBlock(uint64_t block_seq) const {
        std::shared_lock<BigReaderLock> lk(mu_);
        size_t n = 0;
        for (const auto& b : blocks_)
            if (b->seq_ == block_seq) n += b->size();
        return n;
    }
    size_t EvictBlock(uint64_t block_seq) {
        std::unique_lock<BigReaderLock> lk(mu_);
        size_t gone = 0;
        for (auto b = blocks_.begin(); b != blocks_.end();) {
            if ((*b)->seq_ != block_seq) { ++b; continue; }
            gone += (*b)->size();
            b = blocks_.erase(b);
        }
        evicted_.fetch_add(gone, std::memory_order_relaxed);
        return gone;
    }
    void Stats(uint64_t* entries, uint64_t* hits, uint64_t* misses, uint64_t* evicted) const {
        std::shared_lock<BigReaderLock> lk(mu_);
        uint64_t n = 0;
        for (const auto& b : blocks_) n += b->size();
        if (entries) *entries = n;
        if (hits) *hits = hits_.load();
        if (misses) *misses = misses_.load();
        if (evicted) *evicted = evicted_.load(std::memory_order_relaxed);
    }
    // takes effect with the next Publish, as the P-256 memo's capacity does
    void SetCapacity(size_t max_entries) {
        std::unique_lock<BigReaderLock> lk(mu_);
        cap_ = max_entries ? max_entries : 1;
    }

   private:
    friend struct bccsp::TestAccess;
    static uint64_t& last_gen() {                            // Record::gen of the record this thread's last hit came from (0: none)
        static thread_local uint64_t g = 0;
        return g;
    }
    static uint64_t NextGen() {
        static std::atomic<uint64_t> g{1};
        return g.fetch_add(1, std::memory_order_relaxed);
    }
    mutable BigReaderLock mu_;
    std::deque<std::shared_ptr<Record>> blocks_;             // oldest first
    size_t cap_ = kDefaultCapacity;
    mutable ShardedCounter hits_, misses_;
    std::atomic<uint64_t> evicted_{0};
};

}  // namespace fab
