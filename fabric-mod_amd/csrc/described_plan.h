// The span plan of a DESCRIBED batch (include/fabgpu.h: fabgpu_identity_batch, fabgpu_identity_batch_p384): which bytes of the caller's
// arena its messages, prefixes, pseudonym messages and gathered pieces reference, whether anything addresses the tail, and the offsets
// as the device will see them.  This is the only place where a caller's untrusted offsets turn into device offsets.  Pure host code - no
// HIP, no context - so that every refusal and every rebased offset is checked on the CPU (hosttest_described_plan.cpp,
// tests/test_described_plan_host.py).
//
//   spans at or above tail_base address the tail (tail[offset - tail_base]); a span may not straddle tail_base or leave the tail;
//   an empty span references nothing and carries no address; consecutive offsets bound the span even where a message is empty.
//
// Two policies are the entry's: whether a PREFIX may lie in the tail (see()'s may_be_tail - no entry allows it), and where the tail
// lies on the device (Tail).  Feed it, close() it, read rc / lo / hi / tail_used / span(), then rebase().
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/fabgpu.h"

namespace fab {

struct DescribedPlan {
    // IN_ARENA (P-256): the tail is written into the device arena at tail_base, so a used tail pins lo to 0 - tail_base stays an absolute
    // offset of the device arena.  OWN_BUFFER (P-384): the tail lies in a buffer of its own and the arena's spans move down by lo as ever.
    // Either way a tail span's offsets are handed on as they are.
    enum Tail { IN_ARENA, OWN_BUFFER };
    const Tail place;
    const bool spans;
    uint32_t tail_base = 0xFFFFFFFFu, tail_len = 0;       // (0xFFFFFFFF: no tail - nothing lies at or above it)
    uint32_t lo = 0xFFFFFFFFu, hi = 0;                    // of the caller's arena
    bool tail_used = false;
    uint64_t gather_total = 0;                            // bytes of the stitched gather messages
    int rc = FABGPU_OK;                                   // the refusal, if any; FABGPU_EINVAL outranks the gather total's FABGPU_ETOOBIG

    // tail preconditions: tail_base a multiple of 64, the spans flag, tail_base + tail_len within 0xFFFFFFF0
    DescribedPlan(Tail where, bool pairs, const void* tail, uint32_t tbase, uint32_t tlen) : place(where), spans(pairs) {
        if (tail == nullptr || tlen == 0) return;
        tail_base = tbase;
        tail_len = tlen;
        if ((tbase & 63u) || !pairs || (uint64_t)tbase + tlen > 0xFFFFFFF0ull) rc = FABGPU_EINVAL;
    }
    void see(uint32_t s0, uint32_t s1, bool may_be_tail) {
        if (s1 < s0) { rc = FABGPU_EINVAL; return; }
        if (s1 == s0) return;
        if (s0 >= tail_base) {
            if (!may_be_tail || (uint64_t)s1 > (uint64_t)tail_base + tail_len) rc = FABGPU_EINVAL;
            tail_used = true;
            return;
        }
        if (s1 > tail_base) { rc = FABGPU_EINVAL; return; }   // straddles
        bound(s0, s1);
    }
    // k rows in the batch's form: (start, end) pairs, or k + 1 consecutive offsets (empty messages still bound the span)
    void see_rows(const uint32_t* o, size_t k, bool may_be_tail) {
        for (size_t i = 0; i < k; i++) {
            if (spans) {
                see(o[2 * i], o[2 * i + 1], may_be_tail);
            } else {
                if (o[i + 1] < o[i]) { rc = FABGPU_EINVAL; return; }
                bound(o[i], o[i + 1]);
            }
        }
    }
    // gathered pieces, always pairs, from the caller's arena only
    void see_gather(const uint32_t* g, size_t pieces) {
        for (size_t j = 0; j < pieces; j++) {
            const uint32_t s0 = g[2 * j], s1 = g[2 * j + 1];
            if (s1 < s0 || (s1 > s0 && s1 > tail_base)) { rc = FABGPU_EINVAL; return; }
            if (s1 == s0) continue;
            bound(s0, s1);
            gather_total += s1 - s0;
        }
    }
    int close() {
        if (rc == FABGPU_OK && gather_total > 0x7FFFFFF0ull) rc = FABGPU_ETOOBIG;
        if (lo == 0xFFFFFFFFu) lo = hi = 0;                // nothing references the caller's arena
        if (tail_used && place == IN_ARENA) lo = 0;
        return rc;
    }
    void absolute() { lo = 0; }                            // a staged arena: offsets are offsets into the staged bytes
    size_t span() const { return (size_t)hi - lo; }        // bytes taken from the caller's arena
    // k offsets as the device sees them: arena spans move down by lo, spans of the tail stay, empty spans become (0, 0)
    void rebase(uint32_t* dst, const uint32_t* src, size_t k, bool pairs) const {
        if (!pairs) {
            for (size_t i = 0; i < k; i++) dst[i] = src[i] - lo;
            return;
        }
        for (size_t i = 0; i < k; i += 2) {
            const uint32_t s0 = src[i], s1 = src[i + 1], by = s0 >= tail_base ? 0 : lo;
            dst[i] = s1 > s0 ? s0 - by : 0;
            dst[i + 1] = s1 > s0 ? s1 - by : 0;
        }
    }

private:
    void bound(uint32_t s0, uint32_t s1) {
        if (s0 < lo) lo = s0;
        if (s1 > hi) hi = s1;
    }
};

}  // namespace fab
