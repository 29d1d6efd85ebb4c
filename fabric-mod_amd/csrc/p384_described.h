// What p384_described_kernels.hip (SHA-256) and p384_described_sha3_kernels.hip (SHA3-256) share: the description a digest kernel is
// handed, the launcher's checks and fill, and a lane's decoding of its span and its prefix.  The hashing is each unit's own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace fab {

struct Described384 {
    const uint32_t* off;       // n (start, end) pairs, or n + 1 consecutive offsets
    const uint32_t* pre_idx;   // n, or nullptr: the batch has no prefixes
    const uint32_t* pre_off;   // m pairs, or m + 1 offsets
    const uint32_t* mid;       // m mid-states as the family's mid-state kernel wrote them: 8 words each (SHA-256), 50 (SHA3-256)
    uint32_t m;
    uint32_t spans;
    const uint32_t* tail32;    // nullptr: no tail
    uint32_t tail_base;        // 0xFFFFFFFF without a tail
    uint32_t tail_words;
};

// The conditions of kernels.h on a P384DescribedLaunch (mid_align: what the family's mid-states must be aligned to), then the description.
// *prefixed: the batch has prefixes, and the caller makes their mid-states unless v.pa.mid_ready.
inline hipError_t describe384(const P384DescribedLaunch& v, uintptr_t mid_align, Described384* d, bool* prefixed) {
    if (!v.arena || !v.off || !v.digests || v.arena_bytes < 4 || (v.arena_bytes & 3u) || v.arena_bytes > 0xFFFFFFFFull || ((uintptr_t)v.arena & 3u) || ((uintptr_t)v.tail & 3u))
        return hipErrorInvalidValue;
    *prefixed = v.pa.m != 0 && v.pa.pre_idx != nullptr;
    if (*prefixed && (!v.pa.pre_off || !v.pa.mid_scratch || ((uintptr_t)v.pa.mid_scratch & (mid_align - 1)))) return hipErrorInvalidValue;
    d->off = (const uint32_t*)v.off;
    d->pre_idx = *prefixed ? (const uint32_t*)v.pa.pre_idx : nullptr;
    d->pre_off = (const uint32_t*)v.pa.pre_off;
    d->mid = (const uint32_t*)v.pa.mid_scratch;
    d->m = *prefixed ? v.pa.m : 0;
    d->spans = v.pa.spans ? 1u : 0u;
    const bool has_tail = v.tail != nullptr && v.tail_len != 0;
    d->tail32 = has_tail ? (const uint32_t*)v.tail : nullptr;
    d->tail_base = has_tail ? v.tail_base : 0xFFFFFFFFu;
    d->tail_words = has_tail ? (v.tail_len + 3u) / 4u : 0;
    return hipSuccess;
}

// lane `ic`'s own span: where it starts in its source, its length (a reversed span is the entry point's to refuse: hashed as empty), and
// the source - spans at or above tail_base address the tail
struct Described384Span {
    uint32_t start, len;
    bool in_tail;
    const uint32_t* __restrict__ src;
    uint32_t src_words;
};
__device__ __forceinline__ Described384Span described384_span(const Described384& d, uint32_t ic, const uint32_t* __restrict__ arena32, uint32_t arena_words) {
    const uint32_t start = d.off[d.spans ? 2 * (size_t)ic : (size_t)ic];
    const uint32_t end = d.off[d.spans ? 2 * (size_t)ic + 1 : (size_t)ic + 1];
    Described384Span s;
    s.len = end >= start ? end - start : 0;
    s.in_tail = d.tail32 != nullptr && start >= d.tail_base;
    s.src = s.in_tail ? d.tail32 : arena32;
    s.src_words = s.in_tail ? d.tail_words : arena_words;
    s.start = s.in_tail ? start - d.tail_base : start;
    return s;
}
// lane `ic`'s prefix: its index (has: below m), where it starts in the arena and its length (0, 0 without one)
__device__ __forceinline__ uint32_t described384_prefix(const Described384& d, uint32_t ic, bool* has, uint32_t* ps, uint32_t* pl) {
    const uint32_t pi = d.pre_idx[ic];
    *has = pi < d.m;
    *ps = *has ? d.pre_off[d.spans ? 2 * (size_t)pi : (size_t)pi] : 0;
    const uint32_t pe = *has ? d.pre_off[d.spans ? 2 * (size_t)pi + 1 : (size_t)pi + 1] : 0;
    *pl = pe >= *ps ? pe - *ps : 0;
    return pi;
}

}  // namespace fab
