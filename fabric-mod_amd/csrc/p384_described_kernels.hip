// HIP kernel for gfx950 (MI355X / CDNA4): the SHA-256 digests of a DESCRIBED batch for the P-384 verify kernels.
//
// A P-384 identity of a SHA-2 MSP signs over the SHA-256 of its message (msp/identities.go:169-196: the digest comes from the MSP's hash
// family, not from the curve), and the E32 form of p384_verify_kernel / p384_verify_keyed_kernel reads n rows of 32 digest bytes.  The
// messages of a block are not consecutive: an endorsement signs  prp || endorser  (core/common/validation/statebased/
// validator_keylevel.go:246-258) - two spans of the block, the first shared by the transaction's endorsements - and the orderers sign
// bytes the host builds (the tail).  This unit turns such a description into the digest rows in ONE launch, reading the block where it
// already lies on the device:
//   message i = prefix[pre_idx[i]] || src[span_i)            (pre_idx[i] = 0xFFFFFFFF or no prefixes at all: the span alone)
//   src       = the arena for a span below tail_base, the tail (offsets relative to tail_base) for one at or above it
// The whole 64-byte blocks of every prefix are hashed once by sha256_midstate_kernel (kernels.hip, launch_sha256_midstates - the launch the
// P-256 described path uses); a lane continues from that mid-state with the prefix's last (len mod 64) bytes, its own span and the padding
// (device_common.h sha256_stream_t: the tail rule, the schedule and the compression are the ones every other SHA-256 kernel here runs).
// One message per lane, the next block's 17 dwords requested before the current one is compressed.
//
// BOUNDS.  Offsets are u32; a lane's loads are dword indices relative to the base of ITS source (the arena or the tail), formed in 64 bits
// by the address computation (an index is 2^30 at the most: the rule of the hash kernels for offsets at and above 2^31), and every index
// is clamped to [0, words of that source): no read reaches arena_bytes (a multiple of 4, the launcher's condition) or the end of the tail's
// last dword whatever the offsets say.  A span that straddles tail_base is the entry point's to refuse (fabgpu_api.hip); here it reads
// clamped arena bytes and nothing else.  Rows at or above n are never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "kernels.h"
#include "sha256_coop.h"

namespace fab {

struct described384 {
    const uint32_t* off;       // n (start, end) pairs, or n + 1 consecutive offsets
    const uint32_t* pre_idx;   // n, or nullptr: the batch has no prefixes
    const uint32_t* pre_off;   // m pairs, or m + 1 offsets
    const uint32_t* mid;       // m x 8 words (sha256_midstate_kernel)
    uint32_t m;
    uint32_t spans;
    const uint32_t* tail32;    // nullptr: no tail
    uint32_t tail_base;        // 0xFFFFFFFF without a tail
    uint32_t tail_words;
};

__global__ void __launch_bounds__(64) p384_described_digest_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words, described384 d,
                                                                   uint32_t* __restrict__ digests) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : (n - 1);
    uint32_t start = d.off[d.spans ? 2 * (size_t)ic : (size_t)ic];
    const uint32_t end = d.off[d.spans ? 2 * (size_t)ic + 1 : (size_t)ic + 1];
    const uint32_t len = end >= start ? end - start : 0;                  // (a reversed span is the entry point's to refuse: hashed as empty)
    // the lane's source: spans at or above tail_base address the tail
    const bool in_tail = d.tail32 != nullptr && start >= d.tail_base;
    const uint32_t* __restrict__ src = in_tail ? d.tail32 : arena32;
    const uint32_t src_words = in_tail ? d.tail_words : arena_words;
    start = in_tail ? start - d.tail_base : start;
    uint32_t h[8];
    sha256_iv(h);
    if (d.pre_idx == nullptr) {                                           // wave-uniform
        sha256_stream_t<ShaTailArena, true>(src, src_words, h, ShaTailArena{arena32, 0, 0}, 0, start, len, 0, active, false);
    } else {
        const uint32_t pi = d.pre_idx[ic];
        const bool has = pi < d.m;
        const uint32_t ps = has ? d.pre_off[d.spans ? 2 * (size_t)pi : (size_t)pi] : 0;
        const uint32_t pe = has ? d.pre_off[d.spans ? 2 * (size_t)pi + 1 : (size_t)pi + 1] : 0;
        const uint32_t pl = pe >= ps ? pe - ps : 0;
        const uint32_t base = pl & ~63u, rest = pl & 63u;
        if (has && base) {
            const uint4* mp = reinterpret_cast<const uint4*>(d.mid + 8 * (size_t)pi);
            const uint4 m0 = mp[0], m1 = mp[1];
            h[0] = m0.x; h[1] = m0.y; h[2] = m0.z; h[3] = m0.w;
            h[4] = m1.x; h[5] = m1.y; h[6] = m1.z; h[7] = m1.w;
        }
        // the prefix's remaining bytes come from the arena (a prefix never lies in the tail), the lane's own from its source
        const ShaTailArena rest_of_prefix{arena32, arena_words ? (int32_t)arena_words - 1 : 0, ps + base};
        sha256_stream_t<ShaTailArena, true>(src, src_words, h, rest_of_prefix, rest, start, len, base, active, true);
    }
    if (active) sha256_coop_store(digests, i, h);
}

hipError_t launch_p384_described_digests(const P384DescribedLaunch& v, hipStream_t st) {
    if (v.n == 0) return hipSuccess;
    if (!v.arena || !v.off || !v.digests || v.arena_bytes < 4 || (v.arena_bytes & 3u) || v.arena_bytes > 0xFFFFFFFFull || ((uintptr_t)v.arena & 3u) || ((uintptr_t)v.tail & 3u))
        return hipErrorInvalidValue;
    const bool prefixed = v.pa.m != 0 && v.pa.pre_idx != nullptr;
    if (prefixed && (!v.pa.pre_off || !v.pa.mid_scratch)) return hipErrorInvalidValue;
    if (prefixed && !v.pa.mid_ready) {
        const hipError_t e = launch_sha256_midstates(v.arena, v.arena_bytes, v.pa, st);
        if (e != hipSuccess) return e;
    }
    described384 d;
    d.off = (const uint32_t*)v.off;
    d.pre_idx = prefixed ? (const uint32_t*)v.pa.pre_idx : nullptr;
    d.pre_off = (const uint32_t*)v.pa.pre_off;
    d.mid = (const uint32_t*)v.pa.mid_scratch;
    d.m = prefixed ? v.pa.m : 0;
    d.spans = v.pa.spans ? 1u : 0u;
    const bool has_tail = v.tail != nullptr && v.tail_len != 0;
    d.tail32 = has_tail ? (const uint32_t*)v.tail : nullptr;
    d.tail_base = has_tail ? v.tail_base : 0xFFFFFFFFu;
    d.tail_words = has_tail ? (v.tail_len + 3u) / 4u : 0;
    hipLaunchKernelGGL(p384_described_digest_kernel, dim3((v.n + 63) / 64), dim3(64), 0, st, v.n, (const uint32_t*)v.arena, (uint32_t)(v.arena_bytes / 4), d,
                       (uint32_t*)v.digests);
    return hipGetLastError();
}

}  // namespace fab
