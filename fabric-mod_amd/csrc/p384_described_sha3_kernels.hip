// HIP kernel for gfx950 (MI355X / CDNA4): the SHA3-256 digests of a DESCRIBED batch for the P-384 verify kernels - the twin of
// p384_described_kernels.hip for an MSP of the SHA3 hash family (msp/identities.go:216-224: the digest comes from the MSP's family, not
// from the curve; a 32-byte digest enters P-384 as a 256-bit e whatever hash made it, the E32 form of the two verify kernels).
//
// The description is that unit's:
//   message i = prefix[pre_idx[i]] || src[span_i)            (pre_idx[i] = 0xFFFFFFFF or no prefixes at all: the span alone)
//   src       = the arena for a span below tail_base, the tail (offsets relative to tail_base) for one at or above it
// The whole 136-byte blocks of every prefix are absorbed once by sha3_256_midstate_kernel (sha3_kernels.hip, launch_sha3_256_midstates -
// the launch the P-256 described path uses under FABGPU_IDB_SHA3_256; 200 bytes a prefix); a lane continues from that state - from the
// zero state for a prefix shorter than a block - with the prefix's last (len mod 136) bytes, its own span and the padding
// (sha3_256.h sha3_256_stream2: the block assembly, the pad and Keccak-f[1600] are the ones every other SHA3-256 kernel here runs).
// One message per lane, one wavefront per workgroup, no prefetch: the state, a block's 35 raw dwords and the prefix's 35 are live at once.
//
// BOUNDS, as in the SHA-256 unit.  Offsets are u32; a lane's loads are dword indices relative to the base of ITS source (the arena for
// the prefix's bytes; the arena or the tail for its own), at most 2^30, and every index is clamped to [0, words of that source): no read
// reaches arena_bytes (a multiple of 4, the launcher's condition) or the end of the tail's last dword whatever the offsets say.  A
// reversed span or prefix hashes as empty.  Rows at or above n are never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "sha3_256.h"

namespace fab {

// dwords of one source, every index clamped to [0, last]
struct Sha3Source {
    const uint32_t* __restrict__ p;
    int32_t last;
    __device__ __forceinline__ uint32_t word(int32_t i) const {
        i = i < last ? i : last;
        i = i > 0 ? i : 0;
        return p[i];
    }
};

struct described384_sha3 {
    const uint32_t* off;       // n (start, end) pairs, or n + 1 consecutive offsets
    const uint32_t* pre_idx;   // n, or nullptr: the batch has no prefixes
    const uint32_t* pre_off;   // m pairs, or m + 1 offsets
    const uint32_t* mid;       // m x 50 words (sha3_256_midstate_kernel)
    uint32_t m;
    uint32_t spans;
    const uint32_t* tail32;    // nullptr: no tail
    uint32_t tail_base;        // 0xFFFFFFFF without a tail
    uint32_t tail_words;
};

__global__ void __launch_bounds__(64) p384_described_sha3_digest_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                                        described384_sha3 d, uint32_t* __restrict__ digests) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : (n - 1);
    uint32_t start = d.off[d.spans ? 2 * (size_t)ic : (size_t)ic];
    const uint32_t end = d.off[d.spans ? 2 * (size_t)ic + 1 : (size_t)ic + 1];
    const uint32_t len = end >= start ? end - start : 0;                  // (a reversed span is the entry point's to refuse: hashed as empty)
    // the lane's source: spans at or above tail_base address the tail
    const bool in_tail = d.tail32 != nullptr && start >= d.tail_base;
    const Sha3Source arena{arena32, arena_words ? (int32_t)arena_words - 1 : 0};
    const Sha3Source src{in_tail ? d.tail32 : arena32, in_tail ? (d.tail_words ? (int32_t)d.tail_words - 1 : 0) : arena.last};
    start = in_tail ? start - d.tail_base : start;
    uint32_t a[SHA3_STATE_WORDS];
    sha3_zero(a);
    uint32_t sa = 0, la = 0;
    const bool prefixed = d.pre_idx != nullptr;                           // wave-uniform
    if (prefixed) {
        const uint32_t pi = d.pre_idx[ic];
        const bool has = pi < d.m;
        const uint32_t ps = has ? d.pre_off[d.spans ? 2 * (size_t)pi : (size_t)pi] : 0;
        const uint32_t pe = has ? d.pre_off[d.spans ? 2 * (size_t)pi + 1 : (size_t)pi + 1] : 0;
        const uint32_t pl = pe >= ps ? pe - ps : 0;
        const uint32_t base = pl / SHA3_256_RATE * SHA3_256_RATE;
        sa = ps + base;                                                   // the prefix's remaining bytes come from the arena (a prefix never lies in the tail)
        la = pl - base;
        if (has && base) {
            const uint2* mp = reinterpret_cast<const uint2*>(d.mid + (size_t)SHA3_STATE_WORDS * pi);
#pragma unroll
            for (int k = 0; k < SHA3_STATE_WORDS / 2; k++) {
                const uint2 v = mp[k];
                a[2 * k] = v.x;
                a[2 * k + 1] = v.y;
            }
        }
    }
    // every lane loops to its own block count (a lane without a message: none); the wavefront leaves the loop with its longest lane
    sha3_256_stream2<Sha3Source, Sha3Source, false>(arena, src, a, sa, la, start, len, active, prefixed, active ? sha3_256_blocks(la + len) : 0);
    if (active) {
        uint4* o = reinterpret_cast<uint4*>(digests + 8 * (size_t)i);
        o[0] = make_uint4(a[0], a[1], a[2], a[3]);
        o[1] = make_uint4(a[4], a[5], a[6], a[7]);
    }
}

hipError_t launch_p384_described_sha3_digests(const P384DescribedLaunch& v, hipStream_t st) {
    if (v.n == 0) return hipSuccess;
    if (!v.arena || !v.off || !v.digests || v.arena_bytes < 4 || (v.arena_bytes & 3u) || v.arena_bytes > 0xFFFFFFFFull || ((uintptr_t)v.arena & 3u) ||
        ((uintptr_t)v.tail & 3u))
        return hipErrorInvalidValue;
    const bool prefixed = v.pa.m != 0 && v.pa.pre_idx != nullptr;
    if (prefixed && (!v.pa.pre_off || !v.pa.mid_scratch || ((uintptr_t)v.pa.mid_scratch & 7u))) return hipErrorInvalidValue;
    if (prefixed && !v.pa.mid_ready) {
        const hipError_t e = launch_sha3_256_midstates(v.arena, v.arena_bytes, v.pa, st);
        if (e != hipSuccess) return e;
    }
    described384_sha3 d;
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
    hipLaunchKernelGGL(p384_described_sha3_digest_kernel, dim3((v.n + 63) / 64), dim3(64), 0, st, v.n, (const uint32_t*)v.arena, (uint32_t)(v.arena_bytes / 4), d,
                       (uint32_t*)v.digests);
    return hipGetLastError();
}

}  // namespace fab
