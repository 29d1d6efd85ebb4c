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
#include "p384_described.h"
#include "sha256_coop.h"

namespace fab {

__global__ void __launch_bounds__(64) p384_described_digest_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words, Described384 d,
                                                                   uint32_t* __restrict__ digests) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : (n - 1);
    const Described384Span sp = described384_span(d, ic, arena32, arena_words);
    uint32_t h[8];
    sha256_iv(h);
    if (d.pre_idx == nullptr) {                                           // wave-uniform
        sha256_stream_t<ShaTailArena, true>(sp.src, sp.src_words, h, ShaTailArena{arena32, 0, 0}, 0, sp.start, sp.len, 0, active, false);
    } else {
        bool has;
        uint32_t ps, pl;
        const uint32_t pi = described384_prefix(d, ic, &has, &ps, &pl);
        const uint32_t base = pl & ~63u, rest = pl & 63u;
        if (has && base) {
            const uint4* mp = reinterpret_cast<const uint4*>(d.mid + 8 * (size_t)pi);
            const uint4 m0 = mp[0], m1 = mp[1];
            h[0] = m0.x; h[1] = m0.y; h[2] = m0.z; h[3] = m0.w;
            h[4] = m1.x; h[5] = m1.y; h[6] = m1.z; h[7] = m1.w;
        }
        // the prefix's remaining bytes come from the arena (a prefix never lies in the tail), the lane's own from its source
        const ShaTailArena rest_of_prefix{arena32, arena_words ? (int32_t)arena_words - 1 : 0, ps + base};
        sha256_stream_t<ShaTailArena, true>(sp.src, sp.src_words, h, rest_of_prefix, rest, sp.start, sp.len, base, active, true);
    }
    if (active) sha256_coop_store(digests, i, h);
}

hipError_t launch_p384_described_digests(const P384DescribedLaunch& v, hipStream_t st) {
    if (v.n == 0) return hipSuccess;
    Described384 d;
    bool prefixed;
    hipError_t e = describe384(v, 1, &d, &prefixed);
    if (e == hipSuccess && prefixed && !v.pa.mid_ready) e = launch_sha256_midstates(v.arena, v.arena_bytes, v.pa, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(p384_described_digest_kernel, dim3((v.n + 63) / 64), dim3(64), 0, st, v.n, (const uint32_t*)v.arena, (uint32_t)(v.arena_bytes / 4), d,
                       (uint32_t*)v.digests);
    return hipGetLastError();
}

}  // namespace fab
