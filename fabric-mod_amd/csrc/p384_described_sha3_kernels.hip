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
#include "p384_described.h"
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

__global__ void __launch_bounds__(64) p384_described_sha3_digest_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                                        Described384 d, uint32_t* __restrict__ digests) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : (n - 1);
    const Described384Span sp = described384_span(d, ic, arena32, arena_words);
    const Sha3Source arena{arena32, arena_words ? (int32_t)arena_words - 1 : 0};
    const Sha3Source src{sp.src, sp.in_tail ? (sp.src_words ? (int32_t)sp.src_words - 1 : 0) : arena.last};
    uint32_t a[SHA3_STATE_WORDS];
    sha3_zero(a);
    uint32_t sa = 0, la = 0;
    const bool prefixed = d.pre_idx != nullptr;                           // wave-uniform
    if (prefixed) {
        bool has;
        uint32_t ps, pl;
        const uint32_t pi = described384_prefix(d, ic, &has, &ps, &pl);
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
    sha3_256_stream2<Sha3Source, Sha3Source, false>(arena, src, a, sa, la, sp.start, sp.len, active, prefixed, active ? sha3_256_blocks(la + sp.len) : 0);
    if (active) {
        uint4* o = reinterpret_cast<uint4*>(digests + 8 * (size_t)i);
        o[0] = make_uint4(a[0], a[1], a[2], a[3]);
        o[1] = make_uint4(a[4], a[5], a[6], a[7]);
    }
}

hipError_t launch_p384_described_sha3_digests(const P384DescribedLaunch& v, hipStream_t st) {
    if (v.n == 0) return hipSuccess;
    Described384 d;
    bool prefixed;
    hipError_t e = describe384(v, 8, &d, &prefixed);       // (a mid-state is read as 8-byte pairs)
    if (e == hipSuccess && prefixed && !v.pa.mid_ready) e = launch_sha3_256_midstates(v.arena, v.arena_bytes, v.pa, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(p384_described_sha3_digest_kernel, dim3((v.n + 63) / 64), dim3(64), 0, st, v.n, (const uint32_t*)v.arena, (uint32_t)(v.arena_bytes / 4), d,
                       (uint32_t*)v.digests);
    return hipGetLastError();
}

}  // namespace fab
