// HIP kernels for gfx950 (MI355X / CDNA4): batched SHA3-256 over a ragged arena, one message per lane (sha3_256.h), with shared-prefix
// mid-states.  Integer VALU work only: v_alignbit_b32 for the rotations, v_bitop3_b32 for theta's parities and for chi.  The state
// (50 words), a block's 35 raw dwords and the next block's 35 stay in registers: the unit's build refuses any scratch.
//
// Replaces (reference, CPU): bccsp/sw/hash.go under SHA3_256Opts - the hash identity.Verify takes for an MSP of the SHA3 family
// (msp/identities.go:216-224).  The digests feed the unchanged P-256 verify kernels as `e` (fabgpu_api.hip): two launches on one
// stream, no fused Keccak + verify kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "sha3_256.h"

namespace fab {

// dwords of the arena allocation, every index clamped to [0, last]: no read outside the arena whatever the offsets say
struct Sha3DevArena {
    const uint32_t* __restrict__ p;
    int32_t last;
    __device__ __forceinline__ uint32_t word(int32_t i) const {
        i = i < last ? i : last;
        i = i > 0 ? i : 0;
        return p[i];
    }
};

__device__ __forceinline__ uint32_t sha3_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        uint32_t other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}

// prefix p = arena[pre_off[p], pre_off[p+1]) (spans: pairs); its whole 136-byte blocks -> mid[50 p .. 50 p + 50)
__global__ void __launch_bounds__(256) sha3_256_midstate_kernel(uint32_t m, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                                 const uint32_t* __restrict__ pre_off, uint32_t spans, uint32_t* __restrict__ mid) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = p < m;
    const uint32_t pc = active ? p : (m - 1);
    const uint32_t start = pre_off[spans ? 2 * pc : pc], len = pre_off[spans ? 2 * pc + 1 : pc + 1] - start;
    const uint32_t nfull = active ? len / SHA3_256_RATE : 0;
    const uint32_t maxfull = sha3_wave_max(nfull);
    Sha3DevArena ar{arena32, arena_words ? (int32_t)arena_words - 1 : 0};
    uint32_t a[SHA3_STATE_WORDS];
    sha3_zero(a);
    sha3_256_midstate<Sha3DevArena, true>(ar, a, start, nfull, maxfull);
    if (active) {
        uint2* o = reinterpret_cast<uint2*>(mid + (size_t)SHA3_STATE_WORDS * p);
#pragma unroll
        for (int k = 0; k < SHA3_STATE_WORDS / 2; k++) o[k] = make_uint2(a[2 * k], a[2 * k + 1]);
    }
}

// message i = arena[off[i], off[i+1]) (spans: off holds (start, end) pairs); PREFIXED: behind prefix pre_idx[i] (0xFFFFFFFF = none),
// continuing from mid[pre_idx[i]].  digests: n x 32 bytes.
template <bool PREFIXED>
__global__ void __launch_bounds__(256) sha3_256_batch_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                              const uint32_t* __restrict__ off, uint32_t spans, const uint32_t* __restrict__ pre_idx,
                                                              const uint32_t* __restrict__ pre_off, const uint32_t* __restrict__ mid, uint32_t m,
                                                              uint32_t* __restrict__ digests) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : (n - 1);
    const uint32_t start = off[spans ? 2 * ic : ic], len = off[spans ? 2 * ic + 1 : ic + 1] - start;
    Sha3DevArena ar{arena32, arena_words ? (int32_t)arena_words - 1 : 0};
    uint32_t a[SHA3_STATE_WORDS];
    sha3_zero(a);
    uint32_t sa = 0, la = 0;
    if (PREFIXED) {
        const uint32_t pi = pre_idx[ic];
        const bool has = pi < m;
        const uint32_t ps = has ? pre_off[spans ? 2 * pi : pi] : 0, pl = has ? pre_off[spans ? 2 * pi + 1 : pi + 1] - ps : 0;
        const uint32_t base = pl / SHA3_256_RATE * SHA3_256_RATE;
        sa = ps + base;
        la = pl - base;
        if (has && base) {
            const uint2* mp = reinterpret_cast<const uint2*>(mid + (size_t)SHA3_STATE_WORDS * pi);
#pragma unroll
            for (int k = 0; k < SHA3_STATE_WORDS / 2; k++) {
                uint2 v = mp[k];
                a[2 * k] = v.x;
                a[2 * k + 1] = v.y;
            }
        }
    }
    const uint32_t maxblk = sha3_wave_max(active ? sha3_256_blocks(la + len) : 0);
    sha3_256_stream<Sha3DevArena, !PREFIXED>(ar, a, sa, la, start, len, active, PREFIXED, maxblk);   // (the prefixed form holds the tail's 35 dwords too: no prefetch there)
    if (active) {
        uint4* o = reinterpret_cast<uint4*>(digests + 8 * (size_t)i);
        o[0] = make_uint4(a[0], a[1], a[2], a[3]);
        o[1] = make_uint4(a[4], a[5], a[6], a[7]);
    }
}

// ------------------------------------------------------------------------------------------------
// launchers (host)
// ------------------------------------------------------------------------------------------------
hipError_t launch_sha3_256_midstates(const void* arena, size_t arena_bytes, const ShaPrefixArgs& pa, hipStream_t st) {
    if (pa.m == 0) return hipSuccess;
    dim3 grid((pa.m + 255) / 256), block(256);
    hipLaunchKernelGGL(sha3_256_midstate_kernel, grid, block, 0, st, pa.m, (const uint32_t*)arena, (uint32_t)((arena_bytes + 3) / 4),
                       (const uint32_t*)pa.pre_off, pa.spans ? 1u : 0u, (uint32_t*)pa.mid_scratch);
    return hipGetLastError();
}
hipError_t launch_sha3_256_messages(uint32_t n, const void* arena, size_t arena_bytes, const void* off, const ShaPrefixArgs& pa, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (pa.digests == nullptr) return hipErrorInvalidValue;
    const bool prefixed = pa.m != 0 && pa.pre_idx != nullptr;
    if (prefixed && (pa.pre_off == nullptr || pa.mid_scratch == nullptr)) return hipErrorInvalidValue;
    dim3 grid((n + 255) / 256), block(256);
    const uint32_t arena_words = (uint32_t)((arena_bytes + 3) / 4);
    if (prefixed)
        hipLaunchKernelGGL(sha3_256_batch_kernel<true>, grid, block, 0, st, n, (const uint32_t*)arena, arena_words, (const uint32_t*)off, pa.spans ? 1u : 0u,
                           (const uint32_t*)pa.pre_idx, (const uint32_t*)pa.pre_off, (const uint32_t*)pa.mid_scratch, pa.m, (uint32_t*)pa.digests);
    else
        hipLaunchKernelGGL(sha3_256_batch_kernel<false>, grid, block, 0, st, n, (const uint32_t*)arena, arena_words, (const uint32_t*)off, pa.spans ? 1u : 0u,
                           (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0u, (uint32_t*)pa.digests);
    return hipGetLastError();
}
hipError_t launch_sha3_256_batch(uint32_t n, const void* arena, size_t arena_bytes, const void* off, bool spans, void* digests, hipStream_t st) {
    ShaPrefixArgs pa;
    pa.spans = spans;
    pa.digests = digests;
    return launch_sha3_256_messages(n, arena, arena_bytes, off, pa, st);
}

// As warm_kernel_functions_kernels (kernels.hip), for a caller that wants the unit's functions resolved ahead of their first launch.  The
// provider's construction does not call it: it rehearses what a block pass launches, and the pass launches nothing of this unit.
int warm_kernel_functions_sha3() {
    int ok = 0;
    hipFuncAttributes a;
    const void* fns[] = {(const void*)sha3_256_midstate_kernel, (const void*)sha3_256_batch_kernel<false>, (const void*)sha3_256_batch_kernel<true>};
    for (const void* f : fns) ok += hipFuncGetAttributes(&a, f) == hipSuccess ? 1 : 0;
    return ok;
}

}  // namespace fab
