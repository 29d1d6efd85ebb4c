// HIP kernels for gfx950 (MI355X / CDNA4): SHA3-256 with thirty-two lanes on a message (sha3_coop.h) - two messages a wavefront, one
// 64-bit word of Keccak's state per lane, the exchanges of theta, pi and chi as ds_bpermute_b32 (the LDS crossbar; no LDS is allocated).
// Two roads, both behind FABGPU_FLAG_SHA3_COOP (fabgpu_api.hip):
//   sha3_256_coop_kernel   launches of at most SHA3_COOP_MAX messages, which cannot fill the chip with one lane per message; a prefixed
//                          message is hashed whole, prefix first: no mid-states;
//   sha3_256_mixed_kernel  larger plain launches: one lane per message (sha3_256_stream, unchanged), except that the first two messages
//                          of more than `long_over` bytes in every 64 are hashed on 32 lanes each by wavefronts of their own, in the same launch.
// The unit's build refuses any scratch; nothing is kept in LDS.
//
// Replaces (reference, CPU): bccsp/sw/hash.go under SHA3_256Opts, as sha3_kernels.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "sha3_coop.h"

namespace fab {

// dwords of the arena allocation, every index clamped to [0, last] (the rule of sha3_kernels.hip's Sha3DevArena): no read outside the
// arena whatever the offsets say
struct Sha3CoopArena {
    const uint32_t* __restrict__ p;
    int32_t last;
    __device__ __forceinline__ uint32_t word(int32_t i) const {
        i = i < last ? i : last;
        i = i > 0 ? i : 0;
        return p[i];
    }
};

// the exchange policy of sha3_coop.h on a wavefront: a group is lanes 0 .. 31 or 32 .. 63
struct Sha3WaveX {
    using U = uint32_t;
    static __device__ __forceinline__ U lane() { return threadIdx.x & 31u; }
    static __device__ __forceinline__ U index(U src) { return ((threadIdx.x & 32u) | (src & 31u)) << 2; }   // ds_bpermute_b32 takes the lane's byte address
    static __device__ __forceinline__ U read(U v, U index) { return (U)__builtin_amdgcn_ds_bpermute((int)index, (int)v); }
    template <class F, class... A>
    static __device__ __forceinline__ U map(F f, A... a) {
        return f(a...);
    }
};

// one message on the 32 lanes of the caller's half-wavefront -> its digest row; both halves of the wavefront must come here together
__device__ __forceinline__ void sha3_coop_row(const Sha3CoopArena& ar, uint32_t sa, uint32_t la, uint32_t sb, uint32_t lb, bool active, uint32_t i,
                                              uint32_t* __restrict__ digests) {
    const uint32_t nblk = active ? sha3_256_blocks(la + lb) : 0;
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)nblk, 0), b1 = (uint32_t)__builtin_amdgcn_readlane((int)nblk, 32);
    uint32_t lo, hi;
    sha3_256_coop<Sha3WaveX>(ar, sa, la, sb, lb, active, b0 > b1 ? b0 : b1, lo, hi);
    const uint32_t l = threadIdx.x & 31u;
    if (active && l < 4) reinterpret_cast<uint2*>(digests + 8 * (size_t)i)[l] = make_uint2(lo, hi);   // the bytes the one-lane kernel stores
}

// message i = arena[off[i], off[i+1]) (spans: off holds (start, end) pairs; a reversed span is empty); PREFIXED: behind the whole prefix
// pre_idx[i] (0xFFFFFFFF, or any index >= m: none).  digests: n x 32 bytes; rows at or above n are never written.
template <bool PREFIXED>
__global__ void __launch_bounds__(256) sha3_256_coop_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                             const uint32_t* __restrict__ off, uint32_t spans, const uint32_t* __restrict__ pre_idx,
                                                             const uint32_t* __restrict__ pre_off, uint32_t m, uint32_t* __restrict__ digests) {
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    if ((i & ~1u) >= n) return;                                            // (wavefront-uniform: neither half has a message)
    const bool active = i < n;
    const uint32_t ic = active ? i : (n - 1);
    const uint32_t start = off[spans ? 2 * ic : ic], end = off[spans ? 2 * ic + 1 : ic + 1];
    uint32_t ps = 0, pl = 0;
    if (PREFIXED) {
        const uint32_t pi = pre_idx[ic];
        if (pi < m) {
            ps = pre_off[spans ? 2 * pi : pi];
            const uint32_t pe = pre_off[spans ? 2 * pi + 1 : pi + 1];
            pl = pe >= ps ? pe - ps : 0;
        }
    }
    Sha3CoopArena ar{arena32, arena_words ? (int32_t)arena_words - 1 : 0};
    sha3_coop_row(ar, ps, pl, start, end >= start ? end - start : 0, active, i, digests);
}

__device__ __forceinline__ uint32_t sha3_mixed_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        uint32_t other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}

// A launch too large for 32 lanes per message: one lane per message, but not for its LONG messages - a launch lasts as long as its
// longest message.  The first scan_wgs workgroups look at 64 messages per wavefront, a lane each, and hash the first TWO of more than
// long_over bytes among them on 32 lanes each (none, nearly always: they leave after one ballot); the workgroups behind them are the
// one-lane ones of sha3_kernels.hip, cut into the same groups of 64, and skip exactly those two.  One launch: the long ones start first.
// coop_rows (optional): += the rows hashed on 32 lanes.
__global__ void __launch_bounds__(256) sha3_256_mixed_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                              const uint32_t* __restrict__ off, uint32_t pairs, uint32_t long_over, uint32_t scan_wgs,
                                                              uint32_t* __restrict__ digests, unsigned long long* __restrict__ coop_rows) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    auto span = [&](uint32_t i, uint32_t& start, uint32_t& len) {
        start = off[pairs ? 2 * i : i];
        const uint32_t end = off[pairs ? 2 * i + 1 : i + 1];
        len = end >= start ? end - start : 0;
    };
    Sha3CoopArena ar{arena32, arena_words ? (int32_t)arena_words - 1 : 0};
    if (blockIdx.x < scan_wgs) {
        const uint32_t i0 = (blockIdx.x * waves + wave) * 64u, mine = i0 + lane;
        uint32_t st0 = 0, ln0 = 0;
        if (mine < n) span(mine, st0, ln0);
        uint64_t longs = __ballot(mine < n && ln0 > long_over);
        if (longs == 0ull) return;
        uint32_t pick = 64, picked = 0;
        for (uint32_t g = 0; g < (uint32_t)SHA3C_PER_WAVE && longs; g++) {   // (wavefront-uniform) the first two, one per half
            const uint32_t b = (uint32_t)__builtin_ctzll(longs);
            longs &= longs - 1;
            if ((lane >> 5) == g) pick = b;
            picked++;
        }
        const bool active = pick < 64;
        const uint32_t i = i0 + (active ? pick : 0u);
        uint32_t start = 0, len = 0;
        if (active) span(i, start, len);
        sha3_coop_row(ar, 0, 0, start, len, active, i, digests);
        if (lane == 0 && coop_rows != nullptr) atomicAdd(coop_rows, (unsigned long long)picked);
        return;
    }
    const uint32_t i = (blockIdx.x - scan_wgs) * blockDim.x + threadIdx.x;
    uint32_t start = 0, len = 0;
    if (i < n) span(i, start, len);
    // (this wavefront's 64 messages are the 64 a scan wavefront looked at: the first two long ones are that one's)
    const uint64_t longs = __ballot(i < n && len > long_over);
    const bool taken = i < n && len > long_over && __builtin_popcountll(longs & ((1ull << lane) - 1ull)) < SHA3C_PER_WAVE;
    const bool active = i < n && !taken;
    uint32_t a[SHA3_STATE_WORDS];
    sha3_zero(a);
    const uint32_t maxblk = sha3_mixed_wave_max(active ? sha3_256_blocks(len) : 0);
    sha3_256_stream<Sha3CoopArena, true>(ar, a, 0, 0, start, len, active, false, maxblk);
    if (active) {
        uint4* o = reinterpret_cast<uint4*>(digests + 8 * (size_t)i);
        o[0] = make_uint4(a[0], a[1], a[2], a[3]);
        o[1] = make_uint4(a[4], a[5], a[6], a[7]);
    }
}

// ------------------------------------------------------------------------------------------------
// launchers (host)
// ------------------------------------------------------------------------------------------------
constexpr uint32_t SHA3C_WG_WAVES = 4;     // a workgroup's wavefronts go to the four SIMDs of its CU (wide_kernels.hip PLACEMENT)

hipError_t launch_sha3_256_messages_coop(uint32_t n, const void* arena, size_t arena_bytes, const void* off, const ShaPrefixArgs& pa, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (pa.digests == nullptr) return hipErrorInvalidValue;
    const bool prefixed = pa.m != 0 && pa.pre_idx != nullptr;
    if (prefixed && pa.pre_off == nullptr) return hipErrorInvalidValue;    // (pa.mid_scratch is not read: it may be null)
    const uint32_t per_wg = SHA3C_WG_WAVES * (uint32_t)SHA3C_PER_WAVE;
    dim3 grid((n + per_wg - 1) / per_wg), block(64 * SHA3C_WG_WAVES);
    const uint32_t arena_words = (uint32_t)((arena_bytes + 3) / 4);
    if (prefixed)
        hipLaunchKernelGGL(sha3_256_coop_kernel<true>, grid, block, 0, st, n, (const uint32_t*)arena, arena_words, (const uint32_t*)off, pa.spans ? 1u : 0u,
                           (const uint32_t*)pa.pre_idx, (const uint32_t*)pa.pre_off, pa.m, (uint32_t*)pa.digests);
    else
        hipLaunchKernelGGL(sha3_256_coop_kernel<false>, grid, block, 0, st, n, (const uint32_t*)arena, arena_words, (const uint32_t*)off, pa.spans ? 1u : 0u,
                           (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0u, (uint32_t*)pa.digests);
    return hipGetLastError();
}

hipError_t launch_sha3_256_mixed(uint32_t n, const void* arena, size_t arena_bytes, const void* off, bool pairs, void* digests, void* coop_rows,
                                 hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (digests == nullptr) return hipErrorInvalidValue;
    const uint32_t wgs = (n + 255) / 256;
    // "long" as launch_sha256_mixed has it: a quarter above what the messages average if they fill their arena, and at least 2 KiB
    const uint64_t mean = arena_bytes / n;
    const uint32_t long_over = (uint32_t)std::min<uint64_t>(0xFFFFFFF0ull, std::max<uint64_t>(2048, mean + mean / 4));
    hipLaunchKernelGGL(sha3_256_mixed_kernel, dim3(2 * wgs), dim3(256), 0, st, n, (const uint32_t*)arena, (uint32_t)((arena_bytes + 3) / 4),
                       (const uint32_t*)off, pairs ? 1u : 0u, long_over, wgs, (uint32_t*)digests, (unsigned long long*)coop_rows);
    return hipGetLastError();
}

// see warm_kernel_functions_kernels (kernels.hip)
int warm_kernel_functions_sha3_coop() {
    int ok = 0;
    hipFuncAttributes a;
    const void* fns[] = {(const void*)sha3_256_coop_kernel<false>, (const void*)sha3_256_coop_kernel<true>, (const void*)sha3_256_mixed_kernel};
    for (const void* f : fns) ok += hipFuncGetAttributes(&a, f) == hipSuccess ? 1 : 0;
    return ok;
}

}  // namespace fab
