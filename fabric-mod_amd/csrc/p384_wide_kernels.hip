// HIP kernels for gfx950 (MI355X / CDNA4): batched ECDSA P-384 verification under REGISTERED keys with EIGHT LANES PER SIGNATURE, in
// two phases (p384_wide.h) - the form of keyed launches of at most P384_WIDE_LAUNCH_MAX rows, which cannot fill the chip: the one-lane
// kernel (p384_keyed_kernels.hip) takes as long for 4 000 rows as for 30 000.  Integer VALU work only; no MFMA, no LDS, no inline assembly.
//
// Replaces (reference, CPU): bccsp/sw/ecdsa.go:41-57 -> Go 1.14 crypto/ecdsa.Verify on the generic math/big curve, for a P-384 key the
// provider has met before (bccsp.KeyImport).
//
// PHASE A (p384_wide_a_kernel), one signature per lane: the gate, s^-1 mod n and the two scalars -> one 100-byte row of the launch's
//   scratch per signature (p384_wide.h wide_phase_a).  It reads no key.
// PHASE B (p384_wide_b_kernel), one wavefront per eight signatures: lane 8 g + j is lane j of the wavefront's g-th signature.  Each lane
//   sums its six windows of both tables, the eight sums meet in three levels over cross-lane shuffles (the 36 words of a Jacobian
//   triple, lanes j ^ 1, j ^ 2, j ^ 4), lane j = 0 decides.  Key ids, the slot snapshot and the rule for a stale, retired or out-of-range
//   id - status 4, the whole stream on the generator's comb - are those of p384_verify_keyed_kernel.
// VERDICT WORDS.  A wavefront of phase B holds eight rows: one BYTE of the verdict words (bit k of byte t = row 8 t + k), which its lane 0
//   stores as a byte - no word is read, modified and written back, no two wavefronts store to the same byte.  The wavefront of the last
//   rows also zeroes the bytes between its own and the end of the last word, ceil(n / 64) * 8: nobody's rows.  Nothing at or above that
//   is written; the bits of rows at or above n stay zero, as emit_verdict leaves them.  (wide_kernels.hip does the same for P-256.)
// Tail groups of the last wavefront compute on row n - 1 and write nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "p384_dev.h"
#include "p384_keys.h"
#include "p384_wide.h"

namespace fab {

namespace {

constexpr int P384W_BLOCK = 64;
constexpr uint32_t P384W_PER_WAVE = P384W_BLOCK / p384::P384W_LANES;      // signatures per wavefront of phase B
static_assert(P384W_PER_WAVE == 8, "one verdict byte per wavefront");
static_assert(P384_WIDE_SCRATCH_BYTES == (size_t)p384::P384W_ROW_BYTES, "kernels.h restates p384_wide.h for the host");

template <bool E32>
__global__ void __launch_bounds__(P384W_BLOCK) p384_wide_a_kernel(uint32_t n, const uint8_t* __restrict__ e, const uint8_t* __restrict__ r,
                                                                  const uint8_t* __restrict__ s, uint32_t* __restrict__ scratch) {
    const uint32_t i = blockIdx.x * P384W_BLOCK + threadIdx.x;
    const bool active = i < n;
    const uint32_t ic = active ? i : (n - 1);
    p384::u384 ve, vr, vs;
    load_e384<E32>(ve, e, ic);
    load_be_field48(vr, r, ic);
    load_be_field48(vs, s, ic);
    uint32_t row[p384::P384W_ROW_WORDS];
    p384::wide_phase_a(row, ve, vr, vs);
    if (active) {
        uint32_t* out = scratch + (size_t)p384::P384W_ROW_WORDS * i;
#pragma unroll
        for (int k = 0; k < p384::P384W_ROW_WORDS; k++) out[k] = row[k];
    }
}

// the triple of lane (this lane ^ m)
__device__ __forceinline__ void lane_xchg(p384::jac& o, const p384::jac& a, int m) {
#pragma unroll
    for (int k = 0; k < 12; k++) {
        o.X.w[k] = __shfl_xor(a.X.w[k], m);
        o.Y.w[k] = __shfl_xor(a.Y.w[k], m);
        o.Z.w[k] = __shfl_xor(a.Z.w[k], m);
    }
}

__global__ void __launch_bounds__(P384W_BLOCK) p384_wide_b_kernel(uint32_t n, const uint32_t* __restrict__ key_id, const uint8_t* __restrict__ r,
                                                                  const uint32_t* __restrict__ gcomb, const P384SlotSnap* __restrict__ snap,
                                                                  uint32_t nkeys, const uint32_t* __restrict__ scratch,
                                                                  uint8_t* __restrict__ verdict8, uint8_t* __restrict__ status) {
    const p384::CombPtr384 gt{gcomb};
    const uint32_t lane = threadIdx.x, sub = lane & (uint32_t)(p384::P384W_LANES - 1);
    const uint32_t ntiles = (n - 1) / P384W_PER_WAVE + 1;                 // (n >= 1)
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t i = tile * P384W_PER_WAVE + (lane >> 3);
        const bool active = i < n;
        const uint32_t ic = active ? i : (n - 1);
        const uint32_t id = key_id[ic], slot = id & ((1u << KEY_SLOT_BITS) - 1u), gen = id >> KEY_SLOT_BITS;
        const uint32_t* qtab = nullptr;
        uint32_t slot_gen = KTAB_GEN_NONE;
        if (slot < nkeys) {
            const P384SlotSnap sn = snap[slot];
            qtab = sn.tab;
            slot_gen = sn.gen;
        }
        const bool key_ok = slot_gen == gen && qtab != nullptr;
        const p384::CombPtr384 qt{key_ok ? qtab : gcomb};
        const uint32_t* row = scratch + (size_t)p384::P384W_ROW_WORDS * ic;
        p384::jac acc;
        p384::wide_lane_sum(acc, row, sub, gt, qt);
        for (uint32_t m = 1; m < (uint32_t)p384::P384W_LANES; m <<= 1) {
            p384::jac other, lo, hi;
            lane_xchg(other, acc, (int)m);
            const bool upper = (sub & m) != 0;
            p384::sel_pt(lo, upper, other, acc);
            p384::sel_pt(hi, upper, acc, other);
            p384::wide_join(acc, lo, hi);
        }
        p384::u384 vr;
        load_be_field48(vr, r, ic);
        const uint32_t st = p384::wide_decide(acc, vr, row[24], key_ok);
        // eight verdicts per wavefront, on lanes 0, 8, .. 56: squeeze them into one byte
        uint64_t x = __ballot(active && sub == 0 && st == 0u) & 0x0101010101010101ull;
        x = (x | (x >> 7)) & 0x0003000300030003ull;
        x = (x | (x >> 14)) & 0x0000000f0000000full;
        x = (x | (x >> 28)) & 0xffull;
        if (lane == 0) {
            verdict8[tile] = (uint8_t)x;
            if (tile == ntiles - 1)
                for (uint32_t b = ntiles; b < ((n - 1) / 64 + 1) * 8; b++) verdict8[b] = 0;
        }
        if (status != nullptr && active && sub == 0) status[i] = (uint8_t)st;
    }
}

}  // namespace

hipError_t launch_p384_verify_keyed_wide(const P384KeyedLaunch& v, hipStream_t st) {
    if (v.n == 0) return hipSuccess;
    if (!v.key_id || !v.e || !v.r || !v.s || !v.gcomb || !v.verdict_bits || (v.nkeys && !v.snap) || v.nkeys > (1u << KEY_SLOT_BITS)) return hipErrorInvalidValue;
    if (v.n > P384_WIDE_LAUNCH_MAX || !v.wide_scratch) return hipErrorInvalidValue;
    dim3 block(P384W_BLOCK), grid_a((v.n - 1) / P384W_BLOCK + 1), grid_b((v.n - 1) / P384W_PER_WAVE + 1);
    if (v.e_is_digest32)
        hipLaunchKernelGGL(p384_wide_a_kernel<true>, grid_a, block, 0, st, v.n, (const uint8_t*)v.e, (const uint8_t*)v.r, (const uint8_t*)v.s,
                           (uint32_t*)v.wide_scratch);
    else
        hipLaunchKernelGGL(p384_wide_a_kernel<false>, grid_a, block, 0, st, v.n, (const uint8_t*)v.e, (const uint8_t*)v.r, (const uint8_t*)v.s,
                           (uint32_t*)v.wide_scratch);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(p384_wide_b_kernel, grid_b, block, 0, st, v.n, (const uint32_t*)v.key_id, (const uint8_t*)v.r, (const uint32_t*)v.gcomb, v.snap,
                       v.nkeys, (const uint32_t*)v.wide_scratch, (uint8_t*)v.verdict_bits, (uint8_t*)v.status);
    return hipGetLastError();
}

}  // namespace fab
