// HIP kernel for gfx950 (MI355X / CDNA4): batched ECDSA P-384 verification under REGISTERED keys, one signature per lane
// (p384_tables.h verify_core_keyed).  Integer VALU work only; no MFMA, no LDS, no inline assembly, no per-lane global workspace:
// the per-signature table of p384_kernels.hip is replaced by the key's comb table, which is read-only and shared by every row.
//
// Replaces (reference, CPU): bccsp/sw/ecdsa.go:41-57 -> Go 1.14 crypto/ecdsa.Verify on the generic math/big curve, for a P-384 key the
// provider has met before (bccsp.KeyImport).
//
// KEY IDS.  A row carries a uint32_t key id, generation << KEY_SLOT_BITS | slot (key_slots.h).  The launch carries a SNAPSHOT of the
// context's slots (p384_keys.h P384SlotSnap): per slot the table's address and the tenant's generation; a slot between two tenants
// shows no table and KTAB_GEN_NONE.  The host writes a snapshot once, completely, before it hands it to any launch, and never edits it.  A row whose slot is at or
// above the snapshot's high-water mark, whose generation is not the slot's, or whose slot shows no table answers status 4 and never
// another key's verdict - the rule of RegisteredKey (kernels.hip).  Such a row still runs the whole stream, on the generator's comb.
// Nothing the kernel reads changes while it runs: no table pointer is published under a running launch.
//
// 16-BIT TABLES (FABGPU_FLAG_P384_KEY_TABLES_16BIT; p384_tables16.h).  The T16 instantiations are launched only when the context has the
// generator's 16-bit table.  The snapshot then carries a second address per slot: the key's finished 16-bit table, or null.  The choice
// is made PER WAVEFRONT (a workgroup is one wavefront): if every lane's row either names a live key that shows a 16-bit table or
// answers 4 (it runs on the generator's table, which exists), the wavefront runs verify_core_keyed over 24 windows of 16 bits;
// otherwise all its lanes run the 48-window stream on the 8-bit tables, as the other instantiations do.  Lanes of one wavefront never
// take different loops; tail lanes repeat the last row and so vote as it does.  Rows, ids, the rule above, verdict words and status
// bytes are the same for every input.  rows16 grows by the rows (tail lanes not counted) of the wavefronts that ran 24 windows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "p384_dev.h"
#include "p384_keys.h"
#include "p384_tables.h"
#include "p384_tables16.h"

namespace fab {

namespace {

constexpr int P384K_BLOCK = 64;
constexpr uint32_t P384K_MAX_WGS = 1024;                         // 256 CUs x 4 SIMDs x the kernel's one wavefront per SIMD

// Tail lanes of the last tile compute on the last tuple and write nothing (kernels.hip).
template <bool E32, bool T16>
__global__ void __launch_bounds__(P384K_BLOCK) p384_verify_keyed_kernel(uint32_t n, const uint32_t* __restrict__ key_id, const uint8_t* __restrict__ e,
                                                                        const uint8_t* __restrict__ r, const uint8_t* __restrict__ s,
                                                                        const uint32_t* __restrict__ gcomb, const P384SlotSnap* __restrict__ snap,
                                                                        uint32_t nkeys, uint64_t* __restrict__ verdict_bits,
                                                                        uint8_t* __restrict__ status, const uint32_t* __restrict__ gcomb16,
                                                                        const uint32_t* const* __restrict__ snap16,
                                                                        unsigned long long* __restrict__ rows16) {
    const p384::CombPtr384 gt{gcomb};
    const uint32_t ntiles = (n - 1) / P384K_BLOCK + 1;           // (n >= 1; exact for every u32 n)
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t i = tile * P384K_BLOCK + threadIdx.x;
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
        p384::u384 ve, vr, vs;
        load_e384<E32>(ve, e, ic);
        load_be_field48(vr, r, ic);
        load_be_field48(vs, s, ic);
        uint32_t st;
        if constexpr (T16) {
            const uint32_t* qtab16 = key_ok ? snap16[slot] : gcomb16;
            if (__all(qtab16 != nullptr)) {
                const p384::CombPtr384x16 gt16{gcomb16}, qt16{qtab16};
                st = p384::verify_core_keyed(ve, vr, vs, gt16, qt16, key_ok);
                const uint32_t rows = n - tile * P384K_BLOCK;
                if (threadIdx.x == 0) atomicAdd(rows16, (unsigned long long)(rows < (uint32_t)P384K_BLOCK ? rows : (uint32_t)P384K_BLOCK));
            } else {
                st = p384::verify_core_keyed(ve, vr, vs, gt, qt, key_ok);
            }
        } else {
            st = p384::verify_core_keyed(ve, vr, vs, gt, qt, key_ok);
        }
        emit_verdict(i, active, st, verdict_bits, status);
    }
}

}  // namespace

hipError_t launch_p384_verify_keyed(const P384KeyedLaunch& v, hipStream_t st) {
    if (v.n == 0) return hipSuccess;
    if (!v.key_id || !v.e || !v.r || !v.s || !v.gcomb || !v.verdict_bits || (v.nkeys && !v.snap) || v.nkeys > (1u << KEY_SLOT_BITS)) return hipErrorInvalidValue;
    const uint32_t ntiles = (v.n - 1) / P384K_BLOCK + 1;
    dim3 grid(ntiles < P384K_MAX_WGS ? ntiles : P384K_MAX_WGS), block(P384K_BLOCK);
    const bool t16 = v.gcomb16 && v.rows16 && (v.snap16 || !v.nkeys);
    auto* kern = v.e_is_digest32 ? (t16 ? p384_verify_keyed_kernel<true, true> : p384_verify_keyed_kernel<true, false>)
                                 : (t16 ? p384_verify_keyed_kernel<false, true> : p384_verify_keyed_kernel<false, false>);
    hipLaunchKernelGGL(kern, grid, block, 0, st, v.n, (const uint32_t*)v.key_id, (const uint8_t*)v.e, (const uint8_t*)v.r, (const uint8_t*)v.s,
                       (const uint32_t*)v.gcomb, v.snap, v.nkeys, (uint64_t*)v.verdict_bits, (uint8_t*)v.status, (const uint32_t*)v.gcomb16,
                       (const uint32_t* const*)v.snap16, (unsigned long long*)v.rows16);
    return hipGetLastError();
}

}  // namespace fab
