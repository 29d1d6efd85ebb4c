// HIP kernel for gfx950 (MI355X / CDNA4): batched ECDSA P-384 verification, one signature per lane (p384.h).  Integer VALU work only
// (v_mad_u64_u32 chains); no MFMA, no LDS, no inline assembly.  Verdicts are ballot-packed as the P-256 kernels pack them
// (device_common.h emit_verdict).
//
// Replaces (reference, CPU): bccsp/sw/ecdsa.go:41-57 -> Go 1.14 crypto/ecdsa.Verify on the generic math/big curve for a P-384 key.
//
// The per-signature table 1 Q .. 15 Q (15 x 144 bytes) lives in a GLOBAL WORKSPACE, lane-major as GlobalQTab29 keeps its own
// (device_common.h): entry j of lane t is 144 contiguous bytes, a gather by digit reads nine 16-byte cells of one lane's own lines.
// LDS cannot hold it: 64 lanes x 2 160 bytes = 135 KiB per wavefront would leave one wavefront per CU.  Persistent workgroups of one
// wavefront: the workspace is sized by the grid (at most P384_MAX_WGS workgroups: 141 MB), not by the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "kernels.h"
#include "p384.h"
#include "p384_dev.h"   // load_be_field48

namespace fab {

constexpr int P384_BLOCK = 64;
constexpr uint32_t P384_MAX_WGS = 1024;                          // 256 CUs x 4 SIMDs x the kernel's one wavefront per SIMD
constexpr size_t P384_QWS_UINT4_PER_LANE = p384::P384_TAB_ENTRIES * 9;   // 15 entries x (36 words = 9 cells)

struct GlobalQTab384 {
    uint4* lane;   // first cell of this lane's table
    __device__ __forceinline__ void store(uint32_t j, const p384::jac& v) const {
        uint4* c = lane + (size_t)(j - 1) * 9;
        const uint32_t* x = v.X.w; const uint32_t* y = v.Y.w; const uint32_t* z = v.Z.w;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            c[k] = make_uint4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
            c[3 + k] = make_uint4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
            c[6 + k] = make_uint4(z[4 * k], z[4 * k + 1], z[4 * k + 2], z[4 * k + 3]);
        }
    }
    __device__ __forceinline__ void load(p384::jac& r, uint32_t j) const {
        const uint4* c = lane + (size_t)(j - 1) * 9;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint4 a = c[k], b = c[3 + k], d = c[6 + k];
            r.X.w[4 * k] = a.x; r.X.w[4 * k + 1] = a.y; r.X.w[4 * k + 2] = a.z; r.X.w[4 * k + 3] = a.w;
            r.Y.w[4 * k] = b.x; r.Y.w[4 * k + 1] = b.y; r.Y.w[4 * k + 2] = b.z; r.Y.w[4 * k + 3] = b.w;
            r.Z.w[4 * k] = d.x; r.Z.w[4 * k + 1] = d.y; r.Z.w[4 * k + 2] = d.z; r.Z.w[4 * k + 3] = d.w;
        }
    }
};

// e: n x 48 bytes (E32 == false), or n x 32 bytes - the digests of a 256-bit hash family, which Go's hashToInt takes as they are
// (a 256-bit integer) for a 384-bit order.  Tail lanes of the last tile compute on the last tuple and write nothing (kernels.hip).
template <bool E32>
__global__ void __launch_bounds__(P384_BLOCK) p384_verify_kernel(uint32_t n, const uint8_t* __restrict__ qx, const uint8_t* __restrict__ qy,
                                                                 const uint8_t* __restrict__ e, const uint8_t* __restrict__ r,
                                                                 const uint8_t* __restrict__ s, const uint32_t* __restrict__ gtab,
                                                                 uint4* __restrict__ qws, uint64_t* __restrict__ verdict_bits,
                                                                 uint8_t* __restrict__ status) {
    GlobalQTab384 qtab{qws + ((size_t)blockIdx.x * P384_BLOCK + threadIdx.x) * P384_QWS_UINT4_PER_LANE};
    const p384::GTabPtr gt{gtab};
    const uint32_t ntiles = (n - 1) / P384_BLOCK + 1;            // (n >= 1; exact for every u32 n: n + 63 would wrap above 0xFFFFFFC0)
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t i = tile * P384_BLOCK + threadIdx.x;
        const bool active = i < n;
        const uint32_t ic = active ? i : (n - 1);
        p384::u384 vqx, vqy, ve, vr, vs;
        load_be_field48(vqx, qx, ic);
        load_be_field48(vqy, qy, ic);
        if (E32) {
            u256 d;
            load_be_field(d, e, ic);
            ve = p384::zero384();
#pragma unroll
            for (int k = 0; k < 8; k++) ve.w[k] = d.w[k];
        } else {
            load_be_field48(ve, e, ic);
        }
        load_be_field48(vr, r, ic);
        load_be_field48(vs, s, ic);
        const uint32_t st = p384::verify_core(vqx, vqy, ve, vr, vs, gt, qtab);
        emit_verdict(i, active, st, verdict_bits, status);
    }
}

static uint32_t p384_grid(uint32_t n) {
    const uint32_t ntiles = n ? (n - 1) / P384_BLOCK + 1 : 0;
    return ntiles < P384_MAX_WGS ? ntiles : P384_MAX_WGS;
}
size_t p384_workspace_bytes(uint32_t n) { return (size_t)p384_grid(n) * P384_BLOCK * P384_QWS_UINT4_PER_LANE * 16; }

hipError_t launch_p384_verify(const P384Launch& v, hipStream_t st) {
    if (v.n == 0) return hipSuccess;
    if (!v.qx || !v.qy || !v.e || !v.r || !v.s || !v.gtab || !v.qws || !v.verdict_bits) return hipErrorInvalidValue;
    dim3 grid(p384_grid(v.n)), block(P384_BLOCK);
    if (v.e_is_digest32)
        hipLaunchKernelGGL(p384_verify_kernel<true>, grid, block, 0, st, v.n, (const uint8_t*)v.qx, (const uint8_t*)v.qy, (const uint8_t*)v.e,
                           (const uint8_t*)v.r, (const uint8_t*)v.s, (const uint32_t*)v.gtab, (uint4*)v.qws, (uint64_t*)v.verdict_bits, (uint8_t*)v.status);
    else
        hipLaunchKernelGGL(p384_verify_kernel<false>, grid, block, 0, st, v.n, (const uint8_t*)v.qx, (const uint8_t*)v.qy, (const uint8_t*)v.e,
                           (const uint8_t*)v.r, (const uint8_t*)v.s, (const uint32_t*)v.gtab, (uint4*)v.qws, (uint64_t*)v.verdict_bits, (uint8_t*)v.status);
    return hipGetLastError();
}

}  // namespace fab
