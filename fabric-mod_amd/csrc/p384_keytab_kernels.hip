// The comb table of a registered P-384 public key (p384_tables.h CombTab384), built ON THE DEVICE: the three launches of
// keytab_kernels.hip over p384.h's arithmetic.  HIP for gfx950; integer VALU only, no LDS, no inline assembly.
//
// What it replaces: nothing on the reference's side does this work at all - Go's crypto/ecdsa multiplies from scratch per signature;
// on this side it replaces p384_tables.h::build_comb384 on a host thread.  The output is BYTE-IDENTICAL to that builder's
// (tests/test_p384_keyed_gpu.py compares them): every coordinate is the one canonical Montgomery form of an integer in [0, p).
//
//   chain    one lane per key: B_w = 2^(8 w) Q, w = 0 .. 47 - 376 dependent doublings, the critical path;
//   affine   one lane per (key, window): B_w to affine (Fermat inverse mod p: fp_inv), so that the entries need mixed additions only;
//   entries  one lane per (key, window, digit): d B_w by double-and-add from the affine base (<= 7 doublings, <= 7 mixed additions),
//            its own inversion, and a 96-byte store (consecutive lanes = consecutive digits of a window: six 16-byte cells each,
//            a wavefront writes 6 KiB of contiguous memory).
// Exceptional cases cannot occur for a point of the curve (prime order, every intermediate is k B_w with 1 <= k <= 255); the
// additions are the complete pt_add all the same.  Every key must be an affine point of the curve: the callers' gate.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "p384_dev.h"
#include "p384_tables.h"

namespace fab {

namespace {

using p384::CombTab384;
using p384::jac;
using p384::u384;

struct KeyBaseAffine384 {
    u384 x, y;
};

__device__ void jac_to_affine384(u384& x, u384& y, const jac& p) {
    u384 zi, zi2, zi3;
    p384::fp_inv(zi, p.Z);
    p384::fp_sqr(zi2, zi);
    p384::fp_mul(zi3, zi2, zi);
    p384::fp_mul(x, p.X, zi2);
    p384::fp_mul(y, p.Y, zi3);
}

__global__ void __launch_bounds__(64) p384_keytab_chain_kernel(uint32_t n_keys, const uint8_t* __restrict__ qxy, jac* __restrict__ bases) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_keys) return;
    const u384 one = FAB_P384_ONE_MONT;
    u384 qx, qy;
    load_be_field48(qx, qxy, 2 * k);
    load_be_field48(qy, qxy, 2 * k + 1);
    jac acc;
    p384::fp_to_mont(acc.X, qx);
    p384::fp_to_mont(acc.Y, qy);
    acc.Z = one;
    bases[(size_t)k * CombTab384::WINDOWS] = acc;
    for (int w = 1; w < CombTab384::WINDOWS; w++) {
        for (int b = 0; b < CombTab384::BITS; b++) {
            jac t;
            p384::pt_dbl(t, acc);
            acc = t;
        }
        bases[(size_t)k * CombTab384::WINDOWS + w] = acc;
    }
}

__global__ void __launch_bounds__(64) p384_keytab_affine_kernel(uint32_t n_bases, const jac* __restrict__ bases, KeyBaseAffine384* __restrict__ aff) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_bases) return;
    const jac b = bases[i];
    KeyBaseAffine384 a;
    jac_to_affine384(a.x, a.y, b);
    aff[i] = a;
}

__global__ void __launch_bounds__(256) p384_keytab_entries_kernel(uint32_t n_keys, const KeyBaseAffine384* __restrict__ aff, uint32_t* const* __restrict__ tabs) {
    constexpr uint32_t PER_KEY = (uint32_t)CombTab384::WINDOWS * CombTab384::DIGITS;
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t key = id / PER_KEY, rem = id % PER_KEY, w = rem / CombTab384::DIGITS, d = rem % CombTab384::DIGITS;
    if (key >= n_keys) return;
    uint4* e = reinterpret_cast<uint4*>(tabs[key] + CombTab384::index(w, d));
    if (d == 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) e[c] = make_uint4(0, 0, 0, 0);
        return;
    }
    const KeyBaseAffine384 base = aff[(size_t)key * CombTab384::WINDOWS + w];
    u384 x = base.x, y = base.y;
    if (d != 1) {
        const u384 one = FAB_P384_ONE_MONT;
        jac b, acc;
        b.X = base.x; b.Y = base.y; b.Z = one;
        acc = b;
        const int top = 31 - __clz((int)d);
        for (int bit = top - 1; bit >= 0; bit--) {
            jac t;
            p384::pt_dbl(t, acc);
            acc = t;
            if ((d >> bit) & 1u) {
                p384::pt_add<true>(t, acc, b);
                acc = t;
            }
        }
        jac_to_affine384(x, y, acc);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        e[c] = make_uint4(x.w[4 * c], x.w[4 * c + 1], x.w[4 * c + 2], x.w[4 * c + 3]);
        e[3 + c] = make_uint4(y.w[4 * c], y.w[4 * c + 1], y.w[4 * c + 2], y.w[4 * c + 3]);
    }
}

size_t bases_bytes(uint32_t n_keys) { return ((size_t)n_keys * CombTab384::WINDOWS * sizeof(jac) + 15) & ~(size_t)15; }

}  // namespace

size_t p384_keytab_scratch_bytes(uint32_t n_keys) { return bases_bytes(n_keys) + (size_t)n_keys * CombTab384::WINDOWS * sizeof(KeyBaseAffine384); }

// qxy: n_keys x 96 bytes (X || Y, 48 big-endian bytes each) on the device, 16-byte aligned; tabs: n_keys device pointers (on the device)
// to 16-byte aligned tables of CombTab384::TABLE_BYTES each; scratch: p384_keytab_scratch_bytes(n_keys), 16-byte aligned.
hipError_t launch_p384_keytab_build(uint32_t n_keys, const void* qxy, void* const* tabs, void* scratch, hipStream_t st) {
    if (n_keys == 0) return hipSuccess;
    if (!qxy || !tabs || !scratch || n_keys > (1u << KEY_SLOT_BITS)) return hipErrorInvalidValue;
    jac* bases = (jac*)scratch;
    KeyBaseAffine384* aff = (KeyBaseAffine384*)((uint8_t*)scratch + bases_bytes(n_keys));
    hipLaunchKernelGGL(p384_keytab_chain_kernel, dim3((n_keys + 63) / 64), dim3(64), 0, st, n_keys, (const uint8_t*)qxy, bases);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t nb = n_keys * (uint32_t)CombTab384::WINDOWS;
    hipLaunchKernelGGL(p384_keytab_affine_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, nb, (const jac*)bases, aff);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t lanes = nb * CombTab384::DIGITS;            // (<= 4096 x 48 x 256 = 2^25 x 1.5: a u32)
    hipLaunchKernelGGL(p384_keytab_entries_kernel, dim3(lanes / 256), dim3(256), 0, st, n_keys, (const KeyBaseAffine384*)aff, (uint32_t* const*)tabs);
    return hipGetLastError();
}

}  // namespace fab
