// Device-side row loads shared by the P-384 kernel units (p384_kernels.hip, p384_keyed_kernels.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "p384.h"

namespace fab {

// 48 big-endian bytes of row i -> twelve little-endian words (rows are 16-byte aligned: 48 i)
__device__ __forceinline__ void load_be_field48(p384::u384& v, const uint8_t* __restrict__ base, uint32_t i) {
    const uint4* p = reinterpret_cast<const uint4*>(base + 48 * (size_t)i);
    const uint4 a = p[0], b = p[1], c = p[2];
    v.w[11] = __builtin_bswap32(a.x); v.w[10] = __builtin_bswap32(a.y); v.w[9] = __builtin_bswap32(a.z); v.w[8] = __builtin_bswap32(a.w);
    v.w[7] = __builtin_bswap32(b.x); v.w[6] = __builtin_bswap32(b.y); v.w[5] = __builtin_bswap32(b.z); v.w[4] = __builtin_bswap32(b.w);
    v.w[3] = __builtin_bswap32(c.x); v.w[2] = __builtin_bswap32(c.y); v.w[1] = __builtin_bswap32(c.z); v.w[0] = __builtin_bswap32(c.w);
}

// e of row i: 48 bytes (E32 == false), or the 32-byte digest of a 256-bit hash family, which Go's hashToInt takes as it is (a 256-bit
// integer) for a 384-bit order
template <bool E32>
__device__ __forceinline__ void load_e384(p384::u384& ve, const uint8_t* __restrict__ e, uint32_t i) {
    if (E32) {
        u256 d;
        load_be_field(d, e, i);
        ve = p384::zero384();
#pragma unroll
        for (int k = 0; k < 8; k++) ve.w[k] = d.w[k];
    } else {
        load_be_field48(ve, e, i);
    }
}

}  // namespace fab
