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
// A fourth kernel, p384_keytab16_kernel (below, with its own story), makes the optional 16-bit table from a finished 8-bit one; it is
// the one kernel of this unit that uses LDS.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "p384_dev.h"
#include "p384_tables.h"
#include "p384_tables16.h"

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

// ---- the optional 16-bit table (p384_tables16.h CombTab384x16) from the key's FINISHED 8-bit table ----
// T16[w][hi * 256 + lo] = T8[2 w][lo] + T8[2 w + 1][hi]: both terms are affine, so the sum is the affine chord rule,
//   l = (yb - ya) / (xb - xa),  x = l^2 - xa - xb,  y = l (xa - x) - ya,
// and the only inversion is of xb - xa, which is never zero for lo, hi != 0 (p384_tables16.h: the two points are neither equal nor
// opposite).  One wavefront per 1 024 consecutive digits of a window; lane l takes the T16_RUN digits base + 64 j + l, so that in every
// store instruction consecutive lanes write consecutive 96-byte entries (six 16-byte cells each: a wavefront writes 6 KiB of contiguous
// memory per step, as the 8-bit entries kernel does).  The lane's T16_RUN denominators share ONE fp_inv behind Montgomery's trick: the
// forward pass leaves the prefix products in LDS (word k of step j of lane l at [j][k][l]: conflict-free), the backward pass recomputes
// each denominator from the 8-bit table (1.125 MiB, cache-resident) instead of keeping it.  A digit with lo = 0 or hi = 0 is a copy of
// the 8-bit entry (entry 0 of the 8-bit window is zero, so digit 0 comes out zero); its denominator is replaced by one.
// Per entry: 1 product forward, 5 backward, and 1 / T16_RUN of an fp_inv (384 squarings + 318 products).
constexpr int T16_RUN = 16;
constexpr uint32_t T16_WAVE_DIGITS = 64u * T16_RUN;
constexpr uint32_t T16_WAVES_PER_WINDOW = p384::CombTab384x16::DIGITS / T16_WAVE_DIGITS;
static_assert(p384::CombTab384x16::DIGITS % T16_WAVE_DIGITS == 0, "a wavefront stays inside one window");

__device__ __forceinline__ void load_xy384(u384& x, u384& y, const uint32_t* __restrict__ t8, uint32_t w, uint32_t d) {
    const uint4* p = reinterpret_cast<const uint4*>(t8 + CombTab384::index(w, d));
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint4 a = p[c], b = p[3 + c];
        x.w[4 * c] = a.x; x.w[4 * c + 1] = a.y; x.w[4 * c + 2] = a.z; x.w[4 * c + 3] = a.w;
        y.w[4 * c] = b.x; y.w[4 * c + 1] = b.y; y.w[4 * c + 2] = b.z; y.w[4 * c + 3] = b.w;
    }
}

__global__ void __launch_bounds__(64) p384_keytab16_kernel(const uint32_t* __restrict__ t8, uint32_t* __restrict__ t16) {
    __shared__ uint32_t pre[T16_RUN][12][64];
    const u384 one = FAB_P384_ONE_MONT;
    const uint32_t lane = threadIdx.x;
    const uint32_t w = blockIdx.x / T16_WAVES_PER_WINDOW;                    // (the grid is exactly 24 x T16_WAVES_PER_WINDOW blocks)
    const uint32_t base = (blockIdx.x % T16_WAVES_PER_WINDOW) * T16_WAVE_DIGITS + lane;
    u384 acc = one;
    for (int j = 0; j < T16_RUN; j++) {
        const uint32_t d = base + 64u * (uint32_t)j, lo = d & 0xffu, hi = d >> 8;
        u384 xa, ya, xb, yb, dx;
        load_xy384(xa, ya, t8, 2 * w, lo);
        load_xy384(xb, yb, t8, 2 * w + 1, hi);
        p384::fp_sub(dx, xb, xa);
        p384::sel384(dx, lo != 0 && hi != 0, dx, one);
#pragma unroll
        for (int k = 0; k < 12; k++) pre[j][k][lane] = acc.w[k];             // the product of the denominators before this one
        p384::fp_mul(acc, acc, dx);
    }
    u384 inv;
    p384::fp_inv(inv, acc);
    for (int j = T16_RUN - 1; j >= 0; j--) {
        const uint32_t d = base + 64u * (uint32_t)j, lo = d & 0xffu, hi = d >> 8;
        u384 xa, ya, xb, yb, dx, dy, pj, di, l, x, y, t;
        load_xy384(xa, ya, t8, 2 * w, lo);
        load_xy384(xb, yb, t8, 2 * w + 1, hi);
        p384::fp_sub(dx, xb, xa);
        p384::sel384(dx, lo != 0 && hi != 0, dx, one);
#pragma unroll
        for (int k = 0; k < 12; k++) pj.w[k] = pre[j][k][lane];
        p384::fp_mul(di, inv, pj);                                           // 1 / dx
        p384::fp_mul(inv, inv, dx);
        p384::fp_sub(dy, yb, ya);
        p384::fp_mul(l, dy, di);
        p384::fp_sqr(x, l);
        p384::fp_sub(x, x, xa);
        p384::fp_sub(x, x, xb);
        p384::fp_sub(t, xa, x);
        p384::fp_mul(y, l, t);
        p384::fp_sub(y, y, ya);
        p384::sel384(x, lo == 0, xb, x);                                     // copies: lo = 0 -> the hi entry; hi = 0 -> the lo entry (zero for digit 0)
        p384::sel384(y, lo == 0, yb, y);
        p384::sel384(x, hi == 0, xa, x);
        p384::sel384(y, hi == 0, ya, y);
        uint4* e = reinterpret_cast<uint4*>(t16 + p384::CombTab384x16::index(w, d));
#pragma unroll
        for (int c = 0; c < 3; c++) {
            e[c] = make_uint4(x.w[4 * c], x.w[4 * c + 1], x.w[4 * c + 2], x.w[4 * c + 3]);
            e[3 + c] = make_uint4(y.w[4 * c], y.w[4 * c + 1], y.w[4 * c + 2], y.w[4 * c + 3]);
        }
    }
}

// The check of the test-hook library (fabgpu_test_p384_key_table16): every entry of t16 against T8[2 w][lo] + T8[2 w + 1][hi] by another
// road - the complete Jacobian pt_add and a projective comparison (x Z^2 == X, y Z^3 == Y), no inversion.  One lane per entry; *bad
// counts the entries that differ.
__global__ void __launch_bounds__(256) p384_keytab16_check_kernel(const uint32_t* __restrict__ t8, const uint32_t* __restrict__ t16, unsigned long long* __restrict__ bad) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;              // (the grid is exactly 24 x 65 536 lanes)
    const uint32_t w = id / p384::CombTab384x16::DIGITS, d = id % p384::CombTab384x16::DIGITS, lo = d & 0xffu, hi = d >> 8;
    const uint32_t* e = t16 + p384::CombTab384x16::index(w, d);
    u384 x, y;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        x.w[k] = e[k];
        y.w[k] = e[12 + k];
    }
    bool ok;
    if (lo == 0 || hi == 0) {
        u384 sx, sy;
        load_xy384(sx, sy, t8, hi == 0 ? 2 * w : 2 * w + 1, hi == 0 ? lo : hi);
        ok = p384::eq384(x, sx) && p384::eq384(y, sy);
    } else {
        const p384::CombPtr384 src{t8};
        jac a, b, s;
        src.load(a, 2 * w, lo);
        src.load(b, 2 * w + 1, hi);
        p384::pt_add<true>(s, a, b);
        u384 z2, z3, lx, ly;
        p384::fp_sqr(z2, s.Z);
        p384::fp_mul(z3, z2, s.Z);
        p384::fp_mul(lx, x, z2);
        p384::fp_mul(ly, y, z3);
        ok = !p384::is_zero(s.Z) && p384::eq384(lx, s.X) && p384::eq384(ly, s.Y);
    }
    if (!ok) atomicAdd(bad, 1ull);
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

hipError_t launch_p384_keytab16_build(const void* tab8, void* tab16, hipStream_t st) {
    if (!tab8 || !tab16 || ((uintptr_t)tab8 & 15) || ((uintptr_t)tab16 & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(p384_keytab16_kernel, dim3((uint32_t)p384::CombTab384x16::WINDOWS * T16_WAVES_PER_WINDOW), dim3(64), 0, st, (const uint32_t*)tab8,
                       (uint32_t*)tab16);
    return hipGetLastError();
}

hipError_t launch_p384_keytab16_check(const void* tab8, const void* tab16, void* bad, hipStream_t st) {
    if (!tab8 || !tab16 || !bad) return hipErrorInvalidValue;
    hipLaunchKernelGGL(p384_keytab16_check_kernel, dim3((uint32_t)p384::CombTab384x16::WINDOWS * p384::CombTab384x16::DIGITS / 256), dim3(256), 0, st,
                       (const uint32_t*)tab8, (const uint32_t*)tab16, (unsigned long long*)bad);
    return hipGetLastError();
}

}  // namespace fab
