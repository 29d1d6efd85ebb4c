// secp384r1 (NIST P-384): field, scalar and point arithmetic and the ECDSA verification core of the P-384 verify kernel
// (p384_kernels.hip).  Plain C++, host and device (FAB_HD): the CPU audit, the host tests and hosttest_p384.cpp compile this file too.
//
// What it replaces: Go 1.14 crypto/ecdsa.Verify on the generic crypto/elliptic CurveParams (math/big), reached from
// bccsp/sw/ecdsa.go:41-57 for a P-384 key.
//
// NUMBER FORM.  u384 = twelve 32-bit words, little-endian, every word a full 32 bits: a value in [0, 2^384).  Field elements and
// scalars travel in MONTGOMERY form (x R mod m, R = 2^384) and are ALWAYS CANONICAL between operations: in [0, m).  There is no lazy
// reduction and therefore one contract for every operation below:
//      in:  a, b in [0, m), every word in [0, 2^32)        out: r in [0, m), every word in [0, 2^32)
// mont_mul (CIOS, word by word):  the running sum t has 13 words (+ one transient carry word).  Every inner step is
//      v = a[j] * b[i] + t[j] + c   with a[j], b[i], t[j], c <= 2^32 - 1:   v <= (2^32-1)^2 + 2 (2^32-1) = 2^64 - 1,
// which is exactly what a uint64_t holds: no accumulator overflows, whatever the operands.  After outer step i,
//      t_i = (t_{i-1} + a b[i] + q m) / 2^32 < (2m + (2^32-1) m + (2^32-1) m) / 2^32 < 2m,
// so t[12] <= 1 and the transient t[13] <= 1; one conditional subtraction of m leaves [0, m).  For p, -p^-1 mod 2^32 = 1 (p = -1 mod 2^32):
// the quotient digit q is t[0] itself; for n it is t[0] * FAB_P384_N0INV.
// add / sub: a 12-word add or subtract with carry / borrow (uint64_t per word: at most 2^33), then one conditional correction by m;
// a + b < 2m and a - b > -m, so one correction suffices.
//
// INVERSION mod n: the Fermat ladder s^(n-2) (fn_inv).  modinv30.h's 600 division steps are proved for moduli below 2^256 only and
// are not used here.  0 maps to 0.
//
// POINTS: Jacobian (X, Y, Z), Z == 0 is the point at infinity.  pt_dbl (a = -3), pt_add (every case: either operand at infinity,
// P + P -> doubling, P + (-P) -> infinity), as crypto/elliptic's addJacobian / doubleJacobian decide them.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "fp256.h"   // FAB_HD

namespace fab {
namespace p384 {

#define FAB_P384_P {0xffffffffu, 0x00000000u, 0x00000000u, 0xffffffffu, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}
#define FAB_P384_N {0xccc52973u, 0xecec196au, 0x48b0a77au, 0x581a0db2u, 0xf4372ddfu, 0xc7634d81u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}
#define FAB_P384_HALF_N {0x666294b9u, 0x76760cb5u, 0x245853bdu, 0xac0d06d9u, 0xfa1b96efu, 0xe3b1a6c0u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu}
#define FAB_P384_P_MINUS_N {0x333ad68cu, 0x1313e696u, 0xb74f5885u, 0xa7e5f24cu, 0x0bc8d21fu, 0x389cb27eu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}
#define FAB_P384_B_MONT {0x9d412dccu, 0x08118871u, 0x7a4c32ecu, 0xf729add8u, 0x1920022eu, 0x77f2209bu, 0x94938ae2u, 0xe3374beeu, 0x1f022094u, 0xb62b21f4u, 0x604fbff9u, 0xcd08114bu}
#define FAB_P384_ONE_MONT {0x00000001u, 0xffffffffu, 0xffffffffu, 0x00000000u, 0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}
#define FAB_P384_R2_P {0x00000001u, 0xfffffffeu, 0x00000000u, 0x00000002u, 0x00000000u, 0xfffffffeu, 0x00000000u, 0x00000002u, 0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u}
#define FAB_P384_R2_N {0x19b409a9u, 0x2d319b24u, 0xdf1aa419u, 0xff3d81e5u, 0xfcb82947u, 0xbc3e483au, 0x4aab1cc5u, 0xd40d4917u, 0x28266895u, 0x3fb05b7au, 0x2b39bf21u, 0x0c84ee01u}
#define FAB_P384_ONE_MONT_N {0x333ad68du, 0x1313e695u, 0xb74f5885u, 0xa7e5f24du, 0x0bc8d220u, 0x389cb27eu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}
#define FAB_P384_GX_MONT {0x49c0b528u, 0x3dd07566u, 0xa0d6ce38u, 0x20e378e2u, 0x541b4d6eu, 0x879c3afcu, 0x59a30effu, 0x64548684u, 0x614ede2bu, 0x812ff723u, 0x299e1513u, 0x4d3aadc2u}
#define FAB_P384_GY_MONT {0x4b03a4feu, 0x23043dadu, 0x7bb4a9acu, 0xa1bfa8bfu, 0x2e83b050u, 0x8bade756u, 0x68f4ffd9u, 0xc6c35219u, 0x3969a840u, 0xdd800226u, 0x5a15c5e9u, 0x2b78abc2u}
#define FAB_P384_N0INV 0xe88fdc45u   // -n^-1 mod 2^32

enum : uint32_t { ST_VALID = 0, ST_BAD_MATH = 1, ST_HIGH_S = 2, ST_RANGE = 3, ST_OFF_CURVE = 4 };   // the P-256 vocabulary (p256_point.h)

struct u384 {
    uint32_t w[12];
};

// On the device the Montgomery product is ONE function the point operations call (576 multiply-adds each time it is inlined: a verify
// kernel that inlines ~40 of them per loop body no longer fits the instruction cache); on the host the compiler decides.
#if defined(__HIP_DEVICE_COMPILE__)
#define FAB_P384_MUL __host__ __device__ __noinline__ inline
#else
#define FAB_P384_MUL inline
#endif

FAB_HD u384 zero384() {
    u384 r;
#pragma unroll
    for (int i = 0; i < 12; i++) r.w[i] = 0;
    return r;
}
FAB_HD bool is_zero(const u384& a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) o |= a.w[i];
    return o == 0;
}
FAB_HD bool eq384(const u384& a, const u384& b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) o |= a.w[i] ^ b.w[i];
    return o == 0;
}
// r = a + b mod 2^384; returns the carry (0 / 1)
FAB_HD uint32_t add384(u384& r, const u384& a, const u384& b) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        c += (uint64_t)a.w[i] + b.w[i];   // <= 2^33 - 1
        r.w[i] = (uint32_t)c;
        c >>= 32;
    }
    return (uint32_t)c;
}
// r = a - b mod 2^384; returns the borrow (0 / 1)
FAB_HD uint32_t sub384(u384& r, const u384& a, const u384& b) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const uint64_t d = (uint64_t)a.w[i] - b.w[i] - br;
        r.w[i] = (uint32_t)d;
        br = (d >> 32) & 1u;
    }
    return (uint32_t)br;
}
FAB_HD bool lt384(const u384& a, const u384& b) {
    u384 t;
    return sub384(t, a, b) != 0;
}
FAB_HD void sel384(u384& r, bool c, const u384& a, const u384& b) {   // r = c ? a : b
#pragma unroll
    for (int i = 0; i < 12; i++) r.w[i] = c ? a.w[i] : b.w[i];
}
FAB_HD void from_be48(u384& r, const uint8_t* be) {
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const uint8_t* p = be + 4 * (11 - i);
        r.w[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
    }
}
FAB_HD void to_be48(uint8_t* be, const u384& a) {
#pragma unroll
    for (int i = 0; i < 12; i++) {
        uint8_t* p = be + 4 * (11 - i);
        p[0] = (uint8_t)(a.w[i] >> 24); p[1] = (uint8_t)(a.w[i] >> 16); p[2] = (uint8_t)(a.w[i] >> 8); p[3] = (uint8_t)a.w[i];
    }
}

// a + b mod m, a - b mod m for a, b in [0, m)
FAB_HD void mod_add(u384& r, const u384& a, const u384& b, const u384& m) {
    u384 s, d;
    const uint32_t c = add384(s, a, b);
    const uint32_t br = sub384(d, s, m);
    sel384(r, c != 0 || br == 0, d, s);     // a + b >= m (a carry out of 2^384 included: m < 2^384 <= a + b)
}
FAB_HD void mod_sub(u384& r, const u384& a, const u384& b, const u384& m) {
    u384 d, s;
    const uint32_t br = sub384(d, a, b);
    add384(s, d, m);
    sel384(r, br != 0, s, d);
}

// Montgomery product a b R^-1 mod m (CIOS; the contract and the bounds are in the file's head).  FIELD: m = p, else m = n.
template <bool FIELD>
FAB_P384_MUL u384 mont_mul(u384 a, u384 b) {
    const uint32_t M[12] = FAB_P384_P, NN[12] = FAB_P384_N;
    uint32_t t[14];
#pragma unroll
    for (int i = 0; i < 14; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        uint64_t c = 0, v;
#pragma unroll
        for (int j = 0; j < 12; j++) {
            v = (uint64_t)a.w[j] * b.w[i] + t[j] + c;      // <= 2^64 - 1
            t[j] = (uint32_t)v;
            c = v >> 32;
        }
        v = (uint64_t)t[12] + c;
        t[12] = (uint32_t)v;
        t[13] = (uint32_t)(v >> 32);
        const uint32_t q = FIELD ? t[0] : t[0] * FAB_P384_N0INV;
        v = (uint64_t)q * (FIELD ? M[0] : NN[0]) + t[0];    // low word becomes 0
        c = v >> 32;
#pragma unroll
        for (int j = 1; j < 12; j++) {
            v = (uint64_t)q * (FIELD ? M[j] : NN[j]) + t[j] + c;
            t[j - 1] = (uint32_t)v;
            c = v >> 32;
        }
        v = (uint64_t)t[12] + c;
        t[11] = (uint32_t)v;
        t[12] = t[13] + (uint32_t)(v >> 32);                // <= 1: t < 2m
    }
    u384 r, d, mm;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        r.w[i] = t[i];
        mm.w[i] = FIELD ? M[i] : NN[i];
    }
    const uint32_t br = sub384(d, r, mm);
    sel384(r, t[12] != 0 || br == 0, d, r);
    return r;
}

// ---- field mod p ----
FAB_HD void fp_mul(u384& r, const u384& a, const u384& b) { r = mont_mul<true>(a, b); }
FAB_HD void fp_sqr(u384& r, const u384& a) { r = mont_mul<true>(a, a); }
FAB_HD void fp_add(u384& r, const u384& a, const u384& b) {
    const u384 P = FAB_P384_P;
    mod_add(r, a, b, P);
}
FAB_HD void fp_sub(u384& r, const u384& a, const u384& b) {
    const u384 P = FAB_P384_P;
    mod_sub(r, a, b, P);
}
FAB_HD void fp_to_mont(u384& r, const u384& a) {   // a in [0, p)
    const u384 R2 = FAB_P384_R2_P;
    r = mont_mul<true>(a, R2);
}
FAB_HD void fp_from_mont(u384& r, const u384& a) {
    u384 one = zero384();
    one.w[0] = 1;
    r = mont_mul<true>(a, one);
}
// a^(p-2) (Montgomery form in and out; 0 -> 0): table building, on the host (build_gtab, p384_tables.h) and on the device
// (p384_keytab_kernels.hip makes its entries affine with it) - the verification itself never inverts mod p.  The exponent is a
// constant: every branch on it is uniform over a wavefront.
FAB_HD void fp_inv(u384& r, const u384& a) {
    const uint32_t P[12] = FAB_P384_P;
    const u384 one = FAB_P384_ONE_MONT;
    u384 acc = one;
    for (int i = 383; i >= 0; i--) {
        acc = mont_mul<true>(acc, acc);
        uint32_t wv = P[i >> 5];
        if (i < 32) wv -= 2;                       // p - 2: the low word of p is 0xFFFFFFFF
        if ((wv >> (i & 31)) & 1u) acc = mont_mul<true>(acc, a);
    }
    r = acc;
}

// ---- scalars mod n ----
FAB_HD void fn_mul(u384& r, const u384& a, const u384& b) { r = mont_mul<false>(a, b); }
FAB_HD void fn_to_mont(u384& r, const u384& a) {   // a in [0, n)
    const u384 R2 = FAB_P384_R2_N;
    r = mont_mul<false>(a, R2);
}
FAB_HD void fn_from_mont(u384& r, const u384& a) {
    u384 one = zero384();
    one.w[0] = 1;
    r = mont_mul<false>(a, one);
}
// a in [0, 2^384) -> a mod n (n > 2^383: one subtraction)
FAB_HD void fn_reduce_once(u384& r, const u384& a) {
    const u384 N = FAB_P384_N;
    u384 d;
    const uint32_t br = sub384(d, a, N);
    sel384(r, br == 0, d, a);
}
// s^-1 mod n = s^(n-2), Montgomery form in and out; 0 -> 0.  n - 2 = (2^192 - 1) 2^192 + L with L its low 192 bits: the upper half by
// the addition chain 1, 2, 3, 6, 12, 24, 48, 96, 192 (191 squarings, 8 products), the lower half bit by bit (192 squarings and one
// product per set bit of L).  The exponent is a constant: every branch on it is uniform over a wavefront.
FAB_HD void fn_inv(u384& r, const u384& a) {
    u384 x2, x3, x6, x12, x24, x48, x96, t;
    x2 = mont_mul<false>(mont_mul<false>(a, a), a);
    x3 = mont_mul<false>(mont_mul<false>(x2, x2), a);
    t = x3;
    for (int i = 0; i < 3; i++) t = mont_mul<false>(t, t);
    x6 = mont_mul<false>(t, x3);
    t = x6;
    for (int i = 0; i < 6; i++) t = mont_mul<false>(t, t);
    x12 = mont_mul<false>(t, x6);
    t = x12;
    for (int i = 0; i < 12; i++) t = mont_mul<false>(t, t);
    x24 = mont_mul<false>(t, x12);
    t = x24;
    for (int i = 0; i < 24; i++) t = mont_mul<false>(t, t);
    x48 = mont_mul<false>(t, x24);
    t = x48;
    for (int i = 0; i < 48; i++) t = mont_mul<false>(t, t);
    x96 = mont_mul<false>(t, x48);
    t = x96;
    for (int i = 0; i < 96; i++) t = mont_mul<false>(t, t);
    t = mont_mul<false>(t, x96);                    // a^(2^192 - 1)
    // low 192 bits of n - 2, most significant word first
    const uint32_t L[6] = {0xc7634d81u, 0xf4372ddfu, 0x581a0db2u, 0x48b0a77au, 0xecec196au, 0xccc52971u};
    for (int k = 0; k < 6; k++) {
        const uint32_t wv = L[k];
        for (int bit = 31; bit >= 0; bit--) {
            t = mont_mul<false>(t, t);
            if ((wv >> bit) & 1u) t = mont_mul<false>(t, a);
        }
    }
    r = t;
}

// ---- points ----
struct jac {
    u384 X, Y, Z;   // Montgomery form mod p; Z == 0: the point at infinity
};
FAB_HD jac pt_infinity() {
    const u384 one = FAB_P384_ONE_MONT;
    jac r;
    r.X = one; r.Y = one; r.Z = zero384();
    return r;
}
FAB_HD void sel_pt(jac& r, bool c, const jac& a, const jac& b) {
    sel384(r.X, c, a.X, b.X);
    sel384(r.Y, c, a.Y, b.Y);
    sel384(r.Z, c, a.Z, b.Z);
}

// y^2 == x^3 - 3x + b (Montgomery form, canonical)
FAB_HD bool on_curve(const u384& x, const u384& y) {
    const u384 B = FAB_P384_B_MONT;
    u384 l, x2, x3, t;
    fp_sqr(l, y);
    fp_sqr(x2, x);
    fp_mul(x3, x2, x);
    fp_add(t, x, x);
    fp_add(t, t, x);
    fp_sub(x3, x3, t);
    fp_add(x3, x3, B);
    return eq384(l, x3);
}

// Doubling, a = -3 (dbl-2001-b): 3M + 5S counted as 8 products.  Infinity (Z = 0) maps to infinity (Z3 = 2 Y Z = 0); a point of order
// two does not exist on P-384 (the group order is an odd prime), an off-curve input gives some triple and nothing else.
FAB_HD void pt_dbl(jac& r, const jac& a) {
    u384 delta, gamma, beta, alpha, t1, t2, x3, y3, z3;
    fp_sqr(delta, a.Z);
    fp_sqr(gamma, a.Y);
    fp_mul(beta, a.X, gamma);
    fp_sub(t1, a.X, delta);
    fp_add(t2, a.X, delta);
    fp_mul(alpha, t1, t2);
    fp_add(t1, alpha, alpha);
    fp_add(alpha, t1, alpha);          // 3 (X - delta)(X + delta)
    fp_add(beta, beta, beta);
    fp_add(beta, beta, beta);          // 4 beta
    fp_sqr(x3, alpha);
    fp_sub(x3, x3, beta);
    fp_sub(x3, x3, beta);              // alpha^2 - 8 beta
    fp_add(t1, a.Y, a.Y);
    fp_mul(z3, t1, a.Z);               // 2 Y Z
    fp_add(gamma, gamma, gamma);
    fp_sqr(t2, gamma);                 // 4 gamma^2
    fp_add(t2, t2, t2);                // 8 gamma^2
    fp_sub(t1, beta, x3);
    fp_mul(y3, alpha, t1);
    fp_sub(y3, y3, t2);
    r.X = x3; r.Y = y3; r.Z = z3;
}

// r = a + b, every case (crypto/elliptic addJacobian): a at infinity -> b; b at infinity -> a; a == b -> the doubling; a == -b -> infinity
// (Z3 = Z1 Z2 H = 0 by the formulas themselves).  AFFINE_B: b.Z is one (a table of affine multiples): 8M + 3S instead of 12M + 4S.
template <bool AFFINE_B>
FAB_HD void pt_add(jac& r, const jac& a, const jac& b) {
    u384 z1z1, z2z2, u1, u2, s1, s2, h, rr, hh, hhh, v, t, x3, y3, z3;
    fp_sqr(z1z1, a.Z);
    fp_mul(u2, b.X, z1z1);
    fp_mul(t, a.Z, z1z1);
    fp_mul(s2, b.Y, t);
    if (AFFINE_B) {
        u1 = a.X;
        s1 = a.Y;
    } else {
        fp_sqr(z2z2, b.Z);
        fp_mul(u1, a.X, z2z2);
        fp_mul(t, b.Z, z2z2);
        fp_mul(s1, a.Y, t);
    }
    fp_sub(h, u2, u1);
    fp_sub(rr, s2, s1);
    fp_sqr(hh, h);
    fp_mul(hhh, h, hh);
    fp_mul(v, u1, hh);
    fp_sqr(x3, rr);
    fp_sub(x3, x3, hhh);
    fp_sub(x3, x3, v);
    fp_sub(x3, x3, v);
    fp_sub(t, v, x3);
    fp_mul(y3, rr, t);
    fp_mul(t, s1, hhh);
    fp_sub(y3, y3, t);
    if (AFFINE_B) {
        fp_mul(z3, a.Z, h);
    } else {
        fp_mul(t, a.Z, b.Z);
        fp_mul(z3, t, h);
    }
    const bool a_inf = is_zero(a.Z), b_inf = is_zero(b.Z);
    jac sum;
    sum.X = x3; sum.Y = y3; sum.Z = z3;
    if (!a_inf && !b_inf && is_zero(h) && is_zero(rr)) pt_dbl(sum, a);    // P + P (rare: a branch, not a select)
    sel_pt(sum, b_inf, a, sum);
    sel_pt(r, a_inf, b, sum);
}

// x(R) mod n == r without inverting Z:  X == r Z^2, or r + n < p (r < p - n ~ 2^190) and X == (r + n) Z^2.  R at infinity: false.
FAB_HD bool x_equals_r(const jac& R, const u384& r) {
    const u384 PMN = FAB_P384_P_MINUS_N, N = FAB_P384_N;
    u384 zz, rm, t, rn;
    fp_sqr(zz, R.Z);
    fp_to_mont(rm, r);
    fp_mul(t, rm, zz);
    bool ok = eq384(t, R.X);
    add384(rn, r, N);                          // (used only when r < p - n: then r + n < p < 2^384)
    fp_to_mont(rm, lt384(r, PMN) ? rn : r);
    fp_mul(t, rm, zz);
    ok = ok || (lt384(r, PMN) && eq384(t, R.X));
    return ok && !is_zero(R.Z);
}

// the gate before the arithmetic, in the precedence of the P-256 gate (p256_point.h range_status): r or s zero or >= n: 3; s above the
// half order: 2 (bccsp/utils/ecdsa.go IsLowS on the key's own curve)
FAB_HD uint32_t range_status(const u384& r, const u384& s) {
    const u384 N = FAB_P384_N, HALF = FAB_P384_HALF_N;
    uint32_t st = ST_VALID;
    if (!lt384(r, N)) st = ST_RANGE;
    if (lt384(HALF, s)) st = ST_HIGH_S;
    if (is_zero(r) | is_zero(s)) st = ST_RANGE;
    return st;
}

// the top four bits of u; u <<= 4
FAB_HD uint32_t take_top_nibble(u384& u) {
    const uint32_t d = u.w[11] >> 28;
#pragma unroll
    for (int i = 11; i > 0; i--) u.w[i] = (u.w[i] << 4) | (u.w[i - 1] >> 28);
    u.w[0] <<= 4;
    return d;
}

constexpr int P384_TAB_ENTRIES = 15;           // j Q (or j G), j = 1 .. 15: 4-bit windows
constexpr int P384_GTAB_WORDS = 15 * 24;       // the generator's table: affine (x, y) in Montgomery form, 24 words per entry

// j G, j = 1 .. 15, affine, Montgomery form (host: built once per context and uploaded; the tests check it against Python integers)
inline void build_gtab(uint32_t* out) {
    const u384 one = FAB_P384_ONE_MONT, gx = FAB_P384_GX_MONT, gy = FAB_P384_GY_MONT;
    jac G, acc;
    G.X = gx; G.Y = gy; G.Z = one;
    acc = G;
    for (int j = 1; j <= P384_TAB_ENTRIES; j++) {
        u384 zi, zi2, zi3, x, y;
        fp_inv(zi, acc.Z);
        fp_sqr(zi2, zi);
        fp_mul(zi3, zi2, zi);
        fp_mul(x, acc.X, zi2);
        fp_mul(y, acc.Y, zi3);
        for (int k = 0; k < 12; k++) {
            out[24 * (j - 1) + k] = x.w[k];
            out[24 * (j - 1) + 12 + k] = y.w[k];
        }
        jac nx;
        pt_add<true>(nx, acc, G);
        acc = nx;
    }
}

// The generator's table as the core reads it: entry j (1 .. 15) -> affine point with Z = one
struct GTabPtr {
    const uint32_t* t;
    FAB_HD void load(jac& r, uint32_t j) const {
        const u384 one = FAB_P384_ONE_MONT;
        const uint32_t* p = t + 24 * (size_t)(j - 1);
#pragma unroll
        for (int k = 0; k < 12; k++) {
            r.X.w[k] = p[k];
            r.Y.w[k] = p[12 + k];
        }
        r.Z = one;
    }
};
// The per-signature table j Q on the host: a local array (the device keeps it in a global workspace: p384_kernels.hip)
struct LocalQTab {
    jac e[P384_TAB_ENTRIES];
    void store(uint32_t j, const jac& v) { e[j - 1] = v; }
    void load(jac& r, uint32_t j) const { r = e[j - 1]; }
};

// ECDSA verification of one tuple: status 0 .. 4 (fabgpu.h).  qx, qy, e, r, s: plain integers as the caller's 48 big-endian bytes give
// them; e is Go's hashToInt of the digest (at most 384 bits: reduced mod n here by one subtraction).
// u1 G + u2 Q in ONE accumulator over 96 interleaved 4-bit windows: four doublings, one addition from the table of Q (built here, per
// signature: 1 Q .. 15 Q, Jacobian), one mixed addition from the table of G.  A zero digit adds nothing (the sum is computed and
// dropped: lane-uniform control flow).  Every addition is the complete pt_add: an accumulator that meets +-(table entry) or is at
// infinity - u1 G = +-u2 Q, Q = +-G, u1 = 0 - is decided as crypto/elliptic decides it.
template <class GTab, class QTab>
FAB_HD uint32_t verify_core(const u384& qx, const u384& qy, const u384& e, const u384& r_in, const u384& s_in, const GTab& gtab, QTab& qtab) {
    const u384 P = FAB_P384_P, one = FAB_P384_ONE_MONT, gxm = FAB_P384_GX_MONT, gym = FAB_P384_GY_MONT;
    const uint32_t early = range_status(r_in, s_in);
    // a tuple the gate refuses still runs the whole stream, on operands inside every contract: r = s = 1, Q = G
    u384 r = r_in, s = s_in, unit = zero384();
    unit.w[0] = 1;
    sel384(r, early == ST_VALID, r_in, unit);
    sel384(s, early == ST_VALID, s_in, unit);
    jac Q;
    const bool q_in_field = lt384(qx, P) & lt384(qy, P);
    u384 x = qx, y = qy;
    sel384(x, q_in_field, qx, unit);
    sel384(y, q_in_field, qy, unit);
    fp_to_mont(Q.X, x);
    fp_to_mont(Q.Y, y);
    const bool q_ok = q_in_field && on_curve(Q.X, Q.Y);
    sel384(Q.X, q_ok, Q.X, gxm);
    sel384(Q.Y, q_ok, Q.Y, gym);
    Q.Z = one;

    // w = s^-1, u1 = e w, u2 = r w (mod n), plain integers out
    u384 sm, wm, em, rm, u1, u2, ered;
    fn_reduce_once(ered, e);
    fn_to_mont(sm, s);
    fn_inv(wm, sm);
    fn_to_mont(em, ered);
    fn_to_mont(rm, r);
    fn_mul(u1, em, wm);
    fn_mul(u2, rm, wm);
    fn_from_mont(u1, u1);
    fn_from_mont(u2, u2);

    // table of Q: 2j Q = 2 (j Q), (2j + 1) Q = 2j Q + Q
    qtab.store(1, Q);
    for (uint32_t j = 2; j <= 14; j += 2) {
        jac half, d, a;
        qtab.load(half, j >> 1);
        pt_dbl(d, half);
        qtab.store(j, d);
        pt_add<true>(a, d, Q);
        qtab.store(j + 1, a);
    }

    jac acc = pt_infinity();
    for (int i = 0; i < 96; i++) {
        jac t, sum;
        pt_dbl(t, acc);
        pt_dbl(acc, t);
        pt_dbl(t, acc);
        pt_dbl(acc, t);
        const uint32_t d2 = take_top_nibble(u2), d1 = take_top_nibble(u1);
        qtab.load(t, d2 ? d2 : 1u);
        pt_add<false>(sum, acc, t);
        sel_pt(acc, d2 != 0, sum, acc);
        gtab.load(t, d1 ? d1 : 1u);
        pt_add<true>(sum, acc, t);
        sel_pt(acc, d1 != 0, sum, acc);
    }
    const bool ok = x_equals_r(acc, r);
    uint32_t st = ok ? ST_VALID : ST_BAD_MATH;
    if (!q_ok) st = ST_OFF_CURVE;
    return early != ST_VALID ? early : st;
}

// ---- host helpers (fabgpu.h) ----
// Go 1.14 crypto/ecdsa hashToInt for a 384-bit order: a digest of 48 bytes or fewer is the integer itself, a longer one is cut to its
// leftmost 48 bytes (orderBits is a multiple of 8: no bit shift follows).
inline void hash_to_int(const uint8_t* digest, size_t len, uint8_t* e48) {
    if (len > 48) len = 48;
    for (size_t i = 0; i < 48 - len; i++) e48[i] = 0;
    for (size_t i = 0; i < len; i++) e48[48 - len + i] = digest[i];
}
inline bool pubkey_on_curve(const uint8_t* qx48, const uint8_t* qy48) {
    const u384 P = FAB_P384_P;
    u384 x, y, xm, ym;
    from_be48(x, qx48);
    from_be48(y, qy48);
    if (!lt384(x, P) || !lt384(y, P)) return false;
    fp_to_mont(xm, x);
    fp_to_mont(ym, y);
    return on_curve(xm, ym);
}
inline bool is_low_s(const uint8_t* s48) {
    const u384 HALF = FAB_P384_HALF_N;
    u384 s;
    from_be48(s, s48);
    return !lt384(HALF, s);
}
// one tuple on the host compilation (the audit, the tests, hosttest_p384.cpp)
inline uint32_t verify_host(const uint32_t* gtab, const uint8_t* qx48, const uint8_t* qy48, const uint8_t* e48, const uint8_t* r48, const uint8_t* s48) {
    u384 qx, qy, e, r, s;
    from_be48(qx, qx48); from_be48(qy, qy48); from_be48(e, e48); from_be48(r, r48); from_be48(s, s48);
    LocalQTab qt;
    GTabPtr gt{gtab};
    return verify_core(qx, qy, e, r, s, gt, qt);
}

}  // namespace p384
}  // namespace fab
