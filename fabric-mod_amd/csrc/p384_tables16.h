// The OPTIONAL 16-bit comb table of a registered P-384 public key (and of the generator): format, host builder, and the comb type that
// makes verify_core_keyed (p384_tables.h) run 24 windows of two mixed additions instead of 48.  Plain C++, host and device.
// The device builder is p384_keytab_kernels.hip (p384_keytab16_kernel), the reader p384_keyed_kernels.hip.
//
// FORMAT.  CombTab384x16: T16[w][d] = d * 2^(16 w) * Q for w = 0 .. 23, d = 0 .. 65 535.  Entries have CombTab384's format - affine
// x[12] y[12] canonical Montgomery words, 96 bytes, 16-byte aligned; entry 0 of every window is all zero.  One table:
// 24 x 65 536 x 96 = 150 994 944 bytes (144 MiB).  A residue has one canonical form: any two correct builders agree byte for byte.
//
// HOW IT IS BUILT.  From the key's finished 8-bit table: T16[w][hi * 256 + lo] = T8[2 w][lo] + T8[2 w + 1][hi].  lo = 0 or hi = 0 is a
// copy (a zero entry is never read as a point).  Otherwise the two points are lo B and 256 hi B for B = 2^(16 w) Q with
// 0 < lo, hi < 256: neither equal nor opposite (lo + 256 hi < 2^16 <= n / 2^368), so the sum takes no exceptional branch - the
// builders use the complete pt_add all the same.
//
// WHAT IT BUYS.  48 mixed additions instead of 96: about 530 field products beside the 690 of the Fermat inverse mod n, 1 220 against
// 1 750.
#pragma once
#include "p384_tables.h"

namespace fab {
namespace p384 {

struct CombTab384x16 {
    static constexpr int WINDOWS = 24;
    static constexpr int BITS = 16;
    static constexpr uint32_t DIGITS = 65536;
    static constexpr int ENTRY_WORDS = 24;
    static constexpr size_t WINDOW_WORDS = (size_t)DIGITS * ENTRY_WORDS;
    static constexpr size_t TABLE_WORDS = (size_t)WINDOWS * WINDOW_WORDS;
    static constexpr size_t TABLE_BYTES = TABLE_WORDS * 4;
    static FAB_HD size_t index(uint32_t w, uint32_t d) { return ((size_t)w * DIGITS + d) * ENTRY_WORDS; }
};
static_assert(CombTab384x16::TABLE_BYTES == 150994944u, "24 x 65 536 x 96");
static_assert(CombTab384x16::WINDOWS * 2 == CombTab384::WINDOWS && CombTab384x16::BITS == 2 * CombTab384::BITS, "one 16-bit window is two 8-bit windows");

// the low sixteen bits of u; u >>= 16
FAB_HD uint32_t take_low_half(u384& u) {
    const uint32_t d = u.w[0] & 0xffffu;
#pragma unroll
    for (int i = 0; i < 11; i++) u.w[i] = (u.w[i] >> 16) | (u.w[i + 1] << 16);
    u.w[11] >>= 16;
    return d;
}

// A 16-bit comb as the core reads it: entry (w, d), d in 1 .. 65 535 -> affine point with Z = one.  t is 16-byte aligned.
struct CombPtr384x16 {
    using Tab = CombTab384x16;
    const uint32_t* t;
    static FAB_HD uint32_t take(u384& u) { return take_low_half(u); }
    FAB_HD void load(jac& r, uint32_t w, uint32_t d) const {
        const u384 one = FAB_P384_ONE_MONT;
        const uint32_t* p = (const uint32_t*)__builtin_assume_aligned(t + CombTab384x16::index(w, d), 16);
#pragma unroll
        for (int k = 0; k < 12; k++) {
            r.X.w[k] = p[k];
            r.Y.w[k] = p[12 + k];
        }
        r.Z = one;
    }
};

// ---- host side ----
// Windows [w_begin, w_end) of the 16-bit table of the key whose finished 8-bit table is t8 (CombTab384::TABLE_WORDS words), into out:
// (w_end - w_begin) x CombTab384x16::WINDOW_WORDS words, window w_begin first.  Per (window, hi) the 255 sums with lo = 1 .. 255 are
// formed in Jacobian form and brought to affine form behind ONE inversion (Montgomery's trick); rows and columns with a zero byte are
// copies of the 8-bit entries, entry 0 among them.
inline void build_comb384x16(const uint32_t* t8, uint32_t w_begin, uint32_t w_end, uint32_t* out) {
    constexpr int M = 255;                         // lo = 1 .. 255
    static thread_local jac pts[M];
    static thread_local u384 pre[M];
    const CombPtr384 src{t8};
    for (uint32_t w = w_begin; w < w_end; w++) {
        uint32_t* win = out + (size_t)(w - w_begin) * CombTab384x16::WINDOW_WORDS;
        for (uint32_t hi = 0; hi < 256; hi++) {
            uint32_t* row = win + (size_t)hi * 256 * CombTab384x16::ENTRY_WORDS;
            const uint32_t* hi_ent = t8 + CombTab384::index(2 * w + 1, hi);
            if (hi == 0) {                         // T16[w][lo] = T8[2 w][lo], lo = 0 included
                const uint32_t* lo_row = t8 + CombTab384::index(2 * w, 0);
                for (size_t k = 0; k < (size_t)256 * CombTab384x16::ENTRY_WORDS; k++) row[k] = lo_row[k];
                continue;
            }
            for (int k = 0; k < CombTab384x16::ENTRY_WORDS; k++) row[k] = hi_ent[k];      // lo = 0
            jac b;
            src.load(b, 2 * w + 1, hi);
            for (int lo = 1; lo <= M; lo++) {
                jac a;
                src.load(a, 2 * w, (uint32_t)lo);
                pt_add<true>(pts[lo - 1], a, b);
            }
            pre[0] = pts[0].Z;
            for (int i = 1; i < M; i++) fp_mul(pre[i], pre[i - 1], pts[i].Z);
            u384 inv;
            fp_inv(inv, pre[M - 1]);
            for (int i = M - 1; i >= 0; i--) {
                u384 zi, zi2, zi3, x, y;
                if (i) {
                    fp_mul(zi, inv, pre[i - 1]);
                    fp_mul(inv, inv, pts[i].Z);
                } else {
                    zi = inv;
                }
                fp_sqr(zi2, zi);
                fp_mul(zi3, zi2, zi);
                fp_mul(x, pts[i].X, zi2);
                fp_mul(y, pts[i].Y, zi3);
                uint32_t* ent = row + (size_t)(i + 1) * CombTab384x16::ENTRY_WORDS;
                for (int k = 0; k < 12; k++) {
                    ent[k] = x.w[k];
                    ent[12 + k] = y.w[k];
                }
            }
        }
    }
}

// A 16-bit comb that makes the entry it is asked for, from the key's 8-bit table (host tests: the 24-window core over many keys
// without 144 MiB per key).  Entry (w, d) is what build_comb384x16 stores there, by the same rule.
struct CombOnDemand384x16 {
    using Tab = CombTab384x16;
    const uint32_t* t8;
    static uint32_t take(u384& u) { return take_low_half(u); }
    void load(jac& r, uint32_t w, uint32_t d) const {
        const u384 one = FAB_P384_ONE_MONT;
        const CombPtr384 src{t8};
        const uint32_t lo = d & 0xffu, hi = d >> 8;
        if (hi == 0 || lo == 0) {
            src.load(r, hi == 0 ? 2 * w : 2 * w + 1, hi == 0 ? lo : hi);
            return;
        }
        jac a, b, s;
        src.load(a, 2 * w, lo);
        src.load(b, 2 * w + 1, hi);
        pt_add<true>(s, a, b);
        u384 zi, zi2, zi3;
        fp_inv(zi, s.Z);
        fp_sqr(zi2, zi);
        fp_mul(zi3, zi2, zi);
        fp_mul(r.X, s.X, zi2);
        fp_mul(r.Y, s.Y, zi3);
        r.Z = one;
    }
};
// one tuple under a registered key through the 24-window instantiation of the core, both keys given by their 8-bit tables
inline uint32_t verify_keyed16_host(const uint32_t* gcomb8, const uint32_t* qcomb8, const uint8_t* e48, const uint8_t* r48, const uint8_t* s48, bool key_ok = true) {
    u384 e, r, s;
    from_be48(e, e48); from_be48(r, r48); from_be48(s, s48);
    const CombOnDemand384x16 g{gcomb8}, q{qcomb8};
    return verify_core_keyed(e, r, s, g, q, key_ok);
}

}  // namespace p384
}  // namespace fab
