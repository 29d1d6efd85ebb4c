// The comb table of a REGISTERED P-384 public key (and of the generator), its host builder, and the verification core that reads two
// of them (p384_keyed_kernels.hip; the device builder is p384_keytab_kernels.hip).  Plain C++, host and device, over p384.h: the same
// twelve canonical Montgomery words, the same complete pt_add, the same fn_inv and x_equals_r.
//
// FORMAT.  CombTab384: T[w][d] = d * 2^(8 w) * Q for w = 0 .. 47, d = 0 .. 255.  Entries are affine, x[12] y[12] canonical Montgomery
// words: 96 bytes, so every entry of a 16-byte aligned table is 16-byte aligned.  Entry 0 of every window is all zero (no lane reads
// it as a point: a zero digit loads entry 1 and drops the sum).  One table: 48 x 256 x 96 = 1 179 648 bytes (1.125 MiB).
// A field element in [0, p) has ONE canonical Montgomery form: a table built by any method is byte-identical to any other.
//
// WHAT THE TABLES BUY.  u1 G + u2 Q is 48 windows x two mixed additions and no doubling: about 1 060 field products against the 5 800
// of verify_core's doublings, per-signature table and full additions (the Fermat inverse mod n, about 690, is common to both).
#pragma once
#include "p384.h"

namespace fab {
namespace p384 {

struct CombTab384 {
    static constexpr int WINDOWS = 48;
    static constexpr int BITS = 8;
    static constexpr uint32_t DIGITS = 256;
    static constexpr int ENTRY_WORDS = 24;
    static constexpr size_t TABLE_WORDS = (size_t)WINDOWS * DIGITS * ENTRY_WORDS;
    static constexpr size_t TABLE_BYTES = TABLE_WORDS * 4;
    static FAB_HD size_t index(uint32_t w, uint32_t d) { return ((size_t)w * DIGITS + d) * ENTRY_WORDS; }
};

// the low eight bits of u; u >>= 8
FAB_HD uint32_t take_low_byte(u384& u) {
    const uint32_t d = u.w[0] & 0xffu;
#pragma unroll
    for (int i = 0; i < 11; i++) u.w[i] = (u.w[i] >> 8) | (u.w[i + 1] << 24);
    u.w[11] >>= 8;
    return d;
}

// A comb table as the core reads it: entry (w, d), d in 1 .. 255 -> affine point with Z = one.  t is 16-byte aligned.
// Tab and take are what verify_core_keyed asks of a comb type: the window count, and the next digit of a scalar.
struct CombPtr384 {
    using Tab = CombTab384;
    const uint32_t* t;
    static FAB_HD uint32_t take(u384& u) { return take_low_byte(u); }
    FAB_HD void load(jac& r, uint32_t w, uint32_t d) const {
        const u384 one = FAB_P384_ONE_MONT;
        const uint32_t* p = (const uint32_t*)__builtin_assume_aligned(t + CombTab384::index(w, d), 16);
#pragma unroll
        for (int k = 0; k < 12; k++) {
            r.X.w[k] = p[k];
            r.Y.w[k] = p[12 + k];
        }
        r.Z = one;
    }
};

// ECDSA verification of one tuple under a registered key: status 0 .. 4, the gate, the vocabulary and the precedence of verify_core.
// gcomb: the generator's comb; qcomb: the key's.  key_ok == false: the row's id names no live key (p384_keyed_kernels.hip) - the caller
// hands the generator's comb as qcomb, the whole stream runs, and the answer is 4 unless the gate refuses the row first.
// The window count and the digit width are the comb types' (CombPtr384: 48 windows of 8 bits; p384_tables16.h CombPtr384x16: 24 of 16).
// The sum runs over the windows, lowest first, two mixed additions each (the order is free: every addition is the complete pt_add, so
// an accumulator at infinity, equal to the entry (-> the doubling) or opposite to it (-> infinity) is decided as crypto/elliptic
// decides it).  A zero digit adds nothing: entry 1 is loaded, the sum computed and dropped - control flow is lane-uniform.
template <class GComb, class QComb>
FAB_HD uint32_t verify_core_keyed(const u384& e, const u384& r_in, const u384& s_in, const GComb& gcomb, const QComb& qcomb, bool key_ok = true) {
    const uint32_t early = range_status(r_in, s_in);
    u384 r = r_in, s = s_in, unit = zero384();
    unit.w[0] = 1;
    sel384(r, early == ST_VALID, r_in, unit);
    sel384(s, early == ST_VALID, s_in, unit);

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

    jac acc = pt_infinity();
    static_assert(GComb::Tab::WINDOWS == QComb::Tab::WINDOWS && GComb::Tab::BITS == QComb::Tab::BITS, "both combs of a call have one digit width");
    for (uint32_t w = 0; w < (uint32_t)GComb::Tab::WINDOWS; w++) {
        jac t, sum;
        const uint32_t d1 = GComb::take(u1), d2 = QComb::take(u2);
        gcomb.load(t, w, d1 ? d1 : 1u);
        pt_add<true>(sum, acc, t);
        sel_pt(acc, d1 != 0, sum, acc);
        qcomb.load(t, w, d2 ? d2 : 1u);
        pt_add<true>(sum, acc, t);
        sel_pt(acc, d2 != 0, sum, acc);
    }
    const bool ok = x_equals_r(acc, r);
    uint32_t st = ok ? ST_VALID : ST_BAD_MATH;
    if (!key_ok) st = ST_OFF_CURVE;
    return early != ST_VALID ? early : st;
}

// ---- host side: the builder for one key (the audit-side tests, hosttest_p384_keyed.cpp and the fallback of a failed device build) ----
// out: CombTab384::TABLE_WORDS words.  (qxm, qym): an affine point of the curve, Montgomery form.  Per window the 255 multiples are
// summed up in Jacobian form (d B = (d - 1) B + B; 2 B takes pt_add's doubling branch) together with 256 B, the next window's base,
// and brought to affine form behind ONE inversion (Montgomery's trick: prefix products, one fp_inv, and back).
inline void build_comb384(uint32_t* out, const u384& qxm, const u384& qym) {
    const u384 one = FAB_P384_ONE_MONT;
    constexpr int M = 256;                         // d = 1 .. 256
    static thread_local jac pts[M];
    static thread_local u384 pre[M];
    jac base;
    base.X = qxm; base.Y = qym; base.Z = one;
    for (uint32_t w = 0; w < (uint32_t)CombTab384::WINDOWS; w++) {
        pts[0] = base;
        for (int d = 1; d < M; d++) pt_add<true>(pts[d], pts[d - 1], base);
        pre[0] = pts[0].Z;
        for (int d = 1; d < M; d++) fp_mul(pre[d], pre[d - 1], pts[d].Z);
        u384 inv;
        fp_inv(inv, pre[M - 1]);
        uint32_t* win = out + CombTab384::index(w, 0);
        for (int k = 0; k < CombTab384::ENTRY_WORDS; k++) win[k] = 0;
        for (int d = M - 1; d >= 0; d--) {
            u384 zi, zi2, zi3, x, y;
            if (d) {
                fp_mul(zi, inv, pre[d - 1]);
                fp_mul(inv, inv, pts[d].Z);
            } else {
                zi = inv;
            }
            fp_sqr(zi2, zi);
            fp_mul(zi3, zi2, zi);
            fp_mul(x, pts[d].X, zi2);
            fp_mul(y, pts[d].Y, zi3);
            if (d == M - 1) {                      // 256 B_w = B_(w+1)
                base.X = x; base.Y = y; base.Z = one;
                continue;
            }
            uint32_t* ent = out + CombTab384::index(w, (uint32_t)d + 1);
            for (int k = 0; k < 12; k++) {
                ent[k] = x.w[k];
                ent[12 + k] = y.w[k];
            }
        }
    }
}
// ... from the key's 48 big-endian bytes each; false (and nothing written): not a point of the curve
inline bool build_comb384_be(uint32_t* out, const uint8_t* qx48, const uint8_t* qy48) {
    if (!pubkey_on_curve(qx48, qy48)) return false;
    u384 x, y, xm, ym;
    from_be48(x, qx48);
    from_be48(y, qy48);
    fp_to_mont(xm, x);
    fp_to_mont(ym, y);
    build_comb384(out, xm, ym);
    return true;
}
// the generator's plain coordinates, 48 big-endian bytes each (what both builders take)
inline void generator_be(uint8_t* gx48, uint8_t* gy48) {
    const u384 gxm = FAB_P384_GX_MONT, gym = FAB_P384_GY_MONT;
    u384 x, y;
    fp_from_mont(x, gxm);
    fp_from_mont(y, gym);
    to_be48(gx48, x);
    to_be48(gy48, y);
}
inline void build_gcomb384(uint32_t* out) {
    const u384 gxm = FAB_P384_GX_MONT, gym = FAB_P384_GY_MONT;
    build_comb384(out, gxm, gym);
}

// one tuple under a registered key on the host compilation (tests, hosttest_p384_keyed.cpp); both tables 16-byte aligned
inline uint32_t verify_keyed_host(const uint32_t* gcomb, const uint32_t* qcomb, const uint8_t* e48, const uint8_t* r48, const uint8_t* s48, bool key_ok = true) {
    u384 e, r, s;
    from_be48(e, e48); from_be48(r, r48); from_be48(s, s48);
    const CombPtr384 g{gcomb}, q{qcomb};
    return verify_core_keyed(e, r, s, g, q, key_ok);
}

}  // namespace p384
}  // namespace fab
