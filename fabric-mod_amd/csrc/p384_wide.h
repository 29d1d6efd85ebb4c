// ECDSA P-384 verification under a REGISTERED key, split so that EIGHT LANES share one signature (p384_wide_kernels.hip): the form for
// launches that cannot fill the chip, whose time is one wavefront's instruction stream.  Plain C++, host and device, over p384.h and
// p384_tables.h: the same canonical Montgomery words, the same complete pt_add, the same fn_inv and x_equals_r; no new field code.
//
// verify_core_keyed (p384_tables.h) is a Fermat inverse mod n (about 690 products) and then 96 complete mixed additions in one chain
// (about 1 060).  The additions have no order, so the chain is cut:
//   PHASE A, one lane per signature: the gate, the substitution of a refused row, w = s^-1, u1 = e w, u2 = r w out of Montgomery form
//            -> one ROW of P384W_ROW_WORDS words: u1 (12 words, little-endian), u2 (12), the early status (1).
//   PHASE B, eight lanes per signature: lane j takes windows 6 j .. 6 j + 5 of BOTH tables - 12 complete mixed additions into its own
//            accumulator, from infinity (wide_lane_sum) - and the eight sums are joined in three levels, j ^ 1, j ^ 2, j ^ 4, by the
//            complete general addition (wide_join; the operand of the lane whose bit is clear comes first, so both lanes of a pair hold
//            the same triple).  Lane 0 decides (wide_decide).
// The serial chain behind the inverse is 12 x 11 + 3 x 16 = 180 products instead of 1 060.
//
// ONE BODY.  The kernel calls wide_phase_a, wide_lane_sum, wide_join and wide_decide; so does verify_core_keyed_split below, with a loop
// over j where the kernel has lanes and the same tree order.  What the host tests prove about the decomposition - a lane that sums
// nothing, equal or opposite partial sums meeting inside the tree, infinity at the root - they prove about the code the device runs.
#pragma once
#include "p384_tables.h"

namespace fab {
namespace p384 {

constexpr int P384W_LANES = 8;                 // lanes per signature
constexpr int P384W_WINDOWS_PER_LANE = CombTab384::WINDOWS / P384W_LANES;
constexpr int P384W_ROW_WORDS = 25;            // u1 | u2 | early status
constexpr int P384W_ROW_BYTES = 4 * P384W_ROW_WORDS;
static_assert(P384W_WINDOWS_PER_LANE * P384W_LANES == CombTab384::WINDOWS && CombTab384::BITS == 8, "six 8-bit windows per lane");

// Phase A: everything up to the scalars, exactly as verify_core_keyed does it.
FAB_HD void wide_phase_a(uint32_t* row, const u384& e, const u384& r_in, const u384& s_in) {
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
#pragma unroll
    for (int k = 0; k < 12; k++) {
        row[k] = u1.w[k];
        row[12 + k] = u2.w[k];
    }
    row[24] = early;
}

// digit w (0 .. 47) of the scalar at u[0 .. 11]
FAB_HD uint32_t wide_digit(const uint32_t* u, uint32_t w) { return (u[w >> 2] >> (8u * (w & 3u))) & 0xffu; }

// Phase B, lane j (0 .. 7): acc = sum over w = 6 j .. 6 j + 5 of T_G[w][digit w of u1] + T_Q[w][digit w of u2], from infinity.  A zero
// digit loads entry 1 and drops the sum, as in verify_core_keyed: control flow does not depend on the digits.
template <class GComb, class QComb>
FAB_HD void wide_lane_sum(jac& acc, const uint32_t* row, uint32_t j, const GComb& gcomb, const QComb& qcomb) {
    acc = pt_infinity();
    for (uint32_t k = 0; k < (uint32_t)P384W_WINDOWS_PER_LANE; k++) {
        const uint32_t w = (uint32_t)P384W_WINDOWS_PER_LANE * j + k;
        const uint32_t d1 = wide_digit(row, w), d2 = wide_digit(row + 12, w);
        jac t, sum;
        gcomb.load(t, w, d1 ? d1 : 1u);
        pt_add<true>(sum, acc, t);
        sel_pt(acc, d1 != 0, sum, acc);
        qcomb.load(t, w, d2 ? d2 : 1u);
        pt_add<true>(sum, acc, t);
        sel_pt(acc, d2 != 0, sum, acc);
    }
}

// One node of the tree: lo is the sum of the lane whose level bit is clear, hi its partner's.  Complete: either at infinity, lo == hi
// (the doubling), lo == -hi (infinity).
FAB_HD void wide_join(jac& r, const jac& lo, const jac& hi) { pt_add<false>(r, lo, hi); }

// The root's answer, with the precedence of verify_core_keyed: the early status first, then key_ok == false -> 4, then 0 or ST_BAD_MATH.
FAB_HD uint32_t wide_decide(const jac& root, const u384& r_in, uint32_t early, bool key_ok) {
    u384 r, unit = zero384();
    unit.w[0] = 1;
    sel384(r, early == ST_VALID, r_in, unit);
    const bool ok = x_equals_r(root, r);
    uint32_t st = ok ? ST_VALID : ST_BAD_MATH;
    if (!key_ok) st = ST_OFF_CURVE;
    return early != ST_VALID ? early : st;
}

// The whole verification as the two phases compute it, one lane after the other (host tests, hosttest_p384_wide.cpp): the statuses of
// verify_core_keyed, for every input.
template <class GComb, class QComb>
FAB_HD uint32_t verify_core_keyed_split(const u384& e, const u384& r, const u384& s, const GComb& gcomb, const QComb& qcomb, bool key_ok = true) {
    uint32_t row[P384W_ROW_WORDS];
    wide_phase_a(row, e, r, s);
    jac acc[P384W_LANES];
    for (uint32_t j = 0; j < (uint32_t)P384W_LANES; j++) wide_lane_sum(acc[j], row, j, gcomb, qcomb);
    for (uint32_t m = 1; m < (uint32_t)P384W_LANES; m <<= 1)
        for (uint32_t j = 0; j < (uint32_t)P384W_LANES; j += 2 * m) {
            jac t;
            wide_join(t, acc[j], acc[j + m]);
            acc[j] = t;
        }
    return wide_decide(acc[0], r, row[24], key_ok);
}

inline uint32_t verify_keyed_split_host(const uint32_t* gcomb, const uint32_t* qcomb, const uint8_t* e48, const uint8_t* r48, const uint8_t* s48, bool key_ok = true) {
    u384 e, r, s;
    from_be48(e, e48); from_be48(r, r48); from_be48(s, s48);
    const CombPtr384 g{gcomb}, q{qcomb};
    return verify_core_keyed_split(e, r, s, g, q, key_ok);
}

}  // namespace p384
}  // namespace fab
