// Regular all-odd signed 4-bit recoding (Joye-Tunstall) of the scalar of u2*Q on P-256, for the 8-entry table of odd multiples
// {1, 3, .., 15} Q of the LDS-table pair kernels (p256_pair29.h).  Host and device: plain integer code (tests/test_pair_odd_windows_host.py
// drives it through csrc/hosttest_pair_odd.cpp).
//
// n is odd, so exactly one of u2 and n - u2 is odd: call it k; u2 Q = +-k Q.  With h = k >> 1 and h_i = (h >> 4i) & 15 the digits
//     d_i = 2 h_i - 15  (i < 63),        d_63 = 2 h_63 + 1
// are all odd, all within +-15, d_63 > 0 (k < 2^256: h_63 <= 7), and sum d_i 16^i = 2h - 15 (16^63 - 1)/15 + 16^63 = 2h + 1 = k.
// No digit is zero: the chain over them never holds infinity and never skips an addition.
#pragma once
#include "fp256.h"

namespace fab {

constexpr int ODD4_WINDOWS = 64;

// k = u2 if u2 is odd, else n - u2 (0 <= u2 < 2^256: k is odd either way, and below 2^256 for every u2 the scalar code can hand over).
// Bit 0 of k is 1 always and the recoding never reads it: on return it carries the SIGN - 1 iff k = n - u2, i.e. u2 Q = -(k | 1) Q.
FAB_HD void u2_fold_odd(u256& k, const u256& u2) {
    const u256 N = FAB_P256_N;
    u256 t;
    sub256(t, N, u2);
    const bool even = (u2.w[0] & 1u) == 0;
    sel256(k, even, t, u2);
    k.w[0] = (k.w[0] & ~1u) | (even ? 1u : 0u);
}

struct odd_digit {
    uint32_t entry;   // table entry 0..7: (2 entry + 1) Q
    bool neg;         // the addend is -(2 entry + 1) Q
};

// The digit of window value h_i = h (0..15): d = 2h - 15, or 2h + 1 for the top window (h <= 7 there).  sign: the fold's (bit 0 of k),
// applied here: the digits returned sum to u2 (mod n), not to k.
FAB_HD odd_digit odd_digit4_of(uint32_t h, bool top, bool sign) {
    const bool upper = top | (h >= 8u);                   // d > 0 before the fold's sign
    odd_digit d;
    d.entry = top ? (h & 7u) : (h >= 8u ? h - 8u : 7u - h);
    d.neg = (!upper) != sign;
    return d;
}

// Digit i (0..63) of a folded k, little-endian words with a zero ninth word: bits 4i + 1 .. 4i + 4 of k are h_i.
FAB_HD odd_digit odd_digit4(const uint32_t (&kw)[9], int i) {
    const int p = 4 * i + 1;
    const uint64_t two = ((uint64_t)kw[(p >> 5) + 1] << 32) | kw[p >> 5];
    const uint32_t h = (uint32_t)(two >> (p & 31)) & 15u;
    return odd_digit4_of(h, i == ODD4_WINDOWS - 1, (kw[0] & 1u) != 0);
}

// The same digits from the top down without indexing the scalar's words by the window (on the device a word index that is not a
// constant puts the scalar into scratch memory): h = k >> 1 in eight words, its top four bits are the next window, then h <<= 4.
// The first call returns digit 63.
struct odd_walk4 {
    u256 h;
    bool sign, top;
};
FAB_HD void odd_walk4_start(odd_walk4& w, const u256& k) {
    for (int i = 0; i < 7; i++) w.h.w[i] = (k.w[i] >> 1) | (k.w[i + 1] << 31);
    w.h.w[7] = k.w[7] >> 1;
    w.sign = (k.w[0] & 1u) != 0;
    w.top = true;
}
FAB_HD odd_digit odd_walk4_next(odd_walk4& w) {
    const odd_digit d = odd_digit4_of(w.h.w[7] >> 28, w.top, w.sign);
    for (int i = 7; i > 0; i--) w.h.w[i] = (w.h.w[i] << 4) | (w.h.w[i - 1] >> 28);
    w.h.w[0] <<= 4;
    w.top = false;
    return d;
}

}  // namespace fab
