// SHA3-256 with THIRTY-TWO LANES on a message: Keccak-f[1600] with one 64-bit word of the state per lane.  For launches that cannot
// fill the chip, and for the few long messages of a large launch (sha3_coop_kernels.hip) - where one lane per message (sha3_256.h) makes
// the launch last as long as one serial chain of 5 032 instructions a block.
//
// LAYOUT.  Lane x + 5 y of a group of 32 holds A[x, y] as two dwords (lo, hi); lanes 25 .. 31 take part in the exchanges, read
// themselves and hold zeros (every step maps zeros to zeros there).  A wavefront is two groups: two messages.
// ROUND, three exchange steps one behind the other, 18 dword exchanges:
//   theta  the other four words of the lane's column (4 x 2 exchanges, independent of one another) -> C[x] on every lane of column x;
//          C[x - 1] and C[x + 1] from the neighbours of the same row (2 x 2) -> D[x] = C[x - 1] ^ rotl(C[x + 1], 1);
//   rho    the lane's own word, A ^ D, rotated by the lane's own offset: a lane-dependent 64-bit rotation on two dwords;
//   pi+chi B[x, y], B[x + 1, y], B[x + 2, y] are read straight from the lanes that hold them before pi (3 x 2) - pi alone is one lane
//          permutation, folded into chi's reads;
//   iota   lane 0.
// ABSORB.  Lane l < 17 XORs bytes [8 l, 8 l + 8) of the block into its word: three dwords of the lane's own span (and three of the prefix
// where the block still lies in it), clamped by the arena (Arena::word, as sha3_256.h), funnel-shifted by the span's byte phase.  The
// next block's dwords are requested before the current block is permuted.
// MESSAGE  =  A || B, two spans of one arena, hashed whole from the zero state: no mid-state is read.  A is a shared prefix or empty;
// the seam may fall on any byte of any block.
//
// The body is written once over an exchange policy X:
//   X::U                     a value per lane (device: a register; host: 32 entries)
//   X::lane()                the lane's number in its group, 0 .. 31
//   X::index(src)            src (a lane number per lane) made ready for X::read
//   X::read(v, index)        v of the lane named by index, within the group
//   X::map(f, u...)          f applied lane by lane
// The kernels instantiate it with wave intrinsics (sha3_coop_kernels.hip Sha3WaveX), the host with Sha3ArrayX below (hosttest_sha3_coop.cpp).
// Round constants, rotation offsets, rate, padding and block count are sha3_256.h's.
#pragma once
#include <stdint.h>

#include "sha3_256.h"

namespace fab {

constexpr int SHA3C_LANES = 32;       // lanes on one message
constexpr int SHA3C_PER_WAVE = 2;     // messages per wavefront
constexpr int SHA3C_RATE_LANES = 17;  // lanes that absorb: 136 bytes, eight a lane
constexpr int SHA3C_EXCHANGES_PER_ROUND = 18;

// low 32 bits of {hi, lo} >> s, 0 <= s < 32
FAB_HD uint32_t k_funnel0(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return s ? (lo >> s) | (hi << (32u - s)) : lo;
#endif
}

// The lane a lane reads in each exchange (l >= 25: itself).  kind 0 .. 3: the other words of its column; 4, 5: columns x - 1, x + 1 in its
// row; 6, 7, 8: where B[x + kind - 6, y] lies before pi - B[X, Y] = rotl(A[(X + 3 Y) mod 5, X])
FAB_HD uint32_t sha3c_src(uint32_t l, int kind) {
    if (l >= 25) return l;
    const uint32_t x = l % 5, y = l / 5;
    if (kind < 4) return (l + 5 * (uint32_t)(kind + 1)) % 25;
    if (kind == 4) return (x + 4) % 5 + 5 * y;
    if (kind == 5) return (x + 1) % 5 + 5 * y;
    const uint32_t bx = (x + (uint32_t)(kind - 6)) % 5;
    return (bx + 3 * y) % 5 + 5 * bx;
}

template <class X>
struct Sha3CoopLanes {
    typename X::U src[9];   // X::index of sha3c_src(l, kind)
    typename X::U ror;      // rho as a rotation to the right, (64 - offset) mod 64: its low five bits ...
    typename X::U swap;     // ... and all ones where it is 32 or more
    typename X::U first;    // all ones on lane 0 (iota)
};
template <class X>
FAB_HD Sha3CoopLanes<X> sha3_coop_lanes() {
    Sha3CoopLanes<X> k;
    const typename X::U l = X::lane();
#pragma unroll
    for (int kind = 0; kind < 9; kind++) k.src[kind] = X::index(X::map([kind](uint32_t ln) { return sha3c_src(ln, kind); }, l));
    const typename X::U right = X::map([](uint32_t ln) {   // (a chain of selects over constants: a table indexed by the lane would live in memory)
        uint32_t r = 0;
#pragma unroll
        for (int i = 0; i < 25; i++) r = ln == (uint32_t)i ? (64u - (uint32_t)sha3_rho(i)) & 63u : r;
        return r;
    }, l);
    k.ror = X::map([](uint32_t r) { return r & 31u; }, right);
    k.swap = X::map([](uint32_t r) { return r & 32u ? 0xFFFFFFFFu : 0u; }, right);
    k.first = X::map([](uint32_t ln) { return ln == 0 ? 0xFFFFFFFFu : 0u; }, l);
    return k;
}

template <class X>
FAB_HD void sha3_coop_round(const Sha3CoopLanes<X>& k, typename X::U& lo, typename X::U& hi, uint32_t rc_lo, uint32_t rc_hi) {
    using U = typename X::U;
    auto xor5 = [](uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e) { return k_xor3(k_xor3(a, b, c), d, e); };
    // theta
    const U c_lo = X::map(xor5, lo, X::read(lo, k.src[0]), X::read(lo, k.src[1]), X::read(lo, k.src[2]), X::read(lo, k.src[3]));
    const U c_hi = X::map(xor5, hi, X::read(hi, k.src[0]), X::read(hi, k.src[1]), X::read(hi, k.src[2]), X::read(hi, k.src[3]));
    const U m_lo = X::read(c_lo, k.src[4]), m_hi = X::read(c_hi, k.src[4]), p_lo = X::read(c_lo, k.src[5]), p_hi = X::read(c_hi, k.src[5]);
    auto theta = [](uint32_t a, uint32_t m, uint32_t p_this, uint32_t p_other) { return k_xor3(a, m, k_funnel(p_this, p_other, 31)); };
    const U t_lo = X::map(theta, lo, m_lo, p_lo, p_hi), t_hi = X::map(theta, hi, m_hi, p_hi, p_lo);
    // rho, by the lane's own offset: the halves change places for 32 and more, then one funnel shift each
    auto pick = [](uint32_t a, uint32_t b, uint32_t m) { return (a & m) | (b & ~m); };
    const U s_lo = X::map(pick, t_hi, t_lo, k.swap), s_hi = X::map(pick, t_lo, t_hi, k.swap);
    auto ror = [](uint32_t h, uint32_t l, uint32_t r) { return k_funnel0(h, l, r); };
    const U r_lo = X::map(ror, s_hi, s_lo, k.ror), r_hi = X::map(ror, s_lo, s_hi, k.ror);
    // pi and chi: a ^ (~b & c) over the row, each word fetched from where pi takes it from
    auto chi = [](uint32_t a, uint32_t b, uint32_t c) { return k_chi(a, b, c); };
    const U n_lo = X::map(chi, X::read(r_lo, k.src[6]), X::read(r_lo, k.src[7]), X::read(r_lo, k.src[8]));
    const U n_hi = X::map(chi, X::read(r_hi, k.src[6]), X::read(r_hi, k.src[7]), X::read(r_hi, k.src[8]));
    // iota
    lo = X::map([rc_lo](uint32_t a, uint32_t f) { return a ^ (rc_lo & f); }, n_lo, k.first);
    hi = X::map([rc_hi](uint32_t a, uint32_t f) { return a ^ (rc_hi & f); }, n_hi, k.first);
}

template <class X>
FAB_HD void sha3_coop_f1600(const Sha3CoopLanes<X>& k, typename X::U& lo, typename X::U& hi) {
#pragma unroll
    for (int r = 0; r < 24; r++) sha3_coop_round<X>(k, lo, hi, (uint32_t)sha3_rc(r), (uint32_t)(sha3_rc(r) >> 32));
}

// the dwords a lane asks for, for one block: three of B's stream (b), three of A's where the lane's eight bytes begin inside A
template <class X>
struct Sha3CoopRaw {
    typename X::U b[3], a[3];
};

// SHA3-256 of  arena[sa, sa + la) || arena[sb, sb + lb)  on the group's 32 lanes -> (lo, hi): the state, of which lanes 0 .. 3 hold the
// digest's 32 bytes.  The message's numbers are the same on every lane of the group.  maxblk: the block count the caller loops to - the
// message's own (sha3_256_blocks(la + lb)) or the largest of the wavefront; a group past its own count, or without a message
// (active false), keeps its state.
template <class X, class Arena>
FAB_HD void sha3_256_coop(const Arena& ar, uint32_t sa, uint32_t la, uint32_t sb, uint32_t lb, bool active, uint32_t maxblk, typename X::U& lo,
                          typename X::U& hi) {
    using U = typename X::U;
    const Sha3CoopLanes<X> k = sha3_coop_lanes<X>();
    const U l = X::lane();
    const uint32_t len = la + lb;
    const uint32_t nblk = active ? sha3_256_blocks(len) : 0;
    // B's bytes sit at stream position la: its stream starts at arena byte sb - la, whose dword is floor((sb - la) / 4) (sha3_256_stream2)
    const uint32_t shift_b = (sb - la) & 3u, shift_a = sa & 3u;
    const int32_t w0_b = (int32_t)(sb >> 2) + (((int32_t)(sb & 3u) - (int32_t)la) >> 2), w0_a = (int32_t)(sa >> 2);
    auto fetch = [&](uint32_t blk) {
        Sha3CoopRaw<X> r;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            r.b[j] = X::map([&ar, w0_b, blk, nblk, j](uint32_t ln) {
                return ln < (uint32_t)SHA3C_RATE_LANES && blk < nblk ? ar.word((int32_t)((uint32_t)w0_b + blk * (uint32_t)SHA3_256_RATE_WORDS + 2 * ln + (uint32_t)j)) : 0u;
            }, l);
            r.a[j] = X::map([&ar, w0_a, blk, nblk, la, j](uint32_t ln) {
                return ln < (uint32_t)SHA3C_RATE_LANES && blk < nblk && blk * SHA3_256_RATE + 8 * ln < la
                           ? ar.word((int32_t)((uint32_t)w0_a + blk * (uint32_t)SHA3_256_RATE_WORDS + 2 * ln + (uint32_t)j)) : 0u;
            }, l);
        }
        return r;
    };
    // dword `half` of the lane's eight bytes of block blk: A's bytes below la, B's from there, nothing from len on, the pad
    auto word = [=](uint32_t blk, int half) {
        return [=](uint32_t ln, uint32_t b_lo, uint32_t b_hi, uint32_t a_lo, uint32_t a_hi) {
            if (ln >= (uint32_t)SHA3C_RATE_LANES || blk >= nblk) return 0u;
            const uint32_t q = blk * SHA3_256_RATE + 8 * ln + 4 * (uint32_t)half;
            const uint32_t keep_a = k_low_bytes((int32_t)la - (int32_t)q);
            uint32_t w = (k_bytes(a_hi, a_lo, shift_a) & keep_a) | (k_bytes(b_hi, b_lo, shift_b) & ~keep_a);
            const int32_t rem = (int32_t)len - (int32_t)q;           // stream bytes left at this dword
            w &= k_low_bytes(rem);
            if (rem >= 0 && rem < 4) w |= 0x06u << (8 * rem);
            if (half == 1 && ln == (uint32_t)SHA3C_RATE_LANES - 1 && blk + 1 == nblk) w ^= 0x80000000u;   // byte 135 of the last block
            return w;
        };
    };
    lo = X::map([](uint32_t) { return 0u; }, l);
    hi = lo;
    Sha3CoopRaw<X> nxt = fetch(0);                                   // (nothing is read for a group without a message)
    for (uint32_t blk = 0; blk < maxblk; blk++) {
        const Sha3CoopRaw<X> raw = nxt;
        if (blk + 1 < maxblk) nxt = fetch(blk + 1);
        U n_lo = X::map([](uint32_t s, uint32_t w) { return s ^ w; }, lo, X::map(word(blk, 0), l, raw.b[0], raw.b[1], raw.a[0], raw.a[1]));
        U n_hi = X::map([](uint32_t s, uint32_t w) { return s ^ w; }, hi, X::map(word(blk, 1), l, raw.b[1], raw.b[2], raw.a[1], raw.a[2]));
        sha3_coop_f1600<X>(k, n_lo, n_hi);
        const uint32_t go = blk < nblk ? 0xFFFFFFFFu : 0u;
        lo = X::map([go](uint32_t nw, uint32_t old) { return (nw & go) | (old & ~go); }, n_lo, lo);
        hi = X::map([go](uint32_t nw, uint32_t old) { return (nw & go) | (old & ~go); }, n_hi, hi);
    }
}

// ---- the host's exchange policy: a group is an array of 32 entries ----
struct Sha3Vec32 {
    uint32_t v[SHA3C_LANES];
};
struct Sha3ArrayX {
    using U = Sha3Vec32;
    static U lane() {
        U r;
        for (int i = 0; i < SHA3C_LANES; i++) r.v[i] = (uint32_t)i;
        return r;
    }
    static U index(const U& src) { return src; }
    static U read(const U& v, const U& index) {
        U r;
        for (int i = 0; i < SHA3C_LANES; i++) r.v[i] = v.v[index.v[i] & (SHA3C_LANES - 1)];
        return r;
    }
    template <class F, class... A>
    static U map(F f, const A&... a) {
        U r;
        for (int i = 0; i < SHA3C_LANES; i++) r.v[i] = f(a.v[i]...);
        return r;
    }
};
// one message  A || B  inside one buffer, through the array model -> 32 bytes
inline void sha3_256_coop_host(const uint8_t* buf, size_t buf_len, uint32_t sa, uint32_t la, uint32_t sb, uint32_t lb, uint8_t out32[32]) {
    Sha3HostArena ar{buf, buf_len};
    Sha3Vec32 lo, hi;
    sha3_256_coop<Sha3ArrayX>(ar, sa, la, sb, lb, true, sha3_256_blocks(la + lb), lo, hi);
    for (int i = 0; i < 4; i++) {
        sha3_words_to_bytes(&lo.v[i], 1, out32 + 8 * i);
        sha3_words_to_bytes(&hi.v[i], 1, out32 + 8 * i + 4);
    }
}

}  // namespace fab
