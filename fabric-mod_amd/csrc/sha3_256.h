// SHA3-256 (FIPS 202): Keccak-f[1600], rate 136 bytes, domain byte 0x06, final bit 0x80.  Host and device: the kernels of
// sha3_kernels.hip, the CPU audit (audit_host.cpp) and the host test library (hosttest.cpp) compile this very code.
//
// Replaces (reference, CPU): bccsp/sw/hash.go for SHA3_256Opts, which identity.Verify picks for an MSP whose SignatureHashFamily is
// SHA3 (msp/identities.go:216-224).
//
// One message per lane.  The 25 x 64-bit state is 50 32-bit words (word 2 i = low half of lane i, 2 i + 1 = high half: the byte order
// of the 200-byte state as FIPS 202 lays it out), every index a compile-time constant once the loops are unrolled, so the state stays
// in registers.  A 64-bit rotation is two funnel shifts (v_alignbit_b32), a five-way parity two three-input xors, chi one three-input
// bit operation per half (v_bitop3_b32 on gfx950).  Keccak's lanes are little-endian: a message word is the arena's dword shifted to
// the message's byte phase, no byte swap.
//
// The 32-lanes-per-message form for launches that cannot fill the chip and for long messages is sha3_coop.h.
#pragma once
#include <stdint.h>

#include "fp256.h"   // FAB_HD

namespace fab {

constexpr uint32_t SHA3_256_RATE = 136;        // bytes absorbed per permutation
constexpr int SHA3_256_RATE_WORDS = 34;
constexpr int SHA3_STATE_WORDS = 50;           // 200 bytes: what a mid-state is
constexpr uint32_t SHA3_MID_BYTES = 200;

// low 32 bits of {hi, lo} >> s, 0 < s < 32
FAB_HD uint32_t k_funnel(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return (lo >> s) | (hi << (32u - s));
#endif
}
// low 32 bits of {hi, lo} >> 8 * (shift & 3)
FAB_HD uint32_t k_bytes(uint32_t hi, uint32_t lo, uint32_t shift) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, shift);
#else
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * (shift & 3u)));
#endif
}
FAB_HD uint32_t k_xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}
// a ^ (~b & c): table bit (a << 2 | b << 1 | c)
FAB_HD uint32_t k_chi(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xD2);
#else
    return a ^ (~b & c);
#endif
}
// the low n bytes of a word, n any integer (n <= 0: none, n >= 4: all)
FAB_HD uint32_t k_low_bytes(int32_t n) { return n >= 4 ? 0xFFFFFFFFu : (n <= 0 ? 0u : (0xFFFFFFFFu >> (32 - 8 * n))); }

// Keccak-f[1600]'s constants, for this file and for sha3_coop.h (functions, so that device code may index them by a lane or a loop count)
FAB_HD constexpr uint64_t sha3_rc(int round) {               // iota
    constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
                                 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
                                 0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
                                 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    return RC[round];
}
FAB_HD constexpr int sha3_rho(int i) {                       // rho: the rotation of lane A[x, y], i = x + 5 y
    constexpr int RHO[25] = {0,  1,  62, 28, 27,
                             36, 44, 6,  55, 20,
                             3,  10, 43, 25, 39,
                             41, 45, 15, 21, 8,
                             18, 2,  61, 56, 14};
    return RHO[i];
}

// (lo, hi) <- rotl64((lo, hi), N), N a constant
template <int N>
FAB_HD void k_rotl(uint32_t lo, uint32_t hi, uint32_t& olo, uint32_t& ohi) {
    if constexpr (N == 0) {
        olo = lo; ohi = hi;
    } else if constexpr (N == 32) {                      // a rename
        olo = hi; ohi = lo;
    } else if constexpr (N < 32) {
        olo = k_funnel(lo, hi, 32 - N);
        ohi = k_funnel(hi, lo, 32 - N);
    } else {
        olo = k_funnel(hi, lo, 64 - N);
        ohi = k_funnel(lo, hi, 64 - N);
    }
}

// rho and pi for lane (X, Y): B[Y, 2 X + 3 Y] = rotl(A[X, Y] ^ D[X], sha3_rho(X + 5 Y))
template <int X, int Y>
FAB_HD void k_rho_pi(const uint32_t (&a)[SHA3_STATE_WORDS], const uint32_t (&d)[10], uint32_t (&b)[SHA3_STATE_WORDS]) {
    constexpr int src = X + 5 * Y, dst = Y + 5 * ((2 * X + 3 * Y) % 5);
    k_rotl<sha3_rho(src)>(a[2 * src] ^ d[2 * X], a[2 * src + 1] ^ d[2 * X + 1], b[2 * dst], b[2 * dst + 1]);
}

template <int ROUND>
FAB_HD void keccak_round(uint32_t (&a)[SHA3_STATE_WORDS]) {
    uint32_t c[10], d[10], b[SHA3_STATE_WORDS];
    // theta: column parities, D[x] = C[x - 1] ^ rotl(C[x + 1], 1)
#pragma unroll
    for (int x = 0; x < 5; x++) {
        c[2 * x] = k_xor3(k_xor3(a[2 * x], a[2 * (x + 5)], a[2 * (x + 10)]), a[2 * (x + 15)], a[2 * (x + 20)]);
        c[2 * x + 1] = k_xor3(k_xor3(a[2 * x + 1], a[2 * (x + 5) + 1], a[2 * (x + 10) + 1]), a[2 * (x + 15) + 1], a[2 * (x + 20) + 1]);
    }
#pragma unroll
    for (int x = 0; x < 5; x++) {
        const int p = (x + 4) % 5, q = (x + 1) % 5;
        uint32_t rl, rh;
        k_rotl<1>(c[2 * q], c[2 * q + 1], rl, rh);
        d[2 * x] = c[2 * p] ^ rl;
        d[2 * x + 1] = c[2 * p + 1] ^ rh;
    }
    // rho + pi, with theta's xor folded in
    k_rho_pi<0, 0>(a, d, b); k_rho_pi<1, 0>(a, d, b); k_rho_pi<2, 0>(a, d, b); k_rho_pi<3, 0>(a, d, b); k_rho_pi<4, 0>(a, d, b); 
    k_rho_pi<0, 1>(a, d, b); k_rho_pi<1, 1>(a, d, b); k_rho_pi<2, 1>(a, d, b); k_rho_pi<3, 1>(a, d, b); k_rho_pi<4, 1>(a, d, b); 
    k_rho_pi<0, 2>(a, d, b); k_rho_pi<1, 2>(a, d, b); k_rho_pi<2, 2>(a, d, b); k_rho_pi<3, 2>(a, d, b); k_rho_pi<4, 2>(a, d, b); 
    k_rho_pi<0, 3>(a, d, b); k_rho_pi<1, 3>(a, d, b); k_rho_pi<2, 3>(a, d, b); k_rho_pi<3, 3>(a, d, b); k_rho_pi<4, 3>(a, d, b); 
    k_rho_pi<0, 4>(a, d, b); k_rho_pi<1, 4>(a, d, b); k_rho_pi<2, 4>(a, d, b); k_rho_pi<3, 4>(a, d, b); k_rho_pi<4, 4>(a, d, b); 
    // chi
#pragma unroll
    for (int y = 0; y < 5; y++) {
#pragma unroll
        for (int x = 0; x < 5; x++) {
            const int i = x + 5 * y, i1 = (x + 1) % 5 + 5 * y, i2 = (x + 2) % 5 + 5 * y;
            a[2 * i] = k_chi(b[2 * i], b[2 * i1], b[2 * i2]);
            a[2 * i + 1] = k_chi(b[2 * i + 1], b[2 * i1 + 1], b[2 * i2 + 1]);
        }
    }
    // iota
    if ((uint32_t)sha3_rc(ROUND)) a[0] ^= (uint32_t)sha3_rc(ROUND);
    if ((uint32_t)(sha3_rc(ROUND) >> 32)) a[1] ^= (uint32_t)(sha3_rc(ROUND) >> 32);
}

// Keccak-f[1600]: 24 rounds, unrolled
FAB_HD void keccak_f1600(uint32_t (&a)[SHA3_STATE_WORDS]) {
    keccak_round<0>(a);  keccak_round<1>(a);  keccak_round<2>(a);  keccak_round<3>(a);  keccak_round<4>(a);  keccak_round<5>(a);
    keccak_round<6>(a);  keccak_round<7>(a);  keccak_round<8>(a);  keccak_round<9>(a);  keccak_round<10>(a); keccak_round<11>(a);
    keccak_round<12>(a); keccak_round<13>(a); keccak_round<14>(a); keccak_round<15>(a); keccak_round<16>(a); keccak_round<17>(a);
    keccak_round<18>(a); keccak_round<19>(a); keccak_round<20>(a); keccak_round<21>(a); keccak_round<22>(a); keccak_round<23>(a);
}

FAB_HD void sha3_zero(uint32_t (&a)[SHA3_STATE_WORDS]) {
#pragma unroll
    for (int k = 0; k < SHA3_STATE_WORDS; k++) a[k] = 0;
}
// one rate block, given as 34 little-endian words
FAB_HD void sha3_256_absorb(uint32_t (&a)[SHA3_STATE_WORDS], const uint32_t (&w)[SHA3_256_RATE_WORDS]) {
#pragma unroll
    for (int k = 0; k < SHA3_256_RATE_WORDS; k++) a[k] ^= w[k];
    keccak_f1600(a);
}

// how many permutations a stream of len bytes takes: the padding needs at least one byte
FAB_HD uint32_t sha3_256_blocks(uint32_t len) { return len / SHA3_256_RATE + 1; }

// Words of an arena: Arena::word(i) is dword i of the allocation, i clamped to what may be read.
// Raw dwords of rate block blk of a stream whose byte 0 sits in arena dword w0 (possibly negative: see sha3_256_stream).  Dword
// indices, never signed byte addresses: an arena byte offset goes up to 2^32 - 1, its dword index to 2^30.
template <class Arena>
FAB_HD void sha3_fetch(const Arena& ar, int32_t w0, uint32_t blk, uint32_t (&dst)[SHA3_256_RATE_WORDS + 1]) {
    const int32_t wi = (int32_t)((uint32_t)w0 + blk * (uint32_t)SHA3_256_RATE_WORDS);   // first aligned dword (negative in block 0 of a prefixed lane whose own bytes start early)
#pragma unroll
    for (int k = 0; k < SHA3_256_RATE_WORDS + 1; k++) dst[k] = ar.word(wi + k);
}

// SHA3-256 of a lane's byte stream  A || B  continuing from state a (zero, or the mid-state of a shared prefix):
//   A = arena[sa, sa + la), la < 136   (the tail of a shared prefix that did not fill a block; la = 0 without prefix)
//   B = arena[sb, sb + lb)             (the lane's own bytes)
// The pad (0x06 ... 0x80, one byte 0x86 when the stream ends one byte short of a block) needs no length, so what the mid-state has
// absorbed does not enter.  maxblk: the block count the caller loops to - the lane's own (sha3_256_blocks(la + lb)), or on the
// device the largest of the wavefront, with `active` false for a lane that has no message; a lane past its count idles.
// any_prefix: some lane of the wavefront has la != 0.  PREFETCH: the 35 dwords of block k + 1 are requested before block k is permuted.
// sha3_256_stream2: A and B in arenas of their own - arA holds A; arB holds B, and sb is an offset into it (a lane of
// p384_described_sha3_kernels.hip whose span lies in the tail while its prefix lies in the block).
template <class ArenaA, class ArenaB, bool PREFETCH>
FAB_HD void sha3_256_stream2(const ArenaA arA, const ArenaB ar, uint32_t (&a)[SHA3_STATE_WORDS], uint32_t sa, uint32_t la, uint32_t sb, uint32_t lb,
                             bool active, bool any_prefix, uint32_t maxblk) {
    const uint32_t len = la + lb;
    const uint32_t nblk = active ? sha3_256_blocks(len) : 0;
    // B's bytes sit at stream position la: the B stream starts at arena byte sb - la, whose dword is floor((sb - la) / 4)
    const uint32_t shift = (sb - la) & 3u;
    const int32_t w0 = (int32_t)(sb >> 2) + (((int32_t)(sb & 3u) - (int32_t)la) >> 2);
    uint32_t nxt[SHA3_256_RATE_WORDS + 1];
    if (PREFETCH && maxblk) sha3_fetch(ar, w0, 0, nxt);
    for (uint32_t blk = 0; blk < maxblk; blk++) {
        uint32_t raw[SHA3_256_RATE_WORDS + 1], w[SHA3_256_RATE_WORDS];
        if (PREFETCH) {
#pragma unroll
            for (int k = 0; k < SHA3_256_RATE_WORDS + 1; k++) raw[k] = nxt[k];
            if (blk + 1 < maxblk) sha3_fetch(ar, w0, blk + 1, nxt);
        } else {
            sha3_fetch(ar, w0, blk, raw);
        }
#pragma unroll
        for (int k = 0; k < SHA3_256_RATE_WORDS; k++) w[k] = k_bytes(raw[k + 1], raw[k], shift);
        if (any_prefix && blk == 0) {                    // uniform: the prefix tail A takes the first la bytes of the first block
            uint32_t rawA[SHA3_256_RATE_WORDS + 1];
            sha3_fetch(arA, (int32_t)(sa >> 2), 0, rawA);
#pragma unroll
            for (int k = 0; k < SHA3_256_RATE_WORDS; k++) {
                const uint32_t keepA = k_low_bytes((int32_t)la - 4 * k);
                w[k] = (k_bytes(rawA[k + 1], rawA[k], sa & 3u) & keepA) | (w[k] & ~keepA);
            }
        }
        const uint32_t pos = blk * SHA3_256_RATE;
#pragma unroll
        for (int k = 0; k < SHA3_256_RATE_WORDS; k++) {  // (a full block: rem >= 4 everywhere, nothing changes)
            const int32_t rem = (int32_t)len - (int32_t)(pos + 4 * k);   // stream bytes left at this word
            uint32_t v = w[k] & k_low_bytes(rem);
            if (rem >= 0 && rem < 4) v |= 0x06u << (8 * rem);
            w[k] = v;
        }
        if (blk + 1 == nblk) w[SHA3_256_RATE_WORDS - 1] ^= 0x80000000u;   // the lane's last block: byte 135
        if (blk < nblk) sha3_256_absorb(a, w);
    }
}

template <class Arena, bool PREFETCH>
FAB_HD void sha3_256_stream(const Arena& ar, uint32_t (&a)[SHA3_STATE_WORDS], uint32_t sa, uint32_t la, uint32_t sb, uint32_t lb, bool active,
                            bool any_prefix, uint32_t maxblk) {
    sha3_256_stream2<Arena, Arena, PREFETCH>(ar, ar, a, sa, la, sb, lb, active, any_prefix, maxblk);
}

// the whole blocks of a prefix arena[start, start + len): nfull = len / 136 of them, looped to maxfull
template <class Arena, bool PREFETCH>
FAB_HD void sha3_256_midstate(const Arena& ar, uint32_t (&a)[SHA3_STATE_WORDS], uint32_t start, uint32_t nfull, uint32_t maxfull) {
    const uint32_t shift = start & 3u;
    uint32_t nxt[SHA3_256_RATE_WORDS + 1];
    if (PREFETCH && maxfull) sha3_fetch(ar, (int32_t)(start >> 2), 0, nxt);
    for (uint32_t blk = 0; blk < maxfull; blk++) {
        uint32_t raw[SHA3_256_RATE_WORDS + 1], w[SHA3_256_RATE_WORDS];
        if (PREFETCH) {
#pragma unroll
            for (int k = 0; k < SHA3_256_RATE_WORDS + 1; k++) raw[k] = nxt[k];
            if (blk + 1 < maxfull) sha3_fetch(ar, (int32_t)(start >> 2), blk + 1, nxt);
        } else {
            sha3_fetch(ar, (int32_t)(start >> 2), blk, raw);
        }
#pragma unroll
        for (int k = 0; k < SHA3_256_RATE_WORDS; k++) w[k] = k_bytes(raw[k + 1], raw[k], shift);
        if (blk < nfull) sha3_256_absorb(a, w);
    }
}

// ---- host forms over the same code: plain bytes in, bytes out (audit_host.cpp, hosttest.cpp) ----
struct Sha3HostArena {       // dword i of a byte buffer; bytes outside it read as zero
    const uint8_t* p;
    size_t n;
    uint32_t word(int32_t i) const {
        uint32_t v = 0;
        for (int k = 0; k < 4; k++) {
            const int64_t at = (int64_t)i * 4 + k;
            if (at >= 0 && (uint64_t)at < n) v |= (uint32_t)p[at] << (8 * k);
        }
        return v;
    }
};
inline void sha3_words_to_bytes(const uint32_t* a, int words, uint8_t* out) {
    for (int k = 0; k < words; k++)
        for (int j = 0; j < 4; j++) out[4 * k + j] = (uint8_t)(a[k] >> (8 * j));
}
// A || B inside one buffer, continuing from state200 (nullptr: from zero) -> 32 bytes
inline void sha3_256_host_stream(const uint8_t* buf, size_t buf_len, const uint8_t* state200, uint32_t sa, uint32_t la, uint32_t sb, uint32_t lb,
                                 uint8_t out32[32]) {
    uint32_t a[SHA3_STATE_WORDS];
    sha3_zero(a);
    if (state200)
        for (int k = 0; k < SHA3_STATE_WORDS; k++)
            a[k] = (uint32_t)state200[4 * k] | (uint32_t)state200[4 * k + 1] << 8 | (uint32_t)state200[4 * k + 2] << 16 | (uint32_t)state200[4 * k + 3] << 24;
    Sha3HostArena ar{buf, buf_len};
    sha3_256_stream<Sha3HostArena, false>(ar, a, sa, la, sb, lb, true, la != 0, sha3_256_blocks(la + lb));
    sha3_words_to_bytes(a, 8, out32);
}
inline void sha3_256_host(const uint8_t* msg, size_t len, uint8_t out32[32]) { sha3_256_host_stream(msg, len, nullptr, 0, 0, 0, (uint32_t)len, out32); }
// the state after the whole 136-byte blocks of prefix[0, len) -> 200 bytes
inline void sha3_256_host_midstate(const uint8_t* prefix, size_t len, uint8_t state200[200]) {
    uint32_t a[SHA3_STATE_WORDS];
    sha3_zero(a);
    Sha3HostArena ar{prefix, len};
    const uint32_t nfull = (uint32_t)(len / SHA3_256_RATE);
    sha3_256_midstate<Sha3HostArena, false>(ar, a, 0, nfull, nfull);
    sha3_words_to_bytes(a, SHA3_STATE_WORDS, state200);
}

}  // namespace fab
