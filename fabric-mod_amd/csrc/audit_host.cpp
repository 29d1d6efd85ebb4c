// CPU audit of device results (audit_host.h): SHA-256 in plain C++, SHA3-256 through sha3_256.h, ECDSA P-256 verification and idemix
// pseudonym-signature verification through the kernels' own one-lane header code compiled for the host.  Linked into libfabgpu.so;
// nothing here touches a device.
#include "audit_host.h"

#include <string.h>

#include <memory>
#include <mutex>
#include <vector>

#include "bccsp_host.h"
#include "bn_tables29.h"
#include "idemix_host.h"
#include "p256_tables29.h"
#include "sha3_256.h"
#include "p384.h"

namespace fab {
namespace bccsp {

// ------------------------------------------------------------------------------------------------
// SHA-256 (FIPS 180-4)
// ------------------------------------------------------------------------------------------------
namespace {
const uint32_t K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

void compress(uint32_t h[8], const uint8_t* p) {
    uint32_t w[64];
    for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
        const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
        const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
        const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
}  // namespace

void audit_sha256(const uint8_t* msg, size_t len, uint8_t* out32) {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    size_t at = 0;
    for (; at + 64 <= len; at += 64) compress(h, msg + at);
    uint8_t last[128];
    const size_t rem = len - at;
    memset(last, 0, sizeof(last));
    if (rem) memcpy(last, msg + at, rem);
    last[rem] = 0x80;
    const size_t total = rem + 9 <= 64 ? 64 : 128;
    const uint64_t bits = (uint64_t)len << 3;
    for (int i = 0; i < 8; i++) last[total - 1 - i] = (uint8_t)(bits >> (8 * i));
    compress(h, last);
    if (total == 128) compress(h, last + 64);
    for (int i = 0; i < 8; i++) {
        out32[4 * i] = (uint8_t)(h[i] >> 24);
        out32[4 * i + 1] = (uint8_t)(h[i] >> 16);
        out32[4 * i + 2] = (uint8_t)(h[i] >> 8);
        out32[4 * i + 3] = (uint8_t)h[i];
    }
}

// SHA3-256 (FIPS 202): the stream code of the device's lanes over the caller's bytes
void audit_sha3_256(const uint8_t* msg, size_t len, uint8_t* out32) { sha3_256_host(msg, len, out32); }

// ------------------------------------------------------------------------------------------------
// ECDSA P-256
// ------------------------------------------------------------------------------------------------
namespace {
// the generator's 8-bit comb (what a registered key gets on the device: 32 windows x 256 entries, 640 KiB), built at the first audit
const KeyTab8& generator_comb() {
    static std::vector<int32_t> words;
    static KeyTab8 tab{nullptr};
    static std::once_flag once;
    std::call_once(once, [] {
        const u256 gx = FAB_P256_GX_PLAIN, gy = FAB_P256_GY_PLAIN;
        words.resize(KeyTab8::TABLE_WORDS);
        build_key_comb_table8(words.data(), gx, gy);
        tab.w = words.data();
    });
    return tab;
}

// p256_verify_core29 with the generator on an 8-bit comb instead of the device's 80 MiB 16-bit one: u2*Q over a per-call table of Q,
// u1*G over the comb, separate accumulators, one final addition, x(R) == r (mod n) without an inversion.
uint32_t verify_core(const u256& qx, const u256& qy, const u256& e, const u256& r, const u256& s) {
    const u256 P = FAB_P256_P;
    const fe ONE = {FE29_R1};
    const uint32_t early = range_status(r, s);
    if (early != ST_VALID) return early;
    if (!(lt256(qx, P) & lt256(qy, P))) return ST_OFF_CURVE;
    jac29 Q;
    fe_to_mont(Q.X, qx);
    fe_to_mont(Q.Y, qy);
    Q.Z = ONE;
    if (!on_curve29(Q.X, Q.Y)) return ST_OFF_CURVE;
    u256 u1, u2;
    ecdsa_scalars29(u1, u2, e, r, s);
    jac29 T, S, Rr;
    bool t_inf, s_inf, r_inf;
    LocalQTab29 qtab;
    var_base_mult29(T, t_inf, u2, Q, qtab);
    comb_mult29(S, s_inf, u1, generator_comb(), Q);
    final_add29(Rr, r_inf, S, s_inf, T, t_inf);
    return x_equals_r29(Rr, r_inf, r) ? ST_VALID : ST_BAD_MATH;
}
}  // namespace

bool audit_p256_verify(const uint8_t* qx32, const uint8_t* qy32, const uint8_t* sig_der, size_t siglen, const uint8_t* digest, size_t dlen) {
    if (!qx32 || !qy32 || !sig_der || !digest || siglen == 0 || dlen == 0) return false;   // bccsp/sw/impl.go:249-257
    BigInt R, S;
    if (!UnmarshalECDSASignature(sig_der, siglen, R, S).ok()) return false;               // DER; r, s > 0
    if (!IsLowS(S)) return false;
    if (!R.fits256() || !S.fits256()) return false;                                      // r >= 2^256 > n: ecdsa.Verify says false
    if (!PublicKeyOnCurve(qx32, qy32)) return false;
    uint8_t r32[32], s32[32], e32[32];
    R.to_be32(r32);
    S.to_be32(s32);
    HashToInt(digest, dlen, e32);
    u256 qx, qy, e, r, s;
    from_be32(qx, qx32);
    from_be32(qy, qy32);
    from_be32(e, e32);
    from_be32(r, r32);
    from_be32(s, s32);
    return verify_core(qx, qy, e, r, s) == ST_VALID;
}

// ------------------------------------------------------------------------------------------------
// ECDSA P-384: p384.h compiled for the host (the generator's fifteen multiples are built at the first audit)
// ------------------------------------------------------------------------------------------------
bool audit_p384_verify(const uint8_t* qx48, const uint8_t* qy48, const uint8_t* sig_der, size_t siglen, const uint8_t* digest, size_t dlen) {
    if (!qx48 || !qy48 || !sig_der || !digest || siglen == 0 || dlen == 0) return false;
    BigInt R, S;
    if (!UnmarshalECDSASignature(sig_der, siglen, R, S).ok()) return false;
    uint8_t rs[2][48], e48[48];
    const BigInt* v[2] = {&R, &S};
    for (int k = 0; k < 2; k++) {
        const std::vector<uint8_t> m = v[k]->magnitude();
        if (m.size() > 48) return false;                                                  // above 2^384 > n
        memset(rs[k], 0, 48);
        if (!m.empty()) memcpy(rs[k] + 48 - m.size(), m.data(), m.size());
    }
    static uint32_t gtab[p384::P384_GTAB_WORDS];
    static std::once_flag once;
    std::call_once(once, [] { p384::build_gtab(gtab); });
    p384::hash_to_int(digest, dlen, e48);
    return p384::verify_host(gtab, qx48, qy48, e48, rs[0], rs[1]) == p384::ST_VALID;      // (its gate: low s, ranges, the key on the curve)
}

// ------------------------------------------------------------------------------------------------
// Idemix pseudonym signature (idemix/nymsignature.go:74-109) on FP256BN's G1
// ------------------------------------------------------------------------------------------------
namespace {
// The 8-bit combs of one issuer's HSk and HRand (what fabgpu_idemix_issuer_register puts on the device), built at the issuer's first
// audit.  A peer has a handful of idemix MSPs: the last kIssuerTabs issuers are kept, the least recently used one goes first.
struct IssuerCombs {
    uint8_t bases[128];                      // hsk_x || hsk_y || hrand_x || hrand_y
    std::vector<int32_t> hsk, hrand;
    bool usable = false;                     // both bases are points of G1 with coordinates below p
    uint64_t used = 0;
};
constexpr size_t kIssuerTabs = 8;

bool bn_base_ok(const u256& x, const u256& y) {
    const u256 P = FAB_BN_P;
    if (!(lt256(x, P) & lt256(y, P))) return false;
    fbn mx, my;
    fe_to_mont(mx, x);
    fe_to_mont(my, y);
    return bn_on_curve29(mx, my);
}

std::shared_ptr<const IssuerCombs> issuer_combs(const uint8_t* hsk_x32, const uint8_t* hsk_y32, const uint8_t* hrand_x32, const uint8_t* hrand_y32) {
    static std::mutex mu;
    static std::vector<std::shared_ptr<IssuerCombs>> held;
    static uint64_t tick = 0;
    uint8_t bases[128];
    memcpy(bases, hsk_x32, 32);
    memcpy(bases + 32, hsk_y32, 32);
    memcpy(bases + 64, hrand_x32, 32);
    memcpy(bases + 96, hrand_y32, 32);
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto& c : held)
            if (!memcmp(c->bases, bases, 128)) {
                c->used = ++tick;
                return c;
            }
    }
    // built outside the lock (6 ms a base); two threads that meet a new issuer at once both build, one copy stays
    std::shared_ptr<IssuerCombs> c(new IssuerCombs);
    memcpy(c->bases, bases, 128);
    u256 sx, sy, rx, ry;
    from_be32(sx, hsk_x32);
    from_be32(sy, hsk_y32);
    from_be32(rx, hrand_x32);
    from_be32(ry, hrand_y32);
    c->usable = bn_base_ok(sx, sy) && bn_base_ok(rx, ry);
    if (c->usable) {
        c->hsk.resize(KeyTab8::TABLE_WORDS);
        c->hrand.resize(KeyTab8::TABLE_WORDS);
        build_bn_comb_table8(c->hsk.data(), sx, sy);
        build_bn_comb_table8(c->hrand.data(), rx, ry);
    }
    std::lock_guard<std::mutex> lk(mu);
    for (auto& o : held)
        if (!memcmp(o->bases, bases, 128)) return o;
    c->used = ++tick;
    if (held.size() >= kIssuerTabs) {
        size_t oldest = 0;
        for (size_t i = 1; i < held.size(); i++)
            if (held[i]->used < held[oldest]->used) oldest = i;
        held[oldest] = c;
    } else {
        held.push_back(c);
    }
    return c;
}

// HashModOrder (idemix/util.go:46-51): SHA-256 of the bytes as a big-endian number, mod the group order
void hash_mod_order(u256& out, const uint8_t* data, size_t len) {
    uint8_t dg[32];
    audit_sha256(data, len, dg);
    u256 x;
    from_be32(x, dg);
    bn_mod_order(out, x);
}
}  // namespace

bool audit_nym_verify(const uint8_t* hsk_x32, const uint8_t* hsk_y32, const uint8_t* hrand_x32, const uint8_t* hrand_y32, const uint8_t* ipk_hash32,
                      const uint8_t* nym_x32, const uint8_t* nym_y32, const uint8_t* sig, size_t siglen, const uint8_t* msg, size_t msglen) {
    if (!hsk_x32 || !hsk_y32 || !hrand_x32 || !hrand_y32 || !ipk_hash32 || !nym_x32 || !nym_y32) return false;
    if (!sig || siglen == 0 || (msglen && !msg)) return false;                             // handlers/nymsigner.go:78-80
    NymSignatureFields sf;
    if (!UnmarshalNymSignature(sig, siglen, sf)) return false;
    for (int k = 0; k < 4; k++)
        if (sf.len[k] != 32) return false;                                                 // (FP256BN.FromBytes reads exactly 32 bytes)
    const std::shared_ptr<const IssuerCombs> combs = issuer_combs(hsk_x32, hsk_y32, hrand_x32, hrand_y32);
    if (!combs->usable) return false;                                                      // (the device registers no such issuer)
    const KeyTab8 hsk{combs->hsk.data()}, hrand{combs->hrand.data()};
    u256 nx, ny, c, s_sk, s_rnym, tx, ty;
    from_be32(nx, nym_x32);
    from_be32(ny, nym_y32);
    from_be32(c, sf.f[0]);
    from_be32(s_sk, sf.f[1]);
    from_be32(s_rnym, sf.f[2]);
    LocalQTab<fbn> qtab;
    // t = HSk s_sk + HRand s_rnym - Nym c; anything but NYM_VALID: c >= r (never equal to a reduced value), or outside the domain the
    // provider decides (pseudonym off the curve or >= p, s-value >= r, t at infinity) - never handed out as "valid"
    if (bn_nym_commitment29(tx, ty, nx, ny, c, s_sk, s_rnym, hsk, hrand, qtab) != NYM_VALID) return false;
    // c' = HashModOrder("sign" || G1(t) || G1(nym) || ipk.Hash || msg)     (idemix/nymsignature.go:90-101; appendBytesG1 is ECP.ToBytes
    // uncompressed: 0x04 || x || y, appendBytesBig 32 bytes big-endian - idemix/util.go:57-61, 79-83)
    std::vector<uint8_t> data(4 + 65 + 65 + 32 + msglen);
    uint8_t* p = data.data();
    memcpy(p, "sign", 4);
    p[4] = 0x04;
    to_be32(p + 5, tx);
    to_be32(p + 37, ty);
    p[69] = 0x04;
    memcpy(p + 70, nym_x32, 32);            // (both below p: the big-endian bytes of the reduced coordinates are the caller's)
    memcpy(p + 102, nym_y32, 32);
    memcpy(p + 134, ipk_hash32, 32);
    if (msglen) memcpy(p + 166, msg, msglen);
    u256 c1, c2;
    hash_mod_order(c1, data.data(), data.size());
    // accept iff ProofC == HashModOrder(c' || Nonce)                       (idemix/nymsignature.go:102-104)
    uint8_t two[64];
    to_be32(two, c1);
    memcpy(two + 32, sf.f[3], 32);
    hash_mod_order(c2, two, 64);
    uint8_t c2b[32];
    to_be32(c2b, c2);
    return memcmp(c2b, sf.f[0], 32) == 0;
}

}  // namespace bccsp
}  // namespace fab
