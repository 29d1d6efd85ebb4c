// CPU audit of what the provider hands out from the device (DESIGN.md 4.4e addendum): SHA-256, one ECDSA P-256 verification and one
// idemix pseudonym-signature verification on the calling thread, and the rule that decides which hits are audited.  Host code only;
// no device, no libcrypto.
//
// The verifications are the one-lane code the kernels are compiled from (fe29.h / ec29.h / modinv30.h / p256_verify29.h; bn29.h /
// bn_nym29.h for FP256BN), compiled for the host, behind the host gates of bccsp_host.cpp (DER unmarshal, r, s > 0, low-S, key on the
// curve, hashToInt) and idemix_host.cpp (NymSignature unmarshal, 32-byte fields); SHA-256 is plain C++ (the device's uses GCN builtins).  So the audit catches wrong memory, a stale table, a race between passes, a kernel that was miscompiled
// or mis-scheduled, a hardware fault - and it does NOT catch an arithmetic mistake in the shared source: both compilations would
// make it.  That is what the oracle parity tests are for.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>

namespace fab {
namespace bccsp {

void audit_sha256(const uint8_t* msg, size_t len, uint8_t* out32);
// SHA3-256 through the kernels' own header (sha3_256.h) compiled for the host
void audit_sha3_256(const uint8_t* msg, size_t len, uint8_t* out32);
// bccsp.Verify(k, sig, digest) as bccsp/sw decides it (bccsp/sw/impl.go:247-270 -> ecdsa.go:41-57): true = (true, nil), false =
// everything else - a signature that does not unmarshal, r or s <= 0, high S, r >= n, a key that is not on the curve, an empty
// signature or digest, a signature that does not verify.
// the same for a P-384 key (48-byte coordinates): the gates against P-384's order, the arithmetic by the host compilation of p384.h
bool audit_p384_verify(const uint8_t* qx48, const uint8_t* qy48, const uint8_t* sig_der, size_t siglen, const uint8_t* digest, size_t dlen);
bool audit_p256_verify(const uint8_t* qx32, const uint8_t* qy32, const uint8_t* sig_der, size_t siglen, const uint8_t* digest, size_t dlen);

// NymVerifier.Verify(k, sig, msg, opts) as bccsp/idemix decides it (bccsp/idemix/handlers/nymsigner.go:62-95 -> idemix/nymsignature.go:
// 74-109): true = nil, false = everything else.  The issuer fields are the 32-byte halves IdemixIssuerPublicKey holds; sig is the
// marshalled idemix.NymSignature; msg is the message itself (idemix signs the message, not a digest).  Behind the gates of
// IdemixCSP::NymVerifyBatch: a signature that does not unmarshal, a field that is not 32 bytes, anything the one-lane commitment
// (bn_nym29.h bn_nym_commitment29 compiled for the host) leaves to bccsp/idemix - a pseudonym off the curve or >= p, an s-value >= r,
// t at infinity - is false: the provider never hands such a tuple out as "valid".  The 8-bit combs of HSk and HRand (640 KiB each)
// are built at an issuer's first audit and kept for the last few issuers.
bool audit_nym_verify(const uint8_t* hsk_x32, const uint8_t* hsk_y32, const uint8_t* hrand_x32, const uint8_t* hrand_y32, const uint8_t* ipk_hash32,
                      const uint8_t* nym_x32, const uint8_t* nym_y32, const uint8_t* sig, size_t siglen, const uint8_t* msg, size_t msglen);

// Which hits are audited: no randomness.  Hit number h (1-based) is audited iff h * permille / 1000 != (h - 1) * permille / 1000:
// 1000 every hit, 250 exactly every fourth (h = 4, 8, ..), 0 none; over H hits exactly H * permille / 1000 audits.
inline bool audit_sampled(uint64_t h, uint32_t permille) { return h * permille / 1000 != (h - 1) * permille / 1000; }
struct AuditSampler {
    std::atomic<uint64_t> hits{0};
    bool hit(uint32_t permille) {
        if (!permille) return false;                        // (the default: hits are not even counted)
        return audit_sampled(hits.fetch_add(1, std::memory_order_relaxed) + 1, permille);
    }
};

}  // namespace bccsp
}  // namespace fab
