// Host side of the provider: the gates bccsp/sw applies BEFORE any curve arithmetic, the error
// vocabulary of the reference, and the block-level batch verifier that feeds the GPU.
//
// Mirrors (same names / argument meaning / error text):
//   bccsp/utils/ecdsa.go:43-67   UnmarshalECDSASignature      -> fab::bccsp::UnmarshalECDSASignature
//   bccsp/utils/ecdsa.go:84-92   IsLowS                       -> fab::bccsp::IsLowS
//   bccsp/sw/ecdsa.go:41-57      verifyECDSA                  -> GPUCSP::Verify / VerifyBatch
//   bccsp/sw/impl.go:247-270     CSP.Verify argument checks   -> GPUCSP::Verify
//   bccsp/sw/impl.go:177-194     CSP.Hash                     -> GPUCSP::Hash
//   bccsp/sw/keyimport.go:103-134 public-key import           -> GPUCSP::KeyImport (on-curve gate)
//   msp/identities.go:169-196    identity.Verify              -> GPUCSP::IdentityVerifyBatch
// There is no CPU implementation of the curve arithmetic or of SHA-256 in here: every verdict comes
// from the HIP kernels through the C ABI; without a device fabgpu_init fails and so does this layer.
// (audit_host.cpp re-computes a sampled share of those verdicts and digests on the CPU before they are handed out - it can only
// ever turn an answer into a miss or poison the provider, never supply a verdict of its own.)
#include <random>

#include "bccsp_host.h"
#include "worker_pool.h"
#include "idemix_host.h"
#include "block_walk_dev.h"
#include "walk_layout.h"
#include "pass_route.h"

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <exception>
#include <functional>
#include <thread>

#include "p256_point.h"
#include "p384.h"

namespace fab {
namespace bccsp {

// ------------------------------------------------------------------------------------------------
// encoding/asn1 (Go) strictness for SEQUENCE { INTEGER r, INTEGER s }
// ------------------------------------------------------------------------------------------------
namespace {

struct TL {
    size_t len = 0;
    const char* err = nullptr;
};

// Go asn1.go parseTagAndLength + the tag comparison of parseField, for a single expected identifier octet.
TL parse_tl(const uint8_t* b, size_t n, size_t& off, uint8_t want) {
    TL r;
    uint8_t id = b[off++];
    if ((id & 0x1F) == 0x1F) {
        // base-128 tag number: whatever it decodes to it is neither SEQUENCE(16) nor INTEGER(2) in minimal form
        r.err = "asn1: structure error: tags don't match";
        // Go may report a syntax error first (truncated / non-minimal tag); all are unmarshalling failures
        return r;
    }
    if (off >= n) { r.err = "asn1: syntax error: truncated tag or length"; return r; }
    uint8_t l0 = b[off++];
    if (!(l0 & 0x80)) {
        r.len = l0;
    } else {
        int nb = l0 & 0x7F;
        if (nb == 0) { r.err = "asn1: syntax error: indefinite length found (not DER)"; return r; }
        size_t L = 0;
        for (int i = 0; i < nb; i++) {
            if (off >= n) { r.err = "asn1: syntax error: truncated tag or length"; return r; }
            if (L >= ((size_t)1 << 23)) { r.err = "asn1: structure error: length too large"; return r; }
            L = (L << 8) | b[off++];
            if (L == 0) { r.err = "asn1: structure error: superfluous leading zeros in length"; return r; }
        }
        if (L < 0x80) { r.err = "asn1: structure error: non-minimal length"; return r; }
        r.len = L;
    }
    if (id != want) { r.err = "asn1: structure error: tags don't match"; return r; }
    if (r.len > n - off) { r.err = "asn1: syntax error: data truncated"; return r; }
    return r;
}

const char* parse_bigint(const uint8_t* b, size_t n, size_t& off, BigInt& out) {
    if (off == n) return "asn1: syntax error: sequence truncated";
    TL tl = parse_tl(b, n, off, 0x02);
    if (tl.err) return tl.err;
    const uint8_t* p = b + off;
    size_t L = tl.len;
    off += L;
    if (L == 0) return "asn1: structure error: empty integer";
    if (L > 1 && ((p[0] == 0x00 && !(p[1] & 0x80)) || (p[0] == 0xFF && (p[1] & 0x80))))
        return "asn1: structure error: integer not minimally-encoded";
    out.negative = (p[0] & 0x80) != 0;
    out.twos.assign(p, p + L);
    return nullptr;
}

}  // namespace

bool BigInt::is_zero() const {
    for (uint8_t c : twos) if (c) return false;
    return true;
}
int BigInt::sign() const { return negative ? -1 : (is_zero() ? 0 : 1); }
// magnitude bytes (big-endian, no leading zeros) of a non-negative value
std::vector<uint8_t> BigInt::magnitude() const {
    std::vector<uint8_t> m;
    if (!negative) {
        size_t i = 0;
        while (i < twos.size() && twos[i] == 0) i++;
        m.assign(twos.begin() + i, twos.end());
    } else {  // two's complement negate
        m = twos;
        for (auto& c : m) c = (uint8_t)~c;
        for (size_t i = m.size(); i-- > 0;) { if (++m[i] != 0) break; }
        size_t i = 0;
        while (i < m.size() && m[i] == 0) i++;
        m.erase(m.begin(), m.begin() + i);
    }
    return m;
}
std::string BigInt::decimal() const {  // big.Int %s
    std::vector<uint8_t> m = magnitude();
    if (m.empty()) return "0";
    std::string digits;
    while (!m.empty()) {
        uint32_t rem = 0;
        std::vector<uint8_t> q;
        q.reserve(m.size());
        for (uint8_t c : m) {
            uint32_t cur = (rem << 8) | c;
            uint8_t d = (uint8_t)(cur / 10);
            rem = cur % 10;
            if (!q.empty() || d) q.push_back(d);
        }
        digits.push_back((char)('0' + rem));
        m.swap(q);
    }
    if (negative) digits.push_back('-');
    std::reverse(digits.begin(), digits.end());
    return digits;
}
bool BigInt::fits256() const { return !negative && magnitude().size() <= 32; }
void BigInt::to_be32(uint8_t* out) const {  // low 256 bits of the magnitude
    std::vector<uint8_t> m = magnitude();
    memset(out, 0, 32);
    size_t k = std::min<size_t>(32, m.size());
    memcpy(out + 32 - k, m.data() + (m.size() - k), k);
}

// bccsp/utils/ecdsa.go:43-67
Error UnmarshalECDSASignature(const uint8_t* raw, size_t len, BigInt& R, BigInt& S) {
    const char* aerr = nullptr;
    do {
        if (len == 0) { aerr = "asn1: syntax error: sequence truncated"; break; }
        size_t off = 0;
        TL tl = parse_tl(raw, len, off, 0x30);
        if (tl.err) { aerr = tl.err; break; }
        const uint8_t* in = raw + off;   // bytes after the SEQUENCE are `rest`: discarded (ecdsa.go:46)
        size_t ioff = 0;
        if ((aerr = parse_bigint(in, tl.len, ioff, R))) break;
        if ((aerr = parse_bigint(in, tl.len, ioff, S))) break;
        // trailing content inside the SEQUENCE is allowed by Go's struct parser
    } while (0);
    if (aerr) return Error(std::string("failed unmashalling signature [") + aerr + "]");
    if (R.sign() != 1) return Error("invalid signature, R must be larger than zero");
    if (S.sign() != 1) return Error("invalid signature, S must be larger than zero");
    return Error();
}

static const uint8_t HALF_N_BE[32] = {0x7f, 0xff, 0xff, 0xff, 0x80, 0x00, 0x00, 0x00, 0x7f, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff,
                                      0xde, 0x73, 0x7d, 0x56, 0xd3, 0x8b, 0xcf, 0x42, 0x79, 0xdc, 0xe5, 0x61, 0x7e, 0x31, 0x92, 0xa8};
const char* HALF_ORDER_DECIMAL = "57896044605178124381348723474703786764998477612067880171211129530534256022184";

// bccsp/utils/ecdsa.go:84-92: s.Cmp(halfOrder) != 1
bool IsLowS(const BigInt& S) {
    if (S.negative) return true;
    if (!S.fits256()) return false;
    uint8_t s32[32];
    S.to_be32(s32);
    return memcmp(s32, HALF_N_BE, 32) <= 0;
}

bool PublicKeyOnCurve(const uint8_t* qx32, const uint8_t* qy32) {
    const u256 P = FAB_P256_P;
    u256 x, y, mx, my;
    from_be32(x, qx32);
    from_be32(y, qy32);
    if (!lt256(x, P) || !lt256(y, P)) return false;
    fp_to_mont(mx, x);
    fp_to_mont(my, y);
    return on_curve_mont(mx, my);
}

void HashToInt(const uint8_t* digest, size_t len, uint8_t* e32) {
    if (len > 32) len = 32;
    memset(e32, 0, 32);
    memcpy(e32 + 32 - len, digest, len);
}

// ------------------------------------------------------------------------------------------------
// GPUCSP
// ------------------------------------------------------------------------------------------------
Error GPUCSP::New(const fabgpu_cfg* cfg, std::unique_ptr<GPUCSP>& out) {
    std::unique_ptr<GPUCSP> p(new GPUCSP());
    fabgpu_ctx* ctx = nullptr;
    int rc = fabgpu_init(cfg, &ctx);
    if (rc != FABGPU_OK) return Error(std::string("Failed initializing GPU BCCSP: ") + fabgpu_strerror(rc));
    std::unique_ptr<Dev> d(new Dev);
    d->ctx = ctx;
    d->ordinal = cfg ? cfg->device : -1;
    p->devs_.push_back(std::move(d));
    p->opts_.ctx_flags = cfg ? cfg->flags : 0;
    p->opts_.p384_wide = (p->opts_.ctx_flags & FABGPU_FLAG_P384_WIDE) ? 1 : 0;
    p->opts_.p384_key_tables16 = (p->opts_.ctx_flags & FABGPU_FLAG_P384_KEY_TABLES_16BIT) ? 1 : 0;
    p->opts_.sha3_coop = (p->opts_.ctx_flags & FABGPU_FLAG_SHA3_COOP) ? 1 : 0;
    out = std::move(p);
    return Error();
}
// One provider, G device contexts: what bccsp/factory hands to every channel of the peer (bccsp/factory/factory.go:41-55).
Error GPUCSP::New(const ProviderOptions& opts, std::unique_ptr<GPUCSP>& out) {
    std::vector<int32_t> devices = opts.devices;
    if (devices.empty()) {
        const int n = fabgpu_device_count(nullptr);
        if (n <= 0) return Error(std::string("Failed initializing GPU BCCSP: ") + fabgpu_strerror(FABGPU_ENODEV));
        for (int i = 0; i < n; i++) devices.push_back(i);
    }
    if ((int)devices.size() > kMaxProviderDevices) return Error("Failed initializing GPU BCCSP: more device contexts than the provider takes");
    std::unique_ptr<GPUCSP> p(new GPUCSP());
    p->opts_ = opts;
    p->retire_evicted_.store(opts.retire_evicted_keys > 0, std::memory_order_relaxed);
    p->hash_sha3_.store(opts.hash_sha3 > 0, std::memory_order_relaxed);
    p->p384_.store(opts.p384 > 0, std::memory_order_relaxed);
    p->opts_.devices = devices;
    if (opts.p384_wide > 0) p->opts_.ctx_flags |= FABGPU_FLAG_P384_WIDE;             // (the option is the flag, on every context)
    p->opts_.p384_wide = (p->opts_.ctx_flags & FABGPU_FLAG_P384_WIDE) ? 1 : 0;
    if (opts.p384_key_tables16 > 0) p->opts_.ctx_flags |= FABGPU_FLAG_P384_KEY_TABLES_16BIT;
    p->opts_.p384_key_tables16 = (p->opts_.ctx_flags & FABGPU_FLAG_P384_KEY_TABLES_16BIT) ? 1 : 0;
    if (opts.sha3_coop > 0) p->opts_.ctx_flags |= FABGPU_FLAG_SHA3_COOP;
    p->opts_.sha3_coop = (p->opts_.ctx_flags & FABGPU_FLAG_SHA3_COOP) ? 1 : 0;
    p->audit_permille_.store(opts.audit_permille > 1000 ? 1000 : opts.audit_permille, std::memory_order_relaxed);
    for (int32_t ord : devices) {
        fabgpu_cfg cfg;
        memset(&cfg, 0, sizeof(cfg));
        cfg.device = ord;
        cfg.flags = p->opts_.ctx_flags;
        fabgpu_ctx* ctx = nullptr;
        const int rc = fabgpu_init(&cfg, &ctx);
        if (rc != FABGPU_OK)                                    // (~GPUCSP shuts the contexts made so far down)
            return Error("Failed initializing GPU BCCSP on device " + std::to_string(ord) + ": " + fabgpu_strerror(rc));
        std::unique_ptr<Dev> d(new Dev);
        d->ctx = ctx;
        d->ordinal = ord;
        p->devs_.push_back(std::move(d));
    }
    p->Preallocate();
    out = std::move(p);
    return Error();
}
GPUCSP::~GPUCSP() {
    memo_blocks_.clear();                                   // (tables the device built live in pinned memory of a context)
    memo_free_.clear();
    for (auto& d : devs_) fabgpu_shutdown(d->ctx);
}
GPUCSP::BlockUpload::~BlockUpload() {
    if (th.joinable()) th.join();
    host_copy_release(&copy);                               // (a pass that published a memo table took it along: nothing left to release)
    if (routed && owner) owner->devs_[(size_t)dev]->in_flight.fetch_sub(1, std::memory_order_acq_rel);
}
int GPUCSP::Sha3CoopRows(uint64_t* rows) const {
    *rows = 0;
    for (auto& d : devs_) {
        uint64_t v = 0;
        if (int rc = fabgpu_sha3_coop_rows(d->ctx, &v)) return rc;
        *rows += v;
    }
    return FABGPU_OK;
}
int GPUCSP::RouteBlock(uint64_t block_seq) const {
    const int G = (int)devs_.size();
    if (G <= 1) return 0;
    uint32_t fl[kMaxProviderDevices];
    for (int g = 0; g < G; g++) fl[g] = devs_[(size_t)g]->in_flight.load(std::memory_order_acquire);
    return route_block(block_seq, fl, G);
}
void GPUCSP::PassesPerDevice(uint64_t* passes) const {
    for (size_t g = 0; g < devs_.size(); g++) passes[g] = devs_[g]->passes.load(std::memory_order_relaxed);
}
// The switches of one provider (they used to be environment variables read inside the pass: VERDICT r3 weak 13).
namespace {
struct OptField {
    const char* name;
    int ProviderOptions::*f;
};
const OptField kIntOpts[] = {{"pass_device_walk", &ProviderOptions::pass_device_walk},
                             {"pass_device_memo", &ProviderOptions::pass_device_memo},
                             {"pass_host_counts", &ProviderOptions::pass_host_counts},
                             {"pass_skip_hash_checks", &ProviderOptions::pass_skip_hash_checks},
                             {"pass_timing", &ProviderOptions::pass_timing},
                             {"pass_hash_memo", &ProviderOptions::pass_hash_memo},
                             {"retire_evicted_keys", &ProviderOptions::retire_evicted_keys},
                             {"hash_sha3", &ProviderOptions::hash_sha3},
                             {"p384", &ProviderOptions::p384}};
}  // namespace
int64_t GPUCSP::SetOption(const std::string& name, int64_t value) const {
    std::lock_guard<std::mutex> lk(opt_mu_);
    if (name == "pass_stage_min_bytes") {
        const int64_t prev = opts_.pass_stage_min_bytes;
        opts_.pass_stage_min_bytes = value;
        return prev;
    }
    if (name == "audit_permille") {                              // (0 .. 1000; anything else is refused like an unknown name)
        if (value < 0 || value > 1000) return INT64_MIN;
        opts_.audit_permille = (uint32_t)value;
        return (int64_t)audit_permille_.exchange((uint32_t)value, std::memory_order_relaxed);
    }
    if (name == "p384_wide") {                                   // (a context flag: the living contexts are switched, all or none)
        const int64_t prev = opts_.p384_wide;
        for (auto& d : devs_)
            if (ctx_set_p384_wide(d->ctx, value > 0) != FABGPU_OK) {
                for (auto& u : devs_) (void)ctx_set_p384_wide(u->ctx, prev > 0);
                return INT64_MIN;
            }
        opts_.p384_wide = value > 0 ? 1 : 0;
        return prev;
    }
    if (name == "sha3_coop") {                                   // (a context flag, as above)
        const int64_t prev = opts_.sha3_coop;
        for (auto& d : devs_)
            if (ctx_set_sha3_coop(d->ctx, value > 0) != FABGPU_OK) {
                for (auto& u : devs_) (void)ctx_set_sha3_coop(u->ctx, prev > 0);
                return INT64_MIN;
            }
        opts_.sha3_coop = value > 0 ? 1 : 0;
        return prev;
    }
    for (const OptField& o : kIntOpts)
        if (name == o.name) {
            const int64_t prev = opts_.*(o.f);
            opts_.*(o.f) = (int)value;
            if (name == "retire_evicted_keys") retire_evicted_.store(value > 0, std::memory_order_relaxed);
            if (name == "hash_sha3") hash_sha3_.store(value > 0, std::memory_order_relaxed);
            if (name == "p384") p384_.store(value > 0, std::memory_order_relaxed);
            return prev;
        }
    return INT64_MIN;
}
int64_t GPUCSP::GetOption(const std::string& name) const {
    std::lock_guard<std::mutex> lk(opt_mu_);
    if (name == "pass_stage_min_bytes") return opts_.pass_stage_min_bytes;
    if (name == "n_devices") return (int64_t)devs_.size();
    if (name == "audit_permille") return (int64_t)AuditPermille();
    if (name == "p384_wide") return opts_.p384_wide;
    if (name == "sha3_coop") return opts_.sha3_coop;
    if (name == "p384_key_tables16") return opts_.p384_key_tables16;       // (read at construction: SetOption does not know the name)
    if (name == "registrations_dropped") return (int64_t)reg_dropped_.load(std::memory_order_relaxed);        // (read-only counters)
    if (name == "registration_id_mismatches") return (int64_t)reg_id_mismatches_.load(std::memory_order_relaxed);
    for (const OptField& o : kIntOpts)
        if (name == o.name) return opts_.*(o.f);
    return INT64_MIN;
}
// A key's comb table on every device: built once on the host, uploaded G times.  Registrations take turns (reg_mu_), so a key that
// only ever enters through the provider gets the same id on every device; a caller that registered keys on one of the provider's
// contexts behind its back makes the ids differ - then the key simply has no table here (-1) and verifies on the fresh-key kernels.
int64_t GPUCSP::RegisterKeyOnAllDevices(const uint8_t* qx32, const uint8_t* qy32, const int32_t* prebuilt_table) const {
    std::lock_guard<std::mutex> lk(reg_mu_);
    FlushRetirementsRegLocked();
    if (!HealPendingRegistrationsLocked()) return -1;       // (nothing new is installed while an earlier registration is still lopsided)
    const int G = (int)devs_.size();
    fabgpu_ctx* cs[kMaxProviderDevices];
    uint32_t ids[kMaxProviderDevices];
    for (int g = 0; g < G; g++) cs[g] = devs_[(size_t)g]->ctx;
    const int rc = key_register_many_prebuilt(cs, G, qx32, qy32, prebuilt_table, ids);
    if (rc != FABGPU_OK) {
        // did any device take it?  then the pool is lopsided until this key is on all of them
        uint32_t id0 = 0;
        bool some = false;
        for (int g = 0; g < G; g++) some = some || fabgpu_p256_key_lookup(cs[g], qx32, qy32, &id0) == FABGPU_OK;
        if (some) {
            PendingKey pk;
            memcpy(pk.qx, qx32, 32);
            memcpy(pk.qy, qy32, 32);
            pending_keys_.push_back(pk);
        }
        if (!reg_failure_logged_) {
            reg_failure_logged_ = true;
            fprintf(stderr, "fabgpu: a key table could not be installed on every device (%s)%s; the key verifies on the fresh-key kernels\n", fabgpu_strerror(rc),
                    some ? " - it will be retried before the next registration" : "");
        }
        return -1;
    }
    for (int g = 1; g < G; g++)
        if (ids[g] != ids[0]) return -1;
    return ids[0];
}
// A batch of keys on every device of the pool, tables built on the devices (key_register_batch).  true: ids[i] = the common id of key
// i, or -1 where the devices disagree (that key verifies on the fresh-key kernels).  false: some device could not - nothing is recorded as
// pending (whatever a device did install is complete and idempotent), the caller registers key by key with host-built tables instead.
bool GPUCSP::RegisterKeysOnAllDevices(const std::vector<std::pair<std::string, CachedIdentity>>& keys, std::vector<int64_t>& ids) const {
    if (keys.empty()) return true;
    std::lock_guard<std::mutex> lk(reg_mu_);
    FlushRetirementsRegLocked();
    if (!HealPendingRegistrationsLocked()) return false;
    const int G = (int)devs_.size(), n = (int)keys.size();
    std::vector<uint8_t> qxy((size_t)64 * n);
    for (int i = 0; i < n; i++) {
        memcpy(&qxy[64 * (size_t)i], keys[(size_t)i].second.qx, 32);
        memcpy(&qxy[64 * (size_t)i + 32], keys[(size_t)i].second.qy, 32);
    }
    std::vector<std::vector<uint32_t>> got((size_t)G, std::vector<uint32_t>((size_t)n, 0));
    std::vector<int> rcs((size_t)G, FABGPU_OK);
    auto one = [&](int g) { rcs[(size_t)g] = key_register_batch(devs_[(size_t)g]->ctx, n, qxy.data(), got[(size_t)g].data()); };
    if (G == 1) one(0);
    else run_workers(G, one);
    for (int g = 0; g < G; g++)
        if (rcs[(size_t)g] != FABGPU_OK) return false;
    for (int i = 0; i < n; i++) {
        bool same = true;
        for (int g = 1; g < G; g++) same = same && got[(size_t)g][(size_t)i] == got[0][(size_t)i];
        ids[(size_t)i] = same ? (int64_t)got[0][(size_t)i] : -1;
    }
    return true;
}
// Replays the registrations that reached only some devices (idempotent where the key / issuer already is).  Called with reg_mu_ held.
bool GPUCSP::HealPendingRegistrationsLocked() const {
    const int G = (int)devs_.size();
    fabgpu_ctx* cs[kMaxProviderDevices];
    uint32_t ids[kMaxProviderDevices];
    for (int g = 0; g < G; g++) cs[g] = devs_[(size_t)g]->ctx;
    // A replay that keeps failing (a device out of memory for good, its key or issuer table full) must not stop every later registration
    // for the life of the provider: after kMaxHealAttempts the entry is DROPPED and counted.  The pool's per-device ids may
    // then differ for what is registered afterwards - RegisterKeyOnAllDevices / ImportIdemixIssuer answer -1 for such a key or issuer
    // (the fresh-key kernels / bccsp/idemix serve it: slower, never wrong), they do not fail.
    constexpr uint32_t kMaxHealAttempts = 3;
    auto give_up = [&](const char* what) {
        heal_attempts_ = 0;
        reg_dropped_.fetch_add(1, std::memory_order_relaxed);
        fprintf(stderr, "fabgpu: %s could not be installed on every device after %u attempts; dropped - registrations go on, ids may differ between devices\n", what,
                kMaxHealAttempts);
    };
    while (!pending_keys_.empty()) {
        const PendingKey& pk = pending_keys_.front();
        if (key_register_many_prebuilt(cs, G, pk.qx, pk.qy, nullptr, ids) != FABGPU_OK) {
            if (++heal_attempts_ < kMaxHealAttempts) return false;
            give_up("a key table");
        } else {
            heal_attempts_ = 0;
        }
        pending_keys_.erase(pending_keys_.begin());
    }
    while (!pending_issuers_.empty()) {
        const std::string& raw = pending_issuers_.front();
        bool ok = true;
        for (int g = 0; g < G && ok; g++) {
            IdemixCSP ic(cs[g]);
            IdemixIssuerPublicKey k;
            ok = ic.IssuerKeyImport((const uint8_t*)raw.data(), raw.size(), k).ok() && k.issuer_id >= 0;
        }
        if (!ok) {
            if (++heal_attempts_ < kMaxHealAttempts) return false;
            give_up("an idemix issuer key");
        } else {
            heal_attempts_ = 0;
        }
        pending_issuers_.erase(pending_issuers_.begin());
    }
    return true;
}
// ProviderOptions::concurrent_passes: what that many overlapping passes per device need, made when the provider is made (DESIGN.md 8
// "Next" item 1) - per device the staging slots, pinned staging and pass arrays (walk_preallocate), for the
// provider one scratch set and one pinned memo table per pass in flight plus the tables that wait, seeded, for their block's validators.
void GPUCSP::Preallocate() const {
    const int G = (int)devs_.size();
    scratch_free_max_ = std::max<size_t>(4, (size_t)4 * G);
    memo_free_max_ = std::max<size_t>(4, (size_t)4 * G);
    const uint32_t P = opts_.concurrent_passes;
    const uint32_t keep_blocks = opts_.hash_memo_blocks ? std::min<uint32_t>(opts_.hash_memo_blocks, 64u) : 8u;
    const bool keep_on = opts_.pass_hash_memo >= 0;
    for (int g = 0; g < G; g++) host_copy_limit(devs_[(size_t)g]->ctx, keep_blocks);
    if (!P) return;
    const size_t block_bytes = opts_.expect_block_bytes ? opts_.expect_block_bytes : (size_t)64 << 20;
    const uint32_t n_tuples = opts_.expect_tuples ? opts_.expect_tuples : 65536u;
    const uint32_t n_tx = std::max<uint32_t>(1024, n_tuples / 3);
    std::vector<std::thread> th;                            // (the devices allocate side by side: 63 MB of device memory per slot takes milliseconds)
    for (int g = 0; g < G; g++) {
        fabgpu_ctx* c = devs_[(size_t)g]->ctx;
        th.emplace_back([c, block_bytes, n_tx, n_tuples, P, keep_on, keep_blocks] {
            (void)walk_preallocate(c, block_bytes, n_tx, n_tuples, (int)P);
            // the digest memo keeps a host copy per block until its validators are through: the passes in flight plus two waiting, pinned now
            if (keep_on) host_copy_preallocate(c, block_bytes, std::min<uint32_t>(keep_blocks, P + 2));
            // The runtime loads a translation unit's code object at the first launch of one of its kernels - 8 ms of a channel's first
            // block when the pass's first launches paid for it.  One launch per unit, now (answers unused: garbage in, statuses out).
            uint8_t msg[64] = {0x30, 0x06, 0x02, 0x01, 0x01, 0x02, 0x01, 0x01}, dig[32], f32[32] = {0}, st1 = 0, code = 0, r32[32], s32[32];
            f32[31] = 1;
            const uint32_t off[2] = {0, 55}, span[2] = {0, 8};
            uint64_t bits = 0;
            (void)fabgpu_sha256_batch(c, 1, msg, off, dig);                                  // wide_kernels.hip
            (void)fabgpu_p256_verify_batch(c, 1, f32, f32, f32, f32, f32, &bits, &st1);      // kernels.hip
            (void)walk_gate_probe(c, 1, msg, sizeof(msg), span, &code, r32, s32);            // block_walk_kernels.hip
        });
    }
    const size_t n_sets = (size_t)P * G, n_tables = n_sets + 6;   // (memo_cap_ holds about six 40 000-entry blocks waiting for their validators)
    scratch_free_max_ = std::max(scratch_free_max_, n_sets);
    memo_free_max_ = std::max(memo_free_max_, n_tables);
    {
        std::lock_guard<std::mutex> lk(pass_mu_);
        while (scratch_free_.size() < n_sets) {
            std::unique_ptr<PassScratch> ps(new PassScratch);
            ps->env_spans.reserve(2 * (size_t)n_tx);
            ps->payload_spans.reserve(2 * (size_t)n_tx);
            ps->id_idx.reserve(n_tuples);
            ps->learn.reserve(WALK_LEARN_SLOTS);
            scratch_free_.push_back(std::move(ps));
        }
    }
    {
        size_t total = 0;
        uint32_t cap = 0;
        size_t keys_cap = 0;
        MemoPinLayout(n_tuples, n_tx, &cap, &keys_cap, &total);
        std::vector<std::shared_ptr<BlockMemo>> made;
        for (size_t k = 0; k < n_tables; k++) {
            std::shared_ptr<BlockMemo> bm(new BlockMemo);
            fabgpu_ctx* c = devs_[k % (size_t)G]->ctx;
            bm->pin = walk_pinned_alloc(c, total + total / 4);
            if (!bm->pin) break;
            bm->pin_ctx = c;
            bm->pin_cap = total + total / 4;
            made.push_back(bm);
        }
        for (auto& t : th) t.join();
        th.clear();
        // The copies of a memo-seeding pass, rehearsed: device -> each table's pinned room, WHILE a block-sized upload travels the other
        // way - the situation in which the runtime was seen to create further DMA queues inside hipMemcpyAsync (10-14 ms each, three or
        // four times per provider: walk_preallocate).  Until the calls return at once, at most six rounds per device.
        if (!made.empty()) {
            std::vector<uint8_t> dummy(std::min<size_t>(block_bytes, (size_t)32 << 20), 0x5a);
            std::vector<void*> pins;
            std::vector<size_t> sizes;
            for (auto& bm : made) {
                pins.push_back(bm->pin);
                sizes.push_back(bm->pin_cap);
            }
            for (int g = 0; g < G; g++) {
                fabgpu_ctx* c = devs_[(size_t)g]->ctx;
                int calm = 0;
                for (int round = 0; round < 6 && calm < 2; round++) {
                    uint64_t tok = 0;
                    std::thread up([&] { (void)fabgpu_arena_stage(c, dummy.data(), dummy.size(), &tok); });
                    const double worst = walk_warm_copies(c, pins.data(), sizes.data(), (int)pins.size());
                    up.join();
                    if (worst < 0) break;
                    calm = worst < 1.0 ? calm + 1 : 0;
                }
            }
        }
        std::unique_lock<BigReaderLock> lk(memo_mu_);
        for (auto& bm : made) memo_free_.push_back(bm);
    }
    for (auto& t : th) t.join();
}
// where the arrays of a device-built memo table lie in its pinned room (one layout for the pass and for the pre-allocation)
size_t GPUCSP::MemoPinLayout(uint32_t n_tuples, uint32_t n_creators, uint32_t* slot_cap, size_t* keys_cap, size_t* total, size_t* offs7) {
    // a slot table of at least twice the tuples, offsets, statuses, digests, and keys of 109 (141 for a pseudonym signature) +
    // signature bytes each - 96 bytes of signature on average are allowed for (an ECDSA signature has <= 72; a block whose keys do
    // not fit gets more room at the end of the pass: WalkRequest::memo_grow)
    const uint32_t cap = walk_memo_slot_cap(n_tuples);              // (walk_layout.h: the pass's worst case is sized with the same table)
    const size_t kc = (size_t)n_tuples * (109 + 96) + (size_t)n_creators * 32 + 256;
    auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t a_slots = 0, a_off = up256((size_t)cap * 4), a_st = a_off + up256(((size_t)n_tuples + 1) * 4), a_dig = a_st + up256(n_tuples),
                 a_hslots = a_dig + up256((size_t)n_tuples * 32),      // the digest memo's index: a second slot table, four span words per entry
                 a_hspans = a_hslots + up256((size_t)cap * 4), a_keys = a_hspans + up256((size_t)n_tuples * 16);
    if (slot_cap) *slot_cap = cap;
    if (keys_cap) *keys_cap = kc;
    if (total) *total = a_keys + up256(kc);
    if (offs7) {
        offs7[0] = a_slots; offs7[1] = a_off; offs7[2] = a_st; offs7[3] = a_dig; offs7[4] = a_keys; offs7[5] = a_hslots; offs7[6] = a_hspans;
    }
    return a_keys + up256(kc);
}
int64_t GPUCSP::ImportIdemixIssuer(const uint8_t* ipk_raw, size_t len, std::string* err) const {
    std::lock_guard<std::mutex> lk(reg_mu_);
    if (!HealPendingRegistrationsLocked()) {
        if (err) *err = "an earlier registration has not reached every device yet";
        return -1;
    }
    int64_t id = -1;
    for (size_t g = 0; g < devs_.size(); g++) {
        IdemixCSP ic(devs_[g]->ctx);
        IdemixIssuerPublicKey k;
        Error e = ic.IssuerKeyImport(ipk_raw, len, k);
        const bool took = e.ok() && k.issuer_id >= 0;
        if (!took) {
            if (err) *err = e.ok() ? "a device did not take the issuer key" : e.msg;
            // (devices before g have it: replayed before the next registration, so that the per-device issuer ids stay aligned)
            if (g > 0 && e.ok()) pending_issuers_.emplace_back((const char*)ipk_raw, len);
            return -1;
        }
        if (g == 0) {
            id = k.issuer_id;
            AuditIssuer a;                                     // the pseudonym audit verifies under the same fields, on the host
            memcpy(a.data(), k.hsk_x, 32);
            memcpy(a.data() + 32, k.hsk_y, 32);
            memcpy(a.data() + 64, k.hrand_x, 32);
            memcpy(a.data() + 96, k.hrand_y, 32);
            memcpy(a.data() + 128, k.hash, 32);
            std::lock_guard<std::mutex> alk(audit_issuer_mu_);
            audit_issuers_[id] = a;
        } else if (k.issuer_id != id) {
            // ids are handed out in order per context: once they differ they differ for every later issuer too.  Nothing to replay -
            // every device HAS the key - but it is counted and said once, and the issuer is not accelerated (bccsp/idemix serves it).
            reg_id_mismatches_.fetch_add(1, std::memory_order_relaxed);
            if (!issuer_mismatch_logged_) {
                issuer_mismatch_logged_ = true;
                fprintf(stderr, "fabgpu: the devices of the pool gave an idemix issuer different ids (%lld on device 0, %lld on device %zu): not accelerated\n", (long long)id,
                        (long long)k.issuer_id, g);
            }
            if (err) *err = "the devices of the pool disagree about the issuer's id";
            return -1;
        }
    }
    return id;
}
GPUCSP::BlockMemo::~BlockMemo() {
    host_copy_release(&copy);
    if (pin) walk_pinned_free(pin_ctx, pin);
    if (pin_keys) walk_pinned_free(pin_ctx, pin_keys);
}

// bccsp/sw/keyimport.go:103-112 (ECDSAGoPublicKeyImportOpts) with the curve check x509 parsing implies
Error GPUCSP::KeyImport(const uint8_t* qx32, const uint8_t* qy32, ECDSAPublicKey& out, bool device_table) const {
    if (!qx32 || !qy32) return Error("Invalid raw. It must not be nil.");
    memcpy(out.x, qx32, 32);
    memcpy(out.y, qy32, 32);
    out.on_curve = PublicKeyOnCurve(qx32, qy32);
    // a long-lived identity's key gets its comb table on the device (best effort: on failure the fresh-key kernels serve it)
    if (out.on_curve && device_table) {
        {
            std::string k((const char*)qx32, 32);
            k.append((const char*)qy32, 32);
            std::lock_guard<std::mutex> lk(retire_mu_);
            imported_keys_.insert(std::move(k));            // (an imported key's table is the caller's: no eviction retires it)
        }
        (void)RegisterKeyOnAllDevices(qx32, qy32);
    }
    return Error();
}

// bccsp/sw/impl.go:177-194
Error GPUCSP::Hash(const uint8_t* msg, size_t len, const HashOpts* opts, std::vector<uint8_t>& digest) const {
    if (opts == nullptr) return Error("Invalid opts. It must not be nil.");
    const bool sha3 = opts->algorithm == "SHA3_256" && Sha3Enabled();       // (bccsp/sw/new.go:77: SHA3_256Opts -> sha3.New256)
    if (opts->algorithm != "SHA256" && !sha3) return Error("Unsupported 'HashOpt' provided [" + opts->algorithm + "]");
    uint32_t off[2] = {0, (uint32_t)len};
    digest.assign(32, 0);
    int rc = sha3 ? fabgpu_sha3_256_batch(flat_ctx(), 1, msg, off, digest.data()) : fabgpu_sha256_batch(flat_ctx(), 1, msg, off, digest.data());
    if (rc != FABGPU_OK) return Error("Failed hashing with opts [" + opts->algorithm + "]: " + fabgpu_strerror(rc));
    return Error();
}
// msp/identities.go:216-224 getHashOpt
bool GPUCSP::HashFamily(const char* family, bool* sha3, std::string* err) const {
    return ParseHashFamily(family, Sha3Enabled(), sha3, err);                // (msp_family.h: the texts live there)
}
// the family the pass hashes an MSP's P-384 tuples with (msp_family.h)
bool GPUCSP::SetMspHashFamily(const std::string& mspid, const char* family, std::string* err) const {
    bool sha3 = false;
    if (!HashFamily(family, &sha3, err)) return false;
    if (!msp_family_.Set(mspid, sha3)) {
        if (err) *err = "invalid mspid";
        return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------
// the direct-call verbs: one body each over a curve description (bccsp_host.h Curve256 / Curve384)
// ------------------------------------------------------------------------------------------------
bool Curve256::low_s(const uint8_t* s32) { return memcmp(s32, HALF_N_BE, 32) <= 0; }
void Curve256::generator(uint8_t* qx32, uint8_t* qy32) {
    static const uint8_t GX[32] = {0x6b, 0x17, 0xd1, 0xf2, 0xe1, 0x2c, 0x42, 0x47, 0xf8, 0xbc, 0xe6, 0xe5, 0x63, 0xa4, 0x40, 0xf2,
                                   0x77, 0x03, 0x7d, 0x81, 0x2d, 0xeb, 0x33, 0xa0, 0xf4, 0xa1, 0x39, 0x45, 0xd8, 0x98, 0xc2, 0x96};
    static const uint8_t GY[32] = {0x4f, 0xe3, 0x42, 0xe2, 0xfe, 0x1a, 0x7f, 0x9b, 0x8e, 0xe7, 0xeb, 0x4a, 0x7c, 0x0f, 0x9e, 0x16,
                                   0x2b, 0xce, 0x33, 0x57, 0x6b, 0x31, 0x5e, 0xce, 0xcb, 0xb6, 0x40, 0x68, 0x37, 0xbf, 0x51, 0xf5};
    memcpy(qx32, GX, 32);
    memcpy(qy32, GY, 32);
}
const char* Curve384::half_order_decimal() {
    return "19701003098197239606139520050071806902539869635232723333973452639813829699556631784699478154076147456777216826971321";
}
bool Curve384::low_s(const uint8_t* s48) { return p384::is_low_s(s48); }
void Curve384::hash_to_int(const uint8_t* digest, size_t len, uint8_t* e48) { p384::hash_to_int(digest, len, e48); }
void Curve384::generator(uint8_t* qx48, uint8_t* qy48) {
    p384::u384 gx = FAB_P384_GX_MONT, gy = FAB_P384_GY_MONT, t;
    p384::fp_from_mont(t, gx); p384::to_be48(qx48, t);
    p384::fp_from_mont(t, gy); p384::to_be48(qy48, t);
}

namespace {
// outcome of the pre-arithmetic gates for one item; `submit` means the device decides
template <class C>
struct GateT {
    bool submit = false;
    VerifyResult res;
    uint8_t r[C::W], s[C::W], e[C::W];
};

// the low `w` bytes of a non-negative value; false: it has more
bool low_bytes(const BigInt& v, uint8_t* out, size_t w) {
    const std::vector<uint8_t> m = v.magnitude();
    memset(out, 0, w);
    const size_t take = m.size() < w ? m.size() : w;
    if (take) memcpy(out + w - take, m.data() + m.size() - take, take);
    return m.size() <= w;
}

// The checks bccsp/sw makes before any arithmetic, in its order and with its texts, for a key of either curve: low S against the
// half order of the key's own curve (bccsp/utils/ecdsa.go:84-92), r above 2^(8 W) > n: (false, nil).  A row that is not submitted
// keeps r = s = 1, e = 0.
template <class C>
GateT<C> gate_item(const typename C::Key* k, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen) {
    constexpr size_t W = C::W;
    GateT<C> g;
    memset(g.r, 0, W); memset(g.s, 0, W); memset(g.e, 0, W);
    g.r[W - 1] = g.s[W - 1] = 1;
    // bccsp/sw/impl.go:249-257
    if (k == nullptr) { g.res = {false, Error("Invalid Key. It must not be nil.")}; return g; }
    if (siglen == 0) { g.res = {false, Error("Invalid signature. Cannot be empty.")}; return g; }
    if (dlen == 0) { g.res = {false, Error("Invalid digest. Cannot be empty.")}; return g; }
    // Fast path for the overwhelmingly common shape - a minimal DER SEQUENCE { INTEGER r, INTEGER s } with positive r, s below
    // 2^256 and low s - which the general parser below would accept with exactly these values; anything else (long-form
    // lengths, trailing bytes, negative or zero integers, high s, oversize r ...) takes the general path and its error texts.
    // P-256 only: a P-384 signature of this shape is past 127 bytes half the time and then has a long-form length.
    if constexpr (C::kDerFastPath) {
        static_assert(W == 32, "the lengths below are those of 256-bit integers");
        if (k->on_curve && siglen >= 8 && siglen <= 72 && sig[0] == 0x30 && sig[1] == siglen - 2 && sig[2] == 0x02) {
            size_t lr = sig[3];
            if (lr >= 1 && lr <= 33 && 4 + lr + 2 <= siglen && sig[4 + lr] == 0x02) {
                size_t ls = sig[5 + lr];
                const uint8_t* pr = sig + 4;
                const uint8_t* ps = sig + 6 + lr;
                auto minimal_positive = [](const uint8_t* p, size_t l) {
                    if (p[0] & 0x80) return false;                                  // negative
                    if (p[0] == 0) return l > 1 && (p[1] & 0x80) != 0 && l <= 33;   // a leading zero must be needed (also excludes zero)
                    return l <= 32;
                };
                if (ls >= 1 && ls <= 33 && 6 + lr + ls == siglen && minimal_positive(pr, lr) && minimal_positive(ps, ls)) {
                    if (pr[0] == 0) { pr++; lr--; }
                    if (ps[0] == 0) { ps++; ls--; }
                    memset(g.r, 0, 32); memset(g.s, 0, 32);
                    memcpy(g.r + 32 - lr, pr, lr);
                    memcpy(g.s + 32 - ls, ps, ls);
                    if (C::low_s(g.s)) {                                            // low-S: the device decides (r >= n included)
                        C::hash_to_int(digest, dlen, g.e);
                        g.submit = true;
                        return g;
                    }
                    memset(g.r, 0, 32); memset(g.s, 0, 32);
                    g.r[31] = g.s[31] = 1;
                }
            }
        }
    }
    const std::string wrap = "Failed verifing with opts [<nil>]: ";   // errors.Wrapf at impl.go:266
    BigInt R, S;
    Error e = UnmarshalECDSASignature(sig, siglen, R, S);
    if (!e.ok()) { g.res = {false, Error(wrap + "Failed unmashalling signature [" + e.msg + "]")}; return g; }
    uint8_t r_be[W], s_be[W];                                          // (R and S are positive here)
    const bool s_fits = low_bytes(S, s_be, W), r_fits = low_bytes(R, r_be, W);
    if (!s_fits || !C::low_s(s_be)) {
        g.res = {false, Error(wrap + "Invalid S. Must be smaller than half the order [" + S.decimal() + "][" + C::half_order_decimal() + "].")};
        return g;
    }
    if (!r_fits) { g.res = {false, Error()}; return g; }               // r >= 2^(8 W) > n: ecdsa.Verify returns false
    if (!k->on_curve) {
        g.res = {false, Error(std::string("public key is not on ") + C::kName + ": the GPU provider does not decide this tuple (use bccsp/sw)")};
        g.res.needs_sw = true;
        return g;
    }
    memcpy(g.r, r_be, W);
    memcpy(g.s, s_be, W);
    C::hash_to_int(digest, dlen, g.e);
    g.submit = true;
    return g;
}

// what the block pass writes for a tuple the gate did not submit (both routes' P-256 tuples and the P-384 stage)
uint8_t gate_tuple_status(const VerifyResult& res) {
    if (res.err.ok()) return FABGPU_ST_RANGE;                                            // r does not fit the field: (false, nil)
    if (res.err.msg.find("Invalid S") != std::string::npos) return FABGPU_ST_HIGH_S;
    return TUPLE_ST_BAD_DER;
}

// key ids of the submitted items on `ctx` if EVERY submitted item's key is registered there (then the keyed entries apply)
template <class C>
bool all_registered(fabgpu_ctx* ctx, size_t n, const std::vector<uint8_t>& submitted, const uint8_t* qx, const uint8_t* qy, std::vector<uint32_t>& ids) {
    ids.assign(n, 0);
    uint32_t any = 0;
    bool have = false;
    for (size_t i = 0; i < n; i++) {
        if (!submitted[i]) continue;
        if (C::lookup(ctx, qx + C::W * i, qy + C::W * i, &ids[i]) != FABGPU_OK) return false;
        any = ids[i];
        have = true;
    }
    if (!have) return false;
    for (size_t i = 0; i < n; i++)
        if (!submitted[i]) ids[i] = any;   // fillers: any registered key, the verdict is ignored
    return true;
}

const char* const kSha3RefusalText = "SHA3 is served by bccsp/sw, not by the GPU provider";
}  // namespace

// bccsp/sw/impl.go:247-270 -> bccsp/sw/ecdsa.go:41-57, batched
template <class C>
Error GPUCSP::VerifyBatchT(const std::vector<VerifyItemT<typename C::Key>>& items, std::vector<VerifyResult>& results) const {
    constexpr size_t W = C::W;
    const size_t n = items.size();
    results.assign(n, VerifyResult());
    std::vector<uint8_t> qx(n * W), qy(n * W), e(n * W), r(n * W), s(n * W), st(n), submitted(n, 0);
    std::vector<uint64_t> bits((n + 63) / 64);
    for (size_t i = 0; i < n; i++) {
        const auto& it = items[i];
        const GateT<C> g = gate_item<C>(it.key, it.sig, it.siglen, it.digest, it.dlen);
        results[i] = g.res;
        submitted[i] = g.submit;
        // a slot the gate did not submit carries the generator as its key (r = s = 1, e = 0): the batch stays dense
        if (g.submit) { memcpy(&qx[W * i], it.key->x, W); memcpy(&qy[W * i], it.key->y, W); }
        else C::generator(&qx[W * i], &qy[W * i]);
        memcpy(&e[W * i], g.e, W);
        memcpy(&r[W * i], g.r, W);
        memcpy(&s[W * i], g.s, W);
    }
    if (n == 0) return Error();
    fabgpu_ctx* const ctx = flat_ctx();                      // (one device serves the whole batch; batches take turns round the pool)
    std::vector<uint32_t> ids;
    // (a key retired between the lookup and the launch would answer 4 - "internal inconsistency" below)
    int rc = all_registered<C>(ctx, n, submitted, qx.data(), qy.data(), ids)
                 ? C::verify_keyed(ctx, n, ids.data(), e.data(), r.data(), s.data(), bits.data(), st.data())
                 : C::verify(ctx, n, qx.data(), qy.data(), e.data(), r.data(), s.data(), bits.data(), st.data());
    if (rc != FABGPU_OK) return Error(std::string("GPU verify failed: ") + fabgpu_strerror(rc));
    for (size_t i = 0; i < n; i++) {
        if (!submitted[i]) continue;
        // after the host gates the device can only answer valid / arithmetic reject / r >= n
        if (st[i] == FABGPU_ST_HIGH_S || st[i] == FABGPU_ST_OFF_CURVE) return Error("internal inconsistency between host gate and device status");
        bool valid = ((bits[i >> 6] >> (i & 63)) & 1) && st[i] == FABGPU_ST_VALID;
        if (C::kTestFlip && !valid && st[i] == FABGPU_ST_BAD_MATH) {          // (test hook: a corrupted verdict)
            uint32_t f = test_p384_flip_.load(std::memory_order_relaxed);
            while (f && !test_p384_flip_.compare_exchange_weak(f, f - 1)) {}
            if (f) valid = true;
        }
        results[i].valid = valid;
        results[i].err = Error();
        // a sampled "valid" is verified again on the CPU before it leaves (rejects are re-checked by bccsp/sw on the Go side anyway)
        if (valid && !AuditDirect<C>(*items[i].key, items[i].sig, items[i].siglen, items[i].digest, items[i].dlen, "bccsp.Verify")) {
            results[i] = VerifyResult();
            results[i].err = Error(PoisonedText());
            results[i].poisoned = true;
        }
    }
    return Error();
}
Error GPUCSP::VerifyBatch(const std::vector<VerifyItem>& items, std::vector<VerifyResult>& results) const { return VerifyBatchT<Curve256>(items, results); }

VerifyResult GPUCSP::Verify(const ECDSAPublicKey* k, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen) const {
    std::vector<VerifyItem> items(1);
    items[0] = {k, sig, siglen, digest, dlen};
    std::vector<VerifyResult> res;
    Error e = VerifyBatch(items, res);
    if (!e.ok()) {
        VerifyResult r;
        r.err = e;
        r.infrastructure = true;
        return r;
    }
    return res[0];
}

// msp/identities.go:169-196 over a flattened batch: digest = Hash(msg) in the MSP's family; Verify(pk, sig, digest).  The SHA-256
// hash is fused into the verify kernel, SHA3-256 is a launch of its own ahead of the verify-only kernels (fabgpu.h).
// out[i]: "" (nil) or the error text identity.Verify would return.
template <class C>
Error GPUCSP::IdentityVerifyBatchT(const std::vector<IdentityItemT<typename C::Key>>& items, std::vector<std::string>& out, bool sha3) const {
    constexpr size_t W = C::W;
    const size_t n = items.size();
    out.assign(n, std::string());
    if (n == 0) return Error();
    std::vector<uint8_t> qx(n * W), qy(n * W), r(n * W), s(n * W), st(n), submitted(n, 0), arena;
    std::vector<uint32_t> off(n + 1);
    std::vector<uint64_t> bits((n + 63) / 64);
    static const uint8_t one_digest[1] = {1};
    size_t total = 0;                                        // bytes of the messages that are staged: the submitted rows'
    for (size_t i = 0; i < n; i++) {
        const auto& it = items[i];
        // the digest is non-empty by construction (a hash), so only key / signature gates apply here
        const GateT<C> g = gate_item<C>(it.key, it.sig, it.siglen, one_digest, 1);
        submitted[i] = g.submit;
        if (!g.submit) out[i] = g.res.err.ok() ? "The signature is invalid" : "could not determine the validity of the signature: " + g.res.err.msg;
        if (g.submit) { memcpy(&qx[W * i], it.key->x, W); memcpy(&qy[W * i], it.key->y, W); total += it.msglen; }
        else C::generator(&qx[W * i], &qy[W * i]);          // as in VerifyBatchT; the row's message is an empty span
        memcpy(&r[W * i], g.r, W);
        memcpy(&s[W * i], g.s, W);
    }
    if (total > 0xFFFFFFF0ull) return Error("message arena exceeds 32-bit offsets");
    arena.reserve(total + 8);
    for (size_t i = 0; i < n; i++) {
        off[i] = (uint32_t)arena.size();
        if (submitted[i] && items[i].msglen) arena.insert(arena.end(), items[i].msg, items[i].msg + items[i].msglen);
    }
    off[n] = (uint32_t)arena.size();
    arena.resize(arena.size() + 8);
    fabgpu_ctx* const ctx = flat_ctx();
    // The P-256 verb has always refused SHA3 here, behind the empty batch and the arena check.  The P-384 forward refuses it ahead of both
    // (its own order), so for P-384 this second check never fires.
    if (sha3 && !Sha3Enabled()) return Error(kSha3RefusalText);
    std::vector<uint32_t> ids;
    const int rc = all_registered<C>(ctx, n, submitted, qx.data(), qy.data(), ids)
                       ? (sha3 ? C::sha3_verify_keyed : C::sha256_verify_keyed)(ctx, n, arena.data(), off.data(), ids.data(), r.data(), s.data(), bits.data(), st.data())
                       : (sha3 ? C::sha3_verify : C::sha256_verify)(ctx, n, arena.data(), off.data(), qx.data(), qy.data(), r.data(), s.data(), bits.data(), st.data());
    if (rc != FABGPU_OK) return Error(std::string("GPU verify failed: ") + fabgpu_strerror(rc));
    for (size_t i = 0; i < n; i++) {
        if (!submitted[i]) continue;
        const bool ok = ((bits[i >> 6] >> (i & 63)) & 1) && st[i] == FABGPU_ST_VALID;
        out[i] = ok ? "" : "The signature is invalid";
        // as in VerifyBatchT; a sampled message is hashed again first
        if (ok && !AuditDirect<C>(*items[i].key, items[i].sig, items[i].siglen, nullptr, 0, "identity.Verify", items[i].msg, items[i].msglen, sha3)) out[i] = PoisonedText();
    }
    return Error();
}
Error GPUCSP::IdentityVerifyBatch(const std::vector<IdentityItem>& items, std::vector<std::string>& out, bool sha3) const {
    return IdentityVerifyBatchT<Curve256>(items, out, sha3);
}

// ------------------------------------------------------------------------------------------------
// one-signature calls from many threads, sharing launches (coalescer.h)
// ------------------------------------------------------------------------------------------------
template <class C, class Queue, class BatchVerb>
VerifyResult GPUCSP::VerifyCoalescedT(Queue& queue, BatchVerb verb, const typename C::Key* k, const uint8_t* sig, size_t siglen, const uint8_t* digest,
                                      size_t dlen) const {
    // the argument checks and the DER / low-S gates need no device: decided here, on the caller's thread, like Verify would
    const GateT<C> g = gate_item<C>(k, sig, siglen, digest, dlen);
    if (!g.submit) return g.res;
    typedef CoReqVT<typename C::Key> Req;
    Req req;
    req.item = {k, sig, siglen, digest, dlen};
    queue.submit(&req, [this, verb](std::vector<Req*>& batch) {
        std::vector<VerifyResult> res;
        Error e;
        try {                                                     // a runner must not throw: followers would sleep forever
            std::vector<VerifyItemT<typename C::Key>> items(batch.size());
            for (size_t i = 0; i < batch.size(); i++) items[i] = batch[i]->item;
            e = (this->*verb)(items, res);
        } catch (const std::exception& x) {
            e = Error(std::string("GPU verify failed: ") + x.what());
        }
        for (size_t i = 0; i < batch.size(); i++) {
            if (e.ok()) {
                batch[i]->res = res[i];
            } else {                                              // the device failed: an error for everybody, a verdict for nobody
                batch[i]->res = VerifyResult();
                batch[i]->res.err = e;
                batch[i]->res.infrastructure = true;
            }
        }
    });
    return req.res;
}
VerifyResult GPUCSP::VerifyCoalesced(const ECDSAPublicKey* k, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen) const {
    return VerifyCoalescedT<Curve256>(co_verify_, &GPUCSP::VerifyBatch, k, sig, siglen, digest, dlen);
}

std::string GPUCSP::IdentityVerifyCoalesced(const ECDSAPublicKey* k, const uint8_t* msg, size_t msglen, const uint8_t* sig, size_t siglen,
                                            bool* infrastructure, bool sha3) const {
    if (infrastructure) *infrastructure = false;
    static const uint8_t one_digest[1] = {1};
    const GateT<Curve256> g = gate_item<Curve256>(k, sig, siglen, one_digest, 1);   // as in IdentityVerifyBatchT: the digest is non-empty by construction
    if (!g.submit) return g.res.err.ok() ? "The signature is invalid" : "could not determine the validity of the signature: " + g.res.err.msg;
    CoReqI req;
    req.item = {k, msg, msglen, sig, siglen};
    req.infra = false;
    // one queue per hash family: a launch hashes every message of its batch the same way
    (sha3 ? co_identity_sha3_ : co_identity_).submit(&req, [this, sha3](std::vector<CoReqI*>& batch) {
        std::vector<std::string> out;
        Error e;
        try {
            std::vector<IdentityItem> items(batch.size());
            for (size_t i = 0; i < batch.size(); i++) items[i] = batch[i]->item;
            e = IdentityVerifyBatch(items, out, sha3);
        } catch (const std::exception& x) {
            e = Error(std::string("GPU verify failed: ") + x.what());
        }
        for (size_t i = 0; i < batch.size(); i++) {
            batch[i]->infra = !e.ok();
            batch[i]->out = e.ok() ? out[i] : e.msg;
        }
    });
    if (infrastructure) *infrastructure = req.infra;
    return req.out;
}

void GPUCSP::CoalescerConfigure(uint32_t window_us, uint32_t max_batch) const {
    co_verify_.configure(window_us, max_batch);
    co_identity_.configure(window_us, max_batch);
    co_identity_sha3_.configure(window_us, max_batch);
    co_verify_p384_.configure(window_us, max_batch);
}

void GPUCSP::CoalescerStats(uint64_t* calls, uint64_t* launches, uint64_t* largest_batch) const {
    uint64_t c[4], l[4], g[4];
    co_verify_.stats(&c[0], &l[0], &g[0]);
    co_identity_.stats(&c[1], &l[1], &g[1]);
    co_identity_sha3_.stats(&c[2], &l[2], &g[2]);
    co_verify_p384_.stats(&c[3], &l[3], &g[3]);
    if (calls) *calls = c[0] + c[1] + c[2] + c[3];
    if (launches) *launches = l[0] + l[1] + l[2] + l[3];
    if (largest_batch) *largest_batch = std::max(std::max(g[0], g[1]), std::max(g[2], g[3]));
}

// ------------------------------------------------------------------------------------------------
// block-level pre-verify pass (block_prepass.h)
// ------------------------------------------------------------------------------------------------
bool GPUCSP::HashMemoEnabled() const {
    std::lock_guard<std::mutex> lk(opt_mu_);
    return opts_.pass_hash_memo >= 0;
}
void GPUCSP::StartBlockUpload(BlockUpload& up, const uint8_t* block, size_t len, uint64_t block_seq, bool keep_host_copy) const {
    // The pass's device is chosen here - the block travels to it - and counts as busy until the upload object dies (pass_route.h).
    up.owner = this;
    up.dev = RouteBlock(block_seq);
    up.routed = true;
    up.block = block;
    up.len = len;
    up.seq = block_seq;
    devs_[(size_t)up.dev]->in_flight.fetch_add(1, std::memory_order_acq_rel);
    // With the walk on the device every block is staged ahead - the device route answers a 5-transaction block in 0.63 ms against
    // 0.70 ms on the host walk, a 1 000-transaction block in 0.75 against 1.4 (round-2 probe gpu_dw_tiny.sh, since removed, gpu_dw_small.sh).  Without it
    // (pass_device_walk = 0) small blocks ride with the submission through pinned staging, as before.
    // (a memo-seeding pass is staged whatever the walk: the digest memo needs the library's own copy of the block, which the upload leaves behind)
    const bool keep = keep_host_copy && HashMemoEnabled();
    size_t min_bytes = DeviceWalkEnabled() || keep ? 1 : (size_t)4 << 20;
    {
        std::lock_guard<std::mutex> lk(opt_mu_);
        if (opts_.pass_stage_min_bytes > 0) min_bytes = (size_t)opts_.pass_stage_min_bytes;   // tests choose the route with it
    }
    if (!block || len < min_bytes) return;
    fabgpu_ctx* c = devs_[(size_t)up.dev]->ctx;
    BlockUpload* u = &up;
    up.started = true;
    up.th = std::thread([c, u, block, len, keep] { u->rc = keep ? arena_stage_keep(c, block, len, &u->token, &u->copy) : fabgpu_arena_stage(c, block, len, &u->token); });
}

Error GPUCSP::PreVerifyBlock(const uint8_t* block, size_t len, BlockVerdicts& out, const PassOptions& opt) const {
    BlockUpload up;
    StartBlockUpload(up, block, len, opt.block_seq);      // the block travels while it is walked and its signatures are gated
    static thread_local ParsedBlock pb;                   // storage reused from block to block
    if (!block || !ParseBlock(block, len, pb, WalkThreads())) return Error("block does not parse as common.Block");
    Error e = PreVerifyParsed(block, pb, out, &up, opt);
    return e.ok() ? P384PassStage(block, len, pb, out, &up, opt) : e;
}


// ---- verdict memo -------------------------------------------------------------------------------------------------------
void GPUCSP::MemoKeyWrite(uint8_t* k, const uint8_t* issuer_hash32, const uint8_t* qx32, const uint8_t* qy32, const uint8_t* sig, size_t siglen,
                          const uint8_t* digest, size_t dlen) {
    // Domain first: 1 = ECDSA under the key (X, Y); 2 = idemix pseudonym signature under the ISSUER KEY whose ipk.Hash follows - a
    // verdict about (Nym, signature, message) is only ever found again by a caller who names the same issuer (two channels may define
    // one idemix MSP id with different issuer keys, and provider and memo are shared by all channels).
    *k++ = issuer_hash32 ? 2 : 1;
    if (issuer_hash32) {
        memcpy(k, issuer_hash32, 32);
        k += 32;
    }
    memcpy(k, qx32, 32);
    memcpy(k + 32, qy32, 32);
    const uint32_t sl = (uint32_t)siglen, dl = (uint32_t)dlen;      // length framing: (sig || d[:k], d[k:]) must not collide with (sig, d)
    memcpy(k + 64, &sl, 4);
    memcpy(k + 68, sig, siglen);
    memcpy(k + 68 + siglen, &dl, 4);
    memcpy(k + 72 + siglen, digest, dlen);
}
// Slot choice only (a hit is decided by comparing the whole key): the digest is SHA-256 output - uniformly distributed whatever the
// sender of the block does - mixed with the tail of the signature.
uint64_t GPUCSP::MemoHash(const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen) {
    uint64_t a = 0, b = 0;
    memcpy(&a, digest, dlen < 8 ? dlen : 8);
    memcpy(&b, sig + (siglen > 8 ? siglen - 8 : 0), siglen < 8 ? siglen : 8);
    uint64_t h = (a ^ (b * 0x9E3779B97F4A7C15ull)) * 0xD6E8FEB86659FD93ull;
    return h ^ (h >> 32);
}
// Where this thread's last lookup was answered: the validators ask in the order the block holds its signatures - identity.Verify is
// Hash(msg) then Verify(k, sig, digest) (msp/identities.go:173-188), a transaction's creator before its endorsements - so the entry a
// thread needs next is the one it just used (Verify after Hash) or its successor (the next signature of the transaction; entries are in
// tuple order).  A HINT and nothing more: the hinted entry is compared like any other - every byte of the key / of the message - and a
// thread that jumps elsewhere (another transaction, another block, a goroutine that moved to another OS thread between two cgo calls)
// falls through to the table.  What it saves is the misses: the tables were written by DMA and are cold in every cache; a probe into the
// wrong block's table plus the probe into the right one plus offsets, key, digest and status are eight to ten dependent DRAM round
// trips per signature, the hinted entry's neighbours are one or two (measured through tools/go_call_replay.c, round 6: DESIGN.md 4.4e).
namespace {
struct LookupHint {
    uint64_t gen = 0;        // BlockMemo::gen of the table (0: none)
    uint32_t entry = 0;      // 0-based entry
};
thread_local LookupHint t_hint;
std::atomic<uint64_t> g_memo_gen{1};
inline void prefetch_span(const uint8_t* p, size_t n) {
    // a message is a few KB: short for the hardware prefetcher to get going (its first lines arrive one DRAM latency apart); asked for
    // all at once, they arrive together
    for (size_t o = 0; o < n && o < 8192; o += 64) __builtin_prefetch(p + o, 0, 0);
}
}  // namespace

int GPUCSP::MemoFind(const uint8_t* qx32, const uint8_t* qy32, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen, uint8_t* status,
                     const uint8_t* issuer_hash32, uint64_t* seq, uint32_t* entry, NymCapture* nym) const {
    if (!qx32 || !qy32 || !sig || !digest || siglen == 0 || dlen == 0 || siglen > 1024 || dlen > 1024) return 1;
    uint8_t key[1 + 32 + 64 + 8 + 2048];
    const size_t kl = MemoKeyBytes(siglen, dlen, issuer_hash32 != nullptr);
    MemoKeyWrite(key, issuer_hash32, qx32, qy32, sig, siglen, digest, dlen);
    std::shared_lock<BigReaderLock> lk(memo_mu_);
    // entry e (1-based) of bm holds exactly this key?
    auto same_entry = [&](const BlockMemo& bm, uint32_t e) {
        const uint32_t o = bm.key_off_v[e - 1], l = bm.key_off_v[e] - o;
        return bm.digests_v ? (dlen == 32 && l == kl - 32 && memcmp(bm.keys_v + o, key, l) == 0 && memcmp(bm.digests_v + 32 * (size_t)(e - 1), digest, 32) == 0)
                            : (l == kl && memcmp(bm.keys_v + o, key, kl) == 0);
    };
    auto hit = [&](const BlockMemo& bm, uint32_t e) {
        if (status) *status = bm.status_v[e - 1];
        *seq = bm.seq;
        *entry = e - 1;
        t_hint.gen = bm.gen;
        t_hint.entry = e - 1;
        memo_hits_.add(1);
        // A pseudonym hit the audit samples: the proof hashes the message itself, and the caller holds only its digest - the message is
        // the entry's two spans in the block copy the digest memo keeps (the creator's Envelope.payload), copied while the lock is held.
        if (nym && audit_sample_nym_.hit(AuditPermille())) {
            nym->sampled = true;
            if (bm.hspans_v && bm.copy.p) {
                const uint32_t* sp = bm.hspans_v + 4 * (size_t)(e - 1);
                auto resolve = [&](uint32_t off, uint32_t l) -> const uint8_t* {
                    if ((uint64_t)off + l <= bm.copy.len) return bm.copy.p + off;
                    if (bm.tail_base && off >= bm.tail_base && (uint64_t)(off - bm.tail_base) + l <= bm.tail.size()) return bm.tail.data() + (off - bm.tail_base);
                    return nullptr;
                };
                const uint8_t* a = resolve(sp[0], sp[1]);
                const uint8_t* b = resolve(sp[2], sp[3]);
                if (a && b && (uint64_t)sp[1] + sp[3] != 0) {                // (spans left at zero: the entry remembers no message)
                    try {
                        nym->msg.reserve((size_t)sp[1] + sp[3]);
                        nym->msg.assign(a, a + sp[1]);
                        nym->msg.insert(nym->msg.end(), b, b + sp[3]);
                        nym->held = true;
                    } catch (...) {                                          // bad_alloc: counted as not auditable
                        nym->held = false;
                    }
                }
            }
        }
        // What this thread will most likely ask next is Hash of the NEXT entry's message: its bytes in the block's host copy, its digest
        // and its key are requested now, so that they travel while the validator builds that message (append(prp, endorser...)) instead of
        // one DRAM round trip after the other inside the comparison.  (Entry e, 0-based, is the next one; its spans share a cache line
        // with the spans just used.)
        if (e < bm.n_entries && bm.hspans_v && bm.copy.p) {
            const uint32_t* sp = bm.hspans_v + 4 * (size_t)e;
            if ((uint64_t)sp[0] + sp[1] <= bm.copy.len) prefetch_span(bm.copy.p + sp[0], sp[1]);
            if ((uint64_t)sp[2] + sp[3] <= bm.copy.len) prefetch_span(bm.copy.p + sp[2], sp[3]);
            if (bm.digests_v) __builtin_prefetch(bm.digests_v + 32 * (size_t)e, 0, 3);
            __builtin_prefetch(bm.keys_v + bm.key_off_v[e], 0, 3);
            __builtin_prefetch(bm.keys_v + bm.key_off_v[e] + 64, 0, 3);
        }
        return 0;
    };
    const BlockMemo* hinted = nullptr;
    if (t_hint.gen)
        for (const auto& b : memo_blocks_)
            if (b->gen == t_hint.gen) hinted = b.get();
    if (hinted && hinted->n) {
        // the entry this thread's Hash just found, or the one behind the entry its last Verify found
        for (uint32_t e0 = t_hint.entry; e0 <= t_hint.entry + 1 && e0 < hinted->n_entries; e0++)
            if (hinted->status_v[e0] <= FABGPU_ST_RANGE && same_entry(*hinted, e0 + 1)) return hit(*hinted, e0 + 1);
    }
    const uint64_t h = MemoHash(sig, siglen, digest, dlen);
    auto probe_block = [&](const BlockMemo& bm) -> uint32_t {
        if (!bm.n) return 0;
        for (uint32_t probe = 0, at = (uint32_t)h & bm.mask; probe <= bm.mask && probe < 4096; probe++, at = (at + 1) & bm.mask) {
            const uint32_t e = bm.slots_v[at];                             // (published under the lock: complete)
            if (!e) break;
            if (e > bm.n_entries) break;                                    // (never: an index past the entries)
            if (same_entry(bm, e)) return e;
        }
        return 0;
    };
    if (hinted)
        if (const uint32_t e = probe_block(*hinted)) return hit(*hinted, e);
    for (auto it = memo_blocks_.rbegin(); it != memo_blocks_.rend(); ++it) {      // newest block first
        if (it->get() == hinted) continue;
        if (const uint32_t e = probe_block(**it)) return hit(**it, e);
    }
    memo_misses_.add(1);
    return 1;
}
// bccsp.Hash for bytes a pass has already hashed (bccsp_host.h).  The fingerprint (and the hint above) only choose where to look; what
// is answered is decided by comparing the caller's bytes with the block's, every one of them.
int GPUCSP::HashFind(const uint8_t* msg, size_t len, uint8_t* digest32, uint64_t* seq, uint32_t* entry) const {
    if (!msg || !digest32 || len < walk::HASH_MEMO_MIN_LEN || len > 0x7FFFFFF0ull) return 1;
    std::shared_lock<BigReaderLock> lk(memo_mu_);
    auto usable = [](const BlockMemo& bm) { return bm.n && bm.hslots_v && bm.hspans_v && bm.copy.p; };
    // entry e0 (0-based) of bm: the device hashed and decided it, and its message is the caller's, byte for byte?
    auto matches = [&](const BlockMemo& bm, uint32_t e0) {
        const uint32_t* sp = bm.hspans_v + 4 * (size_t)e0;
        if ((uint64_t)sp[1] + sp[3] != len) return false;
        if (bm.status_v[e0] > FABGPU_ST_RANGE) return false;                // a candidate the device did not hash and decide: no digest to hand out
        // where a span lies on the host: in the copy of the block, or (the orderers' signature messages) in the tail kept beside it
        auto resolve = [&](uint32_t off, uint32_t l) -> const uint8_t* {
            if ((uint64_t)off + l <= bm.copy.len) return bm.copy.p + off;
            if (bm.tail_base && off >= bm.tail_base && (uint64_t)(off - bm.tail_base) + l <= bm.tail.size()) return bm.tail.data() + (off - bm.tail_base);
            return nullptr;
        };
        const uint8_t* a = resolve(sp[0], sp[1]);
        const uint8_t* b = resolve(sp[2], sp[3]);
        if (!a || !b) return false;
        prefetch_span(a, sp[1]);
        prefetch_span(b, sp[3]);
        __builtin_prefetch(bm.digests_v ? bm.digests_v + 32 * (size_t)e0 : bm.keys_v + bm.key_off_v[e0 + 1] - 32, 0, 3);
        return memcmp(msg, a, sp[1]) == 0 && memcmp(msg + sp[1], b, sp[3]) == 0;
    };
    auto hit = [&](const BlockMemo& bm, uint32_t e0) {
        const uint8_t* d = bm.digests_v ? bm.digests_v + 32 * (size_t)e0 : bm.keys_v + bm.key_off_v[e0 + 1] - 32;
        memcpy(digest32, d, 32);
        *seq = bm.seq;
        *entry = e0;
        __builtin_prefetch(bm.keys_v + bm.key_off_v[e0], 0, 3);            // (the Verify that follows compares this entry's key)
        t_hint.gen = bm.gen;
        t_hint.entry = e0;
        hash_hits_.add(1);
        return 0;
    };
    const BlockMemo* hinted = nullptr;
    if (t_hint.gen)
        for (const auto& b : memo_blocks_)
            if (b->gen == t_hint.gen) hinted = b.get();
    if (hinted && !usable(*hinted)) hinted = nullptr;
    if (hinted) {
        // the message behind the one this thread asked about last (the next signature of the transaction), or that one again
        if (t_hint.entry + 1 < hinted->n_entries && matches(*hinted, t_hint.entry + 1)) return hit(*hinted, t_hint.entry + 1);
        if (t_hint.entry < hinted->n_entries && matches(*hinted, t_hint.entry)) return hit(*hinted, t_hint.entry);
    }
    const uint64_t h = walk::msg_fingerprint(msg, (uint32_t)len, nullptr, 0);
    auto probe_block = [&](const BlockMemo& bm) -> int64_t {
        uint32_t compared = 0;
        for (uint32_t probe = 0, at = (uint32_t)h & bm.mask; probe <= bm.mask && probe < 256; probe++, at = (at + 1) & bm.mask) {
            const uint32_t e = bm.hslots_v[at];
            if (!e) break;
            if (e > bm.n_entries) break;                                    // (never: an index past the entries)
            const uint32_t* sp = bm.hspans_v + 4 * (size_t)(e - 1);
            if ((uint64_t)sp[1] + sp[3] != len) continue;
            if (matches(bm, e - 1)) return (int64_t)(e - 1);
            if (++compared >= walk::HASH_MEMO_MAX_PROBES) break;            // equal lengths and fingerprints, other bytes: a bounded number of tries
        }
        return -1;
    };
    if (hinted) {
        const int64_t e0 = probe_block(*hinted);
        if (e0 >= 0) return hit(*hinted, (uint32_t)e0);
    }
    for (auto it = memo_blocks_.rbegin(); it != memo_blocks_.rend(); ++it) {      // newest block first
        if (it->get() == hinted || !usable(**it)) continue;
        const int64_t e0 = probe_block(**it);
        if (e0 >= 0) return hit(**it, (uint32_t)e0);
    }
    hash_misses_.add(1);
    return 1;
}
// ---- CPU audit of what the lookups and the direct calls hand out; poisoning (bccsp_host.h, audit_host.h) -----------------------------
namespace {
struct AuditClock {                                          // time spent auditing, added to the provider's counter when the audit is over
    std::atomic<uint64_t>& ns;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~AuditClock() { ns.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(), std::memory_order_relaxed); }
};
std::string hex8(const uint8_t* p) {
    static const char* H = "0123456789abcdef";
    std::string s;
    for (int i = 0; i < 8; i++) { s.push_back(H[p[i] >> 4]); s.push_back(H[p[i] & 15]); }
    return s;
}
}  // namespace
const char* GPUCSP::PoisonedText() { return "GPU provider poisoned: the CPU audit disagrees with the device (use bccsp/sw)"; }
void GPUCSP::Poison(const std::string& why) const {
    {
        std::lock_guard<std::mutex> lk(poison_mu_);
        if (poison_why_.empty()) poison_why_ = why.empty() ? "poisoned" : why;   // (the first reason stays)
    }
    if (!poisoned_.exchange(true, std::memory_order_acq_rel))
        fprintf(stderr, "fabgpu: provider poisoned, everything is left to bccsp/sw from now on: %s\n", why.c_str());
}
bool GPUCSP::Poisoned(std::string* why) const {
    if (!poisoned_.load(std::memory_order_acquire)) return false;
    if (why) {
        std::lock_guard<std::mutex> lk(poison_mu_);
        *why = poison_why_;
    }
    return true;
}
void GPUCSP::AuditStats(uint64_t out[AUDIT_STATS]) const {
    for (int i = 0; i < AUDIT_STATS; i++) out[i] = audit_count_[i].load(std::memory_order_relaxed);
}
bool GPUCSP::AuditIssuerById(int64_t issuer_id, AuditIssuer& out) const {
    std::lock_guard<std::mutex> lk(audit_issuer_mu_);
    auto it = audit_issuers_.find(issuer_id);
    if (it == audit_issuers_.end()) return false;
    out = it->second;
    return true;
}
bool GPUCSP::AuditIssuerByHash(const uint8_t* hash32, AuditIssuer& out) const {
    std::lock_guard<std::mutex> lk(audit_issuer_mu_);
    for (const auto& kv : audit_issuers_)                                   // (a peer's idemix MSPs: a handful)
        if (!memcmp(kv.second.data() + 128, hash32, 32)) {
            out = kv.second;
            return true;
        }
    return false;
}
bool GPUCSP::AuditNymDirect(int64_t issuer_id, const uint8_t* nym_x32, const uint8_t* nym_y32, const uint8_t* sig, size_t siglen, const uint8_t* msg,
                            size_t msglen) const {
    if (!audit_sample_nym_.hit(AuditPermille())) return true;
    AuditIssuer iss;
    if (!AuditIssuerById(issuer_id, iss)) {                                 // an issuer the provider did not import itself: counted, handed out
        audit_count_[AUDIT_SKIPPED_NYM].fetch_add(1, std::memory_order_relaxed);
        return true;
    }
    bool accept;
    {
        AuditClock clk{audit_count_[AUDIT_NS]};
        accept = audit_nym_verify(iss.data(), iss.data() + 32, iss.data() + 64, iss.data() + 96, iss.data() + 128, nym_x32, nym_y32, sig, siglen, msg, msglen);
    }
    audit_count_[AUDIT_NYM].fetch_add(1, std::memory_order_relaxed);
    if (accept) return true;
    audit_count_[AUDIT_MISMATCHES].fetch_add(1, std::memory_order_relaxed);
    Poison(std::string("pseudonym audit: the device accepted a pseudonym signature in NymVerifier.Verify that the CPU audit rejects (Nym X ") + hex8(nym_x32) + "..)");
    return false;
}
template <class C>
bool GPUCSP::AuditDirect(const typename C::Key& k, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen, const char* what,
                         const uint8_t* msg, size_t msglen, bool sha3) const {
    if (!audit_sample_[AUDIT_DIRECT].hit(AuditPermille())) return true;
    bool accept;
    {
        AuditClock clk{audit_count_[AUDIT_NS]};
        uint8_t dg[32];
        if (msg || msglen) {
            if (sha3) audit_sha3_256(msg, msglen, dg);          // the family the call hashed with
            else audit_sha256(msg, msglen, dg);
            digest = dg;
            dlen = 32;
        }
        accept = C::audit(k.x, k.y, sig, siglen, digest, dlen);
    }
    audit_count_[AUDIT_DIRECT].fetch_add(1, std::memory_order_relaxed);
    if (accept) return true;
    audit_count_[AUDIT_MISMATCHES].fetch_add(1, std::memory_order_relaxed);
    Poison(std::string("direct call: the device accepted ") + C::kAuditNoun + " in " + what + " that the CPU audit rejects (key X " + hex8(k.x) + "..)");
    return false;
}
// ------------------------------------------------------------------------------------------------
// ECDSA P-384 identities (option p384): the P-256 verbs' answers and texts on the P-384 entries of fabgpu.h
// ------------------------------------------------------------------------------------------------
const char* GPUCSP::P384RefusalText() { return "P-384 is served by bccsp/sw, not by the GPU provider"; }
void GPUCSP::KeyImport384(const uint8_t* qx48, const uint8_t* qy48, ECDSAPublicKey384& out) {
    memcpy(out.x, qx48, 48);
    memcpy(out.y, qy48, 48);
    out.on_curve = p384::pubkey_on_curve(qx48, qy48);
}
Error GPUCSP::KeyImportP384(const uint8_t* qx48, const uint8_t* qy48, ECDSAPublicKey384& out) const {
    if (!qx48 || !qy48) return Error("Invalid raw. It must not be nil.");
    KeyImport384(qx48, qy48, out);
    if (!P384Enabled()) return Error(P384RefusalText());
    if (!out.on_curve) return Error();                        // (as KeyImport: such a key stays with bccsp/sw, nothing is registered)
    std::lock_guard<std::mutex> lk(reg_mu_);
    const int G = (int)devs_.size();
    fabgpu_ctx* cs[kMaxProviderDevices];
    uint32_t ids[kMaxProviderDevices];
    for (int g = 0; g < G; g++) cs[g] = devs_[(size_t)g]->ctx;
    const int rc = fabgpu_p384_key_register_many(cs, G, qx48, qy48, ids);
    // best effort: a device without the table serves the key on the fresh-key kernel (the choice is made per batch on the batch's device)
    if (rc != FABGPU_OK && !reg_failure_logged_) {
        reg_failure_logged_ = true;
        fprintf(stderr, "fabgpu: a P-384 key table could not be installed on every device (%s); the key verifies on the fresh-key kernel\n", fabgpu_strerror(rc));
    }
    return Error();
}
// the P-384 direct calls: with the option off every item answers the refusal, nothing is gated or launched
Error GPUCSP::VerifyBatchP384(const std::vector<VerifyItem384>& items, std::vector<VerifyResult>& results) const {
    if (!P384Enabled()) {
        results.assign(items.size(), VerifyResult());
        for (auto& r : results) r.err = Error(P384RefusalText()), r.needs_sw = true;
        return Error();
    }
    return VerifyBatchT<Curve384>(items, results);
}
Error GPUCSP::IdentityVerifyBatchP384(const std::vector<IdentityItem384>& items, std::vector<std::string>& out, bool sha3) const {
    if (!P384Enabled()) {
        out.assign(items.size(), std::string("could not determine the validity of the signature: ") + P384RefusalText());
        return Error();
    }
    out.assign(items.size(), std::string());
    if (sha3 && !Sha3Enabled()) return Error(kSha3RefusalText);   // (ahead of the empty batch, as this verb always had it)
    return IdentityVerifyBatchT<Curve384>(items, out, sha3);
}
VerifyResult GPUCSP::VerifyCoalescedP384(const ECDSAPublicKey384* k, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen) const {
    if (!P384Enabled()) {
        VerifyResult r;
        r.err = Error(P384RefusalText());
        r.needs_sw = true;
        return r;
    }
    return VerifyCoalescedT<Curve384>(co_verify_p384_, &GPUCSP::VerifyBatchP384, k, sig, siglen, digest, dlen);
}

int GPUCSP::MemoLookup(const uint8_t* qx32, const uint8_t* qy32, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen, uint8_t* status,
                       const uint8_t* issuer_hash32) const {
    if (poisoned_.load(std::memory_order_acquire)) return 1;
    uint64_t seq = 0;
    uint32_t entry = 0;
    uint8_t st = 0xFF;
    NymCapture nym;
    if (MemoFind(qx32, qy32, sig, siglen, digest, dlen, &st, issuer_hash32, &seq, &entry, issuer_hash32 && AuditPermille() ? &nym : nullptr) != 0) return 1;
    if (issuer_hash32) {
        // a pseudonym entry: first the device's digest over the message the entry remembers, then NymSignature.Ver under the issuer key
        // the entry is bound to.  No copy of the block, or no fields for that issuer hash: handed out as it is, and counted.
        AuditIssuer iss;
        if (!nym.sampled) {                                                  // (not this hit's turn, or auditing is off)
        } else if (!nym.held || !AuditIssuerByHash(issuer_hash32, iss)) {
            audit_count_[AUDIT_SKIPPED_NYM].fetch_add(1, std::memory_order_relaxed);
        } else {
            uint8_t want[32];
            bool same_digest, accept = false;
            {
                AuditClock clk{audit_count_[AUDIT_NS]};
                audit_sha256(nym.msg.data(), nym.msg.size(), want);
                same_digest = dlen == 32 && memcmp(want, digest, 32) == 0;
                if (same_digest)
                    accept = audit_nym_verify(iss.data(), iss.data() + 32, iss.data() + 64, iss.data() + 96, iss.data() + 128, qx32, qy32, sig, siglen, nym.msg.data(),
                                              nym.msg.size());
            }
            audit_count_[AUDIT_NYM].fetch_add(1, std::memory_order_relaxed);
            if (!same_digest) {
                audit_count_[AUDIT_MISMATCHES].fetch_add(1, std::memory_order_relaxed);
                Poison("pseudonym audit: block " + std::to_string(seq) + " entry " + std::to_string(entry) + " holds digest " + hex8(digest) +
                       ".., the CPU audit computes " + hex8(want) + ".. over the " + std::to_string(nym.msg.size()) + " bytes of the message the entry remembers");
                return 1;
            }
            if (accept != (st == FABGPU_NYM_VALID)) {
                audit_count_[AUDIT_MISMATCHES].fetch_add(1, std::memory_order_relaxed);
                Poison("pseudonym audit: block " + std::to_string(seq) + " entry " + std::to_string(entry) + " holds status " + std::to_string(st) +
                       ", the CPU audit says " + (accept ? "valid" : "invalid") + " (Nym X " + hex8(qx32) + "..)");
                return 1;
            }
        }
    } else if (audit_sample_[AUDIT_VERDICT].hit(AuditPermille())) {
        bool accept;
        {
            AuditClock clk{audit_count_[AUDIT_NS]};
            accept = audit_p256_verify(qx32, qy32, sig, siglen, digest, dlen);
        }
        audit_count_[AUDIT_VERDICT].fetch_add(1, std::memory_order_relaxed);
        if (accept != (st == FABGPU_ST_VALID)) {
            audit_count_[AUDIT_MISMATCHES].fetch_add(1, std::memory_order_relaxed);
            Poison("verdict memo: block " + std::to_string(seq) + " entry " + std::to_string(entry) + " holds status " + std::to_string(st) + ", the CPU audit says " +
                   (accept ? "valid" : "invalid") + " (key X " + hex8(qx32) + "..)");
            return 1;
        }
    }
    if (poisoned_.load(std::memory_order_acquire)) return 1;                 // (another thread's audit failed meanwhile)
    if (status) *status = st;
    return 0;
}
int GPUCSP::HashLookup(const uint8_t* msg, size_t len, uint8_t* digest32) const {
    if (poisoned_.load(std::memory_order_acquire)) return 1;
    uint64_t seq = 0;
    uint32_t entry = 0;
    uint8_t dg[32];
    if (!digest32 || HashFind(msg, len, dg, &seq, &entry) != 0) return 1;
    if (audit_sample_[AUDIT_DIGEST].hit(AuditPermille())) {
        uint8_t want[32];
        {
            AuditClock clk{audit_count_[AUDIT_NS]};
            audit_sha256(msg, len, want);
        }
        audit_count_[AUDIT_DIGEST].fetch_add(1, std::memory_order_relaxed);
        if (memcmp(want, dg, 32) != 0) {
            audit_count_[AUDIT_MISMATCHES].fetch_add(1, std::memory_order_relaxed);
            Poison("digest memo: block " + std::to_string(seq) + " entry " + std::to_string(entry) + " holds digest " + hex8(dg) + ".., the CPU audit computes " + hex8(want) +
                   ".. over the same " + std::to_string(len) + " bytes");
            return 1;
        }
    }
    if (poisoned_.load(std::memory_order_acquire)) return 1;
    memcpy(digest32, dg, 32);
    return 0;
}
void GPUCSP::HashMemoStats(uint64_t* hits, uint64_t* misses, uint64_t* blocks_held, uint64_t* bytes_held, uint64_t* refused) const {
    if (hits) *hits = hash_hits_.load();
    if (misses) *misses = hash_misses_.load();
    uint64_t h = 0, b = 0, r = 0;
    for (const auto& d : devs_) {
        uint64_t dh = 0, db = 0, dr = 0;
        host_copy_stats(d->ctx, &dh, &db, &dr);
        h += dh; b += db; r += dr;
    }
    if (blocks_held) *blocks_held = h;
    if (bytes_held) *bytes_held = b;
    if (refused) *refused = r;
}
size_t GPUCSP::MemoHasBlock(uint64_t block_seq) const {
    size_t n = p384_memo_.HasBlock(block_seq);                               // (its own lock, taken and left before the P-256 table's)
    std::shared_lock<BigReaderLock> lk(memo_mu_);
    for (const auto& b : memo_blocks_)
        if (b->seq == block_seq) n += b->n;
    return n;
}
size_t GPUCSP::MemoEvictBlock(uint64_t block_seq) const {
    size_t gone = p384_memo_.EvictBlock(block_seq);                          // the block's P-384 record, counted by that table's own counter
    const size_t gone384 = gone;
    std::unique_lock<BigReaderLock> lk(memo_mu_);
    for (auto b = memo_blocks_.begin(); b != memo_blocks_.end();) {
        if ((*b)->seq != block_seq) { ++b; continue; }
        gone += (*b)->n;
        (*b)->ReleaseCopy();                                                  // the host copy of the block goes back to its device's pool
        if (memo_free_.size() < memo_free_max_) memo_free_.push_back(*b);     // its buffers serve the next block (lookups hold the shared lock: none in flight here)
        b = memo_blocks_.erase(b);
    }
    memo_evicted_.fetch_add(gone - gone384, std::memory_order_relaxed);      // (MemoStats stays about P-256 entries)
    return gone;
}
void GPUCSP::MemoStats(uint64_t* entries, uint64_t* hits, uint64_t* misses, uint64_t* evicted) const {
    std::shared_lock<BigReaderLock> lk(memo_mu_);
    uint64_t n = 0;
    for (const auto& b : memo_blocks_) n += b->n;
    if (entries) *entries = n;
    if (hits) *hits = memo_hits_.load();
    if (misses) *misses = memo_misses_.load();
    if (evicted) *evicted = memo_evicted_.load();
}
void GPUCSP::MemoSetCapacity(size_t max_entries) const {
    std::unique_lock<BigReaderLock> lk(memo_mu_);
    memo_cap_ = max_entries ? max_entries : 1;
}
// ---- the verdict memo of the pass's P-384 tuples (p384_memo.h; seeded by P384PassStage) ----
int GPUCSP::MemoLookupP384(const uint8_t* qx48, const uint8_t* qy48, const uint8_t* sig, size_t siglen, const uint8_t* digest, size_t dlen, uint8_t* status,
                           uint64_t* block_seq) const {
    if (!P384Enabled() || poisoned_.load(std::memory_order_acquire)) return 1;
    uint64_t seq = 0;
    uint32_t entry = 0;
    uint8_t st = 0xFF;
    if (p384_memo_.Lookup(qx48, qy48, sig, siglen, digest, dlen, &st, &seq, &entry) != 0) return 1;
    // sampled as the P-256 entries are: the hit is decided again over the caller's arguments, against stored status 0 / anything else
    if (audit_sample_p384_memo_.hit(AuditPermille())) {
        bool accept;
        {
            AuditClock clk{audit_count_[AUDIT_NS]};
            accept = audit_p384_verify(qx48, qy48, sig, siglen, digest, dlen);
        }
        audit_count_[AUDIT_VERDICT_P384].fetch_add(1, std::memory_order_relaxed);
        if (accept != (st == FABGPU_ST_VALID)) {
            audit_count_[AUDIT_MISMATCHES].fetch_add(1, std::memory_order_relaxed);
            Poison("P-384 verdict memo: block " + std::to_string(seq) + " entry " + std::to_string(entry) + " holds status " + std::to_string(st) +
                   ", the CPU audit says " + (accept ? "valid" : "invalid") + " (key X " + hex8(qx48) + "..)");
            return 1;
        }
    }
    if (poisoned_.load(std::memory_order_acquire)) return 1;                 // (another thread's audit failed meanwhile)
    if (status) *status = st;
    if (block_seq) *block_seq = seq;
    return 0;
}
void GPUCSP::MemoStatsP384(uint64_t* entries, uint64_t* hits, uint64_t* misses, uint64_t* evicted) const { p384_memo_.Stats(entries, hits, misses, evicted); }
void GPUCSP::MemoSetCapacityP384(size_t max_entries) const { p384_memo_.SetCapacity(max_entries); }
void GPUCSP::SetIdentityCacheLimits(size_t max_identities, size_t max_registered_keys, uint32_t register_after_hits) const {
    {
        std::lock_guard<std::mutex> lk(idmu_);
        id_max_ = max_identities ? max_identities : 1;
        id_max_registered_ = max_registered_keys;
        id_register_after_ = register_after_hits ? register_after_hits : 1;
        EvictIdentitiesLocked();
        id_version_.fetch_add(1, std::memory_order_release);
    }
    FlushRetirements();
}
// (idmu_ held) the LRU bound.  An identity that owned a device comb table gives its place in the table budget back: the table itself
// stays registered with the context (launches in flight may still name it; fabgpu_p256_key_register finds it again by key should the
// identity return), but id_registered_ counts the tables of CACHED identities - otherwise a provider that churned through more than
// id_max_registered_ registered identities could never register another one and stayed on the fresh-key kernels for good.
// With retire_evicted_keys the table goes too: the key is queued here and retired on every device by FlushRetirements (an identity
// whose registration is still under way is queued by RegisterQueued, when that registration finds the identity gone).
void GPUCSP::EvictIdentitiesLocked() const {
    while (idcache_.size() > id_max_) {
        const CachedIdentity c = idlru_.back().second;
        if ((c.key_id >= 0 || c.registering) && id_registered_ > 0) id_registered_--;
        idserial_.erase(c.serial);
        idcache_.erase(idlru_.back().first);
        idlru_.pop_back();
        if (c.p256 && c.key_id >= 0 && retire_evicted_.load(std::memory_order_relaxed)) QueueRetirementLocked(c.qx, c.qy);
    }
}
void GPUCSP::QueueRetirementLocked(const uint8_t* qx32, const uint8_t* qy32) const {
    for (const auto& kv : idlru_) {
        const CachedIdentity& o = kv.second;
        if (o.p256 && (o.key_id >= 0 || o.registering) && !memcmp(o.qx, qx32, 32) && !memcmp(o.qy, qy32, 32)) return;   // (two certificates, one key)
    }
    std::string k((const char*)qx32, 32);
    k.append((const char*)qy32, 32);
    std::lock_guard<std::mutex> lk(retire_mu_);
    retire_queue_.push_back(std::move(k));
}
void GPUCSP::FlushRetirements() const {
    {
        std::lock_guard<std::mutex> lk(retire_mu_);
        if (retire_queue_.empty()) return;
    }
    std::lock_guard<std::mutex> lk(reg_mu_);
    FlushRetirementsRegLocked();
}
void GPUCSP::FlushRetirementsRegLocked() const {
    std::vector<std::string> q;
    {
        std::lock_guard<std::mutex> lk(retire_mu_);
        if (retire_queue_.empty()) return;
        q.swap(retire_queue_);
        for (auto& k : q)
            if (imported_keys_.count(k)) k.clear();
    }
    {
        // an identity with this key may be back in the cache since the key was queued, and may have been handed the still-registered
        // id by an idempotent registration: then the table stays (lock order reg_mu_, then idmu_: nothing takes reg_mu_ while it holds idmu_)
        std::lock_guard<std::mutex> lk(idmu_);
        for (auto& k : q) {
            if (k.empty()) continue;
            for (const auto& kv : idlru_) {
                const CachedIdentity& o = kv.second;
                if (o.p256 && (o.key_id >= 0 || o.registering) && !memcmp(o.qx, k.data(), 32) && !memcmp(o.qy, k.data() + 32, 32)) {
                    k.clear();
                    break;
                }
            }
        }
    }
    const int G = (int)devs_.size();
    fabgpu_ctx* cs[kMaxProviderDevices];
    for (int g = 0; g < G; g++) cs[g] = devs_[(size_t)g]->ctx;
    for (const std::string& k : q) {
        if (k.empty()) continue;
        const int rc = fabgpu_p256_key_unregister_many(cs, G, (const uint8_t*)k.data(), (const uint8_t*)k.data() + 32);
        if (rc == FABGPU_OK || rc == 2) keys_retired_.fetch_add(1, std::memory_order_relaxed);
        if (rc == 2) reg_id_mismatches_.fetch_add(1, std::memory_order_relaxed);      // (some devices had the key and some had not: the pool was lopsided)
    }
}
int GPUCSP::KeyTableStats(int d, uint64_t* out, int cap) const {
    if (d < 0 || d >= (int)devs_.size()) return FABGPU_EINVAL;
    const int n = fabgpu_p256_key_table_stats(devs_[(size_t)d]->ctx, out, cap);
    if (n < 0) return n;
    if (cap > n) out[n] = keys_retired_.load(std::memory_order_relaxed);
    return n + 1;
}
void GPUCSP::InsertIdentityLocked(std::string&& key, CachedIdentity ci, bool evict_now) const {
    ci.table_hash = walk::id_hash_host((const uint8_t*)key.data(), (uint32_t)key.size(), idtab_seed_);
    ci.serial = id_next_serial_++;
    idlru_.emplace_front(std::move(key), ci);
    idcache_[idlru_.front().first] = idlru_.begin();
    idserial_[ci.serial] = idlru_.begin();
    if (evict_now) EvictIdentitiesLocked();
}
void GPUCSP::PassStats(uint64_t out[4]) const {
    out[0] = pass_relaunches_.load(std::memory_order_relaxed);
    out[1] = pass_decoded_.load(std::memory_order_relaxed);
    out[2] = pass_learned_.load(std::memory_order_relaxed);
    out[3] = pass_general_der_.load(std::memory_order_relaxed);
}
size_t GPUCSP::IdentityCacheSize() const {
    std::lock_guard<std::mutex> lk(idmu_);
    return idcache_.size();
}

int64_t GPUCSP::RegisterIdemixMSP(const std::string& mspid, const uint8_t* ipk_raw, size_t len, const std::string& channel) const {
    IdemixIssuerPublicKey k;
    // (what the key holds - its bases and its hash - read once, without a device; the registration itself goes to every device)
    if (!IdemixCSP::IssuerKeyFields(ipk_raw, len, k)) return -1;
    k.issuer_id = ImportIdemixIssuer(ipk_raw, len);
    std::lock_guard<std::mutex> lk(idmu_);
    if (k.issuer_id >= 0) {
        std::array<uint8_t, 32> h;
        memcpy(h.data(), k.hash, 32);
        idemix_issuer_hash_[k.issuer_id] = h;
    }
    // The pass sees a creator's MSP id, not its channel.  Each channel's LATEST key for the MSP id is remembered (a config update that
    // rotates the issuer key replaces that channel's entry); while all channels that name the MSP id agree on one key the pass verifies
    // under it, and while two of them differ (two channels that both call their idemix MSP "IdemixMSP1") it cannot tell under which
    // key a creator verifies: creators of that MSP id stay with bccsp/idemix (-2) - until the channels agree again.
    // (a caller that names no channel cannot rotate: every distinct key counts as a channel of its own)
    std::map<std::string, int64_t>& by_channel = idemix_msp_channels_[mspid];
    by_channel[channel.empty() ? "#" + std::to_string(k.issuer_id) : channel] = k.issuer_id;
    int64_t resolved = k.issuer_id;
    for (const auto& kv : by_channel)
        if (kv.second != k.issuer_id) resolved = -2;
    idemix_msps_[mspid] = resolved;
    return k.issuer_id;
}

namespace {
constexpr int kGateMax = 16;     // most worker threads a pass runs at once: the pool + the caller (worker_pool.h)
// a stage clock of the pass: the milliseconds from its construction to the end of its scope go into `ms`
struct StageClock {
    double& ms;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~StageClock() { ms = ms_since(t0); }
};
}  // namespace

GPUCSP::ScratchLease::ScratchLease(const GPUCSP* c_) : c(c_) {
    std::lock_guard<std::mutex> lk(c->pass_mu_);
    if (!c->scratch_free_.empty()) {
        p = std::move(c->scratch_free_.back());
        c->scratch_free_.pop_back();
    }
    if (!p) p.reset(new PassScratch);
}
GPUCSP::ScratchLease::~ScratchLease() {
    std::lock_guard<std::mutex> lk(c->pass_mu_);
    if (c->scratch_free_.size() < c->scratch_free_max_) c->scratch_free_.push_back(std::move(p));
}

bool GPUCSP::EarnTableLocked(CachedIdentity& c) const {
    if (!c.p256 || c.key_id >= 0 || c.registering || c.hits < id_register_after_ || id_registered_ >= id_max_registered_) return false;
    c.registering = true;
    id_registered_++;
    return true;
}

// identities that earned a device comb table during a block: built and uploaded outside idmu_ (6 ms of host work each)
void GPUCSP::RegisterQueued(const std::vector<std::string>& to_register) const {
    if (to_register.empty()) {
        FlushRetirements();                                  // (what this pass evicted)
        return;
    }
    std::vector<std::pair<std::string, CachedIdentity>> todo;
    {
        std::lock_guard<std::mutex> lk(idmu_);
        for (const std::string& k : to_register) {
            auto it = idcache_.find(k);
            if (it != idcache_.end()) todo.emplace_back(k, it->second->second);
            // (evicted meanwhile: EvictIdentitiesLocked gave its place in the table budget back)
        }
    }
    // Round 6: the tables are built ON THE DEVICE, the whole batch in three launches per device (keytab_kernels.hip: 0.7-0.9 ms for a
    // channel's six signers against 6 ms of host arithmetic per key - eight of the fifteen milliseconds of a fresh provider's first pass),
    // the devices of the pool side by side, every device installing the keys in the same order: the same ids everywhere.  A device that
    // cannot (memory, a failed launch) sends the batch down the old road: host-built tables, one key after the other.
    std::vector<int64_t> batch_ids(todo.size(), -1);
    const bool batch_ok = RegisterKeysOnAllDevices(todo, batch_ids);
    const size_t words = key_table_words();
    std::vector<std::vector<int32_t>> tabs(todo.size());
    if (!batch_ok && todo.size() > 1)
        run_workers((int)todo.size(), [&](int i) {
            tabs[(size_t)i].resize(words);
            if (!key_table_build(todo[(size_t)i].second.qx, todo[(size_t)i].second.qy, tabs[(size_t)i].data())) tabs[(size_t)i].clear();
        });
    for (size_t ti = 0; ti < todo.size(); ti++) {
        auto& kv = todo[ti];
        const int64_t id = batch_ok ? batch_ids[ti]
                                    : RegisterKeyOnAllDevices(kv.second.qx, kv.second.qy, tabs[ti].empty() ? nullptr : tabs[ti].data());   // every device gets a copy
        const bool ok = id >= 0;
        std::lock_guard<std::mutex> lk(idmu_);
        auto it = idcache_.find(kv.first);
        if (it != idcache_.end()) {
            it->second->second.registering = false;
            if (ok) it->second->second.key_id = id;
            else if (id_registered_ > 0) id_registered_--;
        } else if (ok && retire_evicted_.load(std::memory_order_relaxed)) {
            QueueRetirementLocked(kv.second.qx, kv.second.qy);      // (evicted while its table was being built)
        }
        if (ok) id_version_.fetch_add(1, std::memory_order_release);    // (a failed attempt changed nothing the devices' tables show)
    }
    FlushRetirements();
}

void GPUCSP::SeedMemo(const uint8_t* block, const ParsedBlock& pb, BlockVerdicts& out, const PassOptions& opt, std::vector<uint32_t>& sel_scratch,
                      int gate_max, BlockUpload* up) const {
    const size_t nt = pb.tuples.size();
    // verdict memo: one entry per tuple the device hashed and decided, keyed on (key, signature bytes, device digest).  The block's
    // table is built here, outside the memo lock, by the pass's worker threads; publishing it is one push under the lock.
    {
        StageClock memo_clock{out.ms_memo};
        std::shared_ptr<BlockMemo> bm = TakeMemoTable(/*prefer_pinned=*/false);
        bm->seq = opt.block_seq;
        bm->n = 0;
        // Which tuples get an entry: the ones the device hashed and decided with a status bccsp.Verify decides itself (0 valid, 1 bad math,
        // 2 high-S, 3 range).  (Pseudonym signatures: key = domain 2 || ipk.Hash of the issuer it was verified under || Nym.x || Nym.y,
        // digest = SHA-256(message), status 0 valid / 1 proof invalid.)
        // a pseudonym signature's entry is bound to the issuer key it was verified under (BlockVerdicts::tuple_nym_issuer, filled by the pass);
        // a nym tuple whose issuer hash is not at hand gets no entry at all
        std::map<int64_t, std::array<uint8_t, 32>> issuer_hash;
        {
            std::lock_guard<std::mutex> lk(idmu_);
            issuer_hash = idemix_issuer_hash_;
        }
        const bool any_nym = !out.tuple_nym_issuer.empty();
        auto issuer_of = [&](size_t i) -> const uint8_t* {
            if (!any_nym || out.tuple_nym_issuer[i] < 0) return nullptr;
            auto it = issuer_hash.find(out.tuple_nym_issuer[i]);
            return it == issuer_hash.end() ? nullptr : it->second.data();
        };
        auto wanted = [&](size_t i) {
            if (any_nym && out.tuple_nym_issuer[i] >= 0 && !issuer_of(i)) return false;
            return out.tuple_hashed[i] && out.tuple_status[i] <= FABGPU_ST_RANGE && pb.tuples[i].sig.len != 0 && pb.tuples[i].sig.len <= 1024;
        };
        // Two phases on the pass's workers, like the gates: count (entries, key bytes) per range, meet, then every worker writes its
        // entries - index, framed key, status - and inserts them into the block's table.  (Selecting and sizing on one thread first cost
        // 0.3 ms of the 0.6 ms this stage took for a 40 000-tuple block.)
        std::vector<uint32_t>& sel = sel_scratch;          // reuse: indices of the tuples that get an entry
        if (sel.size() < nt) sel.resize(nt);
        const int ft = nt >= 8192 ? std::min(gate_max, 16) : 1;
        std::vector<uint32_t> cnt_e(ft + 1, 0), cnt_b(ft + 1, 0);
        std::atomic<int> met(0), cleared(0);
        // (the workers meet at spin barriers; one that cannot go on - worker 0 allocates between two of them - raises `aborted`, which
        // every barrier watches: nobody spins for a worker that is gone, the block simply gets no memo entries)
        std::atomic<bool> aborted(false);
        BlockMemo* raw = bm.get();
        uint32_t m = 0;
        bool too_big = false;
        auto work_body = [&](int w) {
            const size_t lo = nt * w / ft, hi = nt * (w + 1) / ft;
            uint32_t ce = 0, cb = 0;
            for (size_t i = lo; i < hi; i++)
                if (wanted(i)) {
                    ce++;
                    cb += (uint32_t)MemoKeyBytes(pb.tuples[i].sig.len, 32, issuer_of(i) != nullptr);
                }
            cnt_e[w + 1] = ce;
            cnt_b[w + 1] = cb;
            met.fetch_add(1, std::memory_order_acq_rel);
            while (met.load(std::memory_order_acquire) < ft && !aborted.load(std::memory_order_acquire)) std::this_thread::yield();
            if (aborted.load(std::memory_order_acquire)) return;
            if (w == 0) {                                  // sizes are known: worker 0 makes room, the others wait for it
                uint64_t tm = 0, tb = 0;
                for (int v = 0; v < ft; v++) {
                    tm += cnt_e[v + 1];
                    tb += cnt_b[v + 1];
                }
                m = (uint32_t)tm;
                too_big = tb > 0xFFFFFFF0ull;
                if (m && !too_big) {
                    uint32_t cap = 16;
                    while (cap < 2 * m) cap <<= 1;
                    raw->mask = cap - 1;
                    if (raw->slots_cap < cap) {
                        raw->slots.reset(new std::atomic<uint32_t>[cap]);
                        raw->slots_cap = cap;
                    }
                    if (raw->keys_cap < tb) {
                        raw->keys_cap = (size_t)tb + (size_t)tb / 8;
                        raw->keys.reset(new uint8_t[raw->keys_cap]);
                    }
                    raw->key_off.resize((size_t)m + 1);
                    raw->key_off[m] = (uint32_t)tb;
                    raw->status.resize(m);
                }
                cleared.store(1, std::memory_order_release);
            }
            while (cleared.load(std::memory_order_acquire) < 1 && !aborted.load(std::memory_order_acquire)) std::this_thread::yield();
            if (aborted.load(std::memory_order_acquire) || !m || too_big) return;
            // every worker clears its share of the table, then all meet again before anybody inserts
            const size_t cap = (size_t)raw->mask + 1;
            for (size_t k = cap * w / ft; k < cap * (w + 1) / ft; k++) raw->slots[k].store(0, std::memory_order_relaxed);
            cleared.fetch_add(1, std::memory_order_acq_rel);
            while (cleared.load(std::memory_order_acquire) < 1 + ft && !aborted.load(std::memory_order_acquire)) std::this_thread::yield();
            if (aborted.load(std::memory_order_acquire)) return;
            uint32_t e = 0, off = 0;
            for (int v = 0; v < w; v++) {
                e += cnt_e[v + 1];
                off += cnt_b[v + 1];
            }
            for (size_t i = lo; i < hi; i++) {
                if (!wanted(i)) continue;
                const BlockTuple& tp = pb.tuples[i];
                const uint8_t* sg = block + tp.sig.off;
                sel[e] = (uint32_t)i;
                raw->key_off[e] = off;
                const uint8_t* issuer = issuer_of(i);
                MemoKeyWrite(raw->keys.get() + off, issuer, &out.tuple_qxy[64 * i], &out.tuple_qxy[64 * i + 32], sg, tp.sig.len, &out.tuple_digest[32 * i], 32);
                raw->status[e] = out.tuple_status[i];
                uint32_t at = (uint32_t)MemoHash(sg, tp.sig.len, &out.tuple_digest[32 * i], 32) & raw->mask;
                for (;;) {                                 // lock-free linear probing: the table is at most half full
                    uint32_t expect = 0;
                    if (raw->slots[at].compare_exchange_strong(expect, e + 1, std::memory_order_release, std::memory_order_relaxed)) break;
                    at = (at + 1) & raw->mask;
                }
                off += (uint32_t)MemoKeyBytes(tp.sig.len, 32, issuer != nullptr);
                e++;
            }
        };
        auto work = [&](int w) {
            try {
                work_body(w);
            } catch (...) {                                // bad_alloc: no entries for this block, never a stuck pool or a terminate()
                aborted.store(true, std::memory_order_release);
            }
        };
        if (ft == 1) work(0);
        else run_workers(ft, work);                       // all ft run at once (they meet at spin barriers): worker_pool.h
        if (too_big || aborted.load()) m = 0;
        bm->n = m;
        out.memo_seeded = m;
        if (m) {
            static_assert(sizeof(std::atomic<uint32_t>) == sizeof(uint32_t), "the slot table is read as plain words once it is published");
            bm->slots_v = reinterpret_cast<const uint32_t*>(bm->slots.get());
            bm->key_off_v = bm->key_off.data();
            bm->keys_v = bm->keys.get();
            bm->status_v = bm->status.data();
            bm->digests_v = nullptr;
            bm->n_entries = m;
            // The digest memo's index, the host's version of walk_memo_index_kernel: when the block's upload left a host copy of it
            // (BlockUpload::copy), every entry's message spans and a slot found from walk::msg_fingerprint of the message as it lies in
            // that copy.  Without a copy the table answers bccsp.Verify only.
            bm->hslots_v = bm->hspans_v = nullptr;
            if (up) (void)up->join();                      // (usually long joined: the submission waited for it)
            if (up && up->copy.p && HashMemoEnabled()) {
                try {
                    const size_t cap = (size_t)bm->mask + 1;
                    bm->hslots.assign(cap, 0u);
                    bm->hspans.assign((size_t)m * 4, 0u);
                    const uint8_t* cp = up->copy.p;
                    const size_t cl = up->copy.len;
                    const uint32_t tb = pb.tail_base;
                    auto resolve = [&](uint32_t off, uint32_t l) -> const uint8_t* {
                        if ((uint64_t)off + l <= cl) return cp + off;
                        if (tb && off >= tb && (uint64_t)(off - tb) + l <= pb.tail.size()) return pb.tail.data() + (off - tb);
                        return nullptr;
                    };
                    uint32_t* hs = bm->hslots.data();
                    uint32_t* sp = bm->hspans.data();
                    const uint32_t mask = bm->mask;
                    auto index_some = [&](int w) {
                        for (size_t e = (size_t)m * w / ft; e < (size_t)m * (w + 1) / ft; e++) {
                            const BlockTuple& tp = pb.tuples[sel[e]];
                            const uint8_t* a = resolve(tp.prefix.off, tp.prefix.len);
                            const uint8_t* b = resolve(tp.suffix.off, tp.suffix.len);
                            if (!a || !b || (uint64_t)tp.prefix.len + tp.suffix.len < walk::HASH_MEMO_MIN_LEN) continue;   // (spans stay zero: no lookup matches)
                            sp[4 * e] = tp.prefix.off; sp[4 * e + 1] = tp.prefix.len; sp[4 * e + 2] = tp.suffix.off; sp[4 * e + 3] = tp.suffix.len;
                            uint32_t at = (uint32_t)walk::msg_fingerprint(a, tp.prefix.len, b, tp.suffix.len) & mask;
                            for (;;) {
                                uint32_t expect = 0;
                                if (__atomic_compare_exchange_n(&hs[at], &expect, (uint32_t)e + 1, false, __ATOMIC_RELEASE, __ATOMIC_RELAXED)) break;
                                at = (at + 1) & mask;
                            }
                        }
                    };
                    if (ft == 1) index_some(0);
                    else run_workers(ft, index_some);
                    bm->hslots_v = bm->hslots.data();
                    bm->hspans_v = bm->hspans.data();
                } catch (...) {                            // bad_alloc: the verdict memo stands, the digest memo does not
                    bm->hslots_v = bm->hspans_v = nullptr;
                }
            }
            MemoAdoptCopy(*bm, up, pb.tail.data(), pb.tail.size(), pb.tail_base);
            if (!PublishMemo(bm)) out.memo_seeded = 0;
        }
    }
}
bool GPUCSP::PublishMemo(const std::shared_ptr<BlockMemo>& bm) const {
    bm->gen = g_memo_gen.fetch_add(1, std::memory_order_relaxed);     // (a recycled table is a new table to every thread's hint)
    std::unique_lock<BigReaderLock> lk(memo_mu_);
    if (poisoned_.load(std::memory_order_acquire)) {                   // a pass that was in flight when the audit failed: it seeds nothing
        bm->ReleaseCopy();
        return false;
    }
    memo_blocks_.push_back(bm);
    size_t total = 0;
    for (const auto& b : memo_blocks_) total += b->n;
    while (total > memo_cap_ && memo_blocks_.size() > 1) {        // bounded: the oldest block goes first
        total -= memo_blocks_.front()->n;
        memo_evicted_.fetch_add(memo_blocks_.front()->n, std::memory_order_relaxed);
        memo_blocks_.front()->ReleaseCopy();
        if (memo_free_.size() < memo_free_max_) memo_free_.push_back(memo_blocks_.front());
        memo_blocks_.pop_front();
    }
    return true;
}
std::shared_ptr<GPUCSP::BlockMemo> GPUCSP::TakeMemoTable(bool prefer_pinned) const {
    std::shared_ptr<BlockMemo> bm;
    {
        std::unique_lock<BigReaderLock> lk(memo_mu_);
        if (prefer_pinned)
            for (auto it = memo_free_.begin(); it != memo_free_.end(); ++it)
                if ((*it)->pin) {
                    bm = *it;
                    memo_free_.erase(it);
                    break;
                }
        if (!bm && !memo_free_.empty()) {
            bm = memo_free_.back();
            memo_free_.pop_back();
        }
    }
    if (!bm) bm.reset(new BlockMemo);
    return bm;
}
GPUCSP::MemoReturn::~MemoReturn() {
    if (!bm) return;
    std::unique_lock<BigReaderLock> lk(c->memo_mu_);
    if (c->memo_free_.size() < c->memo_free_max_) c->memo_free_.push_back(bm);
}
void GPUCSP::MemoAdoptCopy(BlockMemo& bm, BlockUpload* up, const uint8_t* tail, size_t tail_len, uint32_t tail_base) {
    host_copy_release(&bm.copy);
    bm.tail.clear();
    bm.tail_base = 0;
    if (!bm.hslots_v || !bm.hspans_v || !up || !up->copy.p) {
        bm.hslots_v = bm.hspans_v = nullptr;
        return;
    }
    bm.copy = up->copy;
    up->copy = HostCopy();
    if (!tail || !tail_len) return;
    try {
        bm.tail.assign(tail, tail + tail_len);
        bm.tail_base = tail_base;
    } catch (...) {                                        // bad_alloc: the verdict memo stands, the digest memo does not
        bm.hslots_v = bm.hspans_v = nullptr;
    }
}

// ---- the pass with the walk on the device (block_walk_dev.h) ----------------------------------------------------------------
bool GPUCSP::DeviceWalkEnabled() const {
    std::lock_guard<std::mutex> lk(opt_mu_);
    return opts_.pass_device_walk >= 0;
}

uint64_t GPUCSP::MakeSeed() {
    std::random_device rd;
    return ((uint64_t)rd() << 32) ^ (uint64_t)rd() ^ (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
}

// the provider's identity cache as the device sees it: every cached identity, most recently used first
int GPUCSP::SyncDeviceIdentityTable(Dev& dv) const {
    std::atomic<uint64_t>& idtab_version_ = dv.idtab_version;
    std::vector<uint64_t>& idtab_host_ = dv.idtab_host;
    if (idtab_version_ == id_version_.load(std::memory_order_acquire)) return FABGPU_OK;
    std::unique_lock<std::shared_timed_mutex> wl(dv.idtab_rw);
    std::vector<DevIdEntry>& ents = dv.idtab_ents;
    std::vector<uint8_t>& bytes = dv.idtab_bytes;
    uint64_t ver;
    {
        // (a provider that meets new clients in every block rebuilds this before every pass: hashes are cached per entry, nothing is
        // allocated per entry, the byte arena is reused - 1.0 -> 0.3 ms for a full cache of 4 096 certificates)
        std::lock_guard<std::mutex> lk(idmu_);
        ver = id_version_.load(std::memory_order_acquire);
        if (idtab_version_ == ver) return FABGPU_OK;
        idtab_host_.clear();
        ents.clear();
        size_t total = 0;
        for (const auto& kv : idlru_) total += (kv.first.size() + 3) & ~(size_t)3;
        bytes.resize(total);
        size_t at = 0;
        for (const auto& kv : idlru_) {
            DevIdEntry e;
            memset(&e, 0, sizeof(e));
            e.hash = kv.second.table_hash;
            e.off = (uint32_t)at;                                           // dword-aligned: the device compares a dword per lane
            e.len = (uint32_t)kv.first.size();
            e.key_id = kv.second.key_id >= 0 ? (int32_t)kv.second.key_id : -1;
            e.p256 = kv.second.p256 ? 1 : 0;
            if (kv.second.p256) {
                memcpy(e.qx, kv.second.qx, 32);
                memcpy(e.qy, kv.second.qy, 32);
            }
            memcpy(bytes.data() + at, kv.first.data(), kv.first.size());
            at += (kv.first.size() + 3) & ~(size_t)3;
            ents.push_back(e);
            idtab_host_.push_back(kv.second.serial);
        }
    }
    int rc = walk_idtab_set(dv.ctx, (uint32_t)ents.size(), ents.data(), bytes.data(), bytes.size(), idtab_seed_);
    if (rc != FABGPU_OK) return rc;
    idtab_version_ = ver;
    return FABGPU_OK;
}

int GPUCSP::WalkBlockOnDevice(const uint8_t* block, size_t len, ParsedBlock& pb, const char** why) const {
    static const char* none = "";
    const char* dummy;
    if (!why) why = &dummy;
    *why = none;
    if (!block || len == 0) return FABGPU_EINVAL;
    std::vector<uint32_t> env_spans;
    std::vector<BlockTuple> block_sigs;
    if (!OutlineBlock(block, len, pb, env_spans, block_sigs)) return FABGPU_EINVAL;
    uint64_t tok = 0;
    fabgpu_ctx* const ctx_ = devs_[0]->ctx;                 // (a test hook: the first device)
    int rc = fabgpu_arena_stage(ctx_, block, len, &tok);
    if (rc != FABGPU_OK) return rc;
    struct Sizer {
        ParsedBlock& pb;
    } sz{pb};
    WalkRequest rq;
    rq.stage_token = tok;
    rq.block_len = len;
    rq.env_spans = env_spans.data();
    rq.n_env = (uint32_t)(env_spans.size() / 2);
    rq.block_sigs = block_sigs.data();
    rq.n_block_sigs = (uint32_t)block_sigs.size();
    if (!block_sigs.empty()) {
        rq.tail = pb.tail.data();
        rq.tail_base = pb.tail_base;
        rq.tail_len = (uint32_t)pb.tail.size();
    }
    rq.walk_only = true;
    rq.user = &sz;
    rq.sizes = [](void* user, const WalkCounts& c, WalkOut& o) {
        ParsedBlock& p = ((Sizer*)user)->pb;
        p.tx_type.resize(c.n_tx);
        p.tx_understood.resize(c.n_tx);
        p.tuples.resize(c.n_tuples);
        p.prefixes.resize(c.n_prefixes);
        p.hash_checks.resize(c.n_checks);
        o.tx_type = p.tx_type.data();
        o.tx_understood = p.tx_understood.data();
        o.tuples = p.tuples.data();
        o.prefixes = p.prefixes.data();
        o.checks = p.hash_checks.data();
        return true;
    };
    rc = walk_block_pass(ctx_, rq);
    if (rc == WALK_DECLINED) {
        *why = rq.declined_why;
        return 1;
    }
    return rc;
}

// What the steps of one device-route pass share; WalkRequest::user of its two callbacks.
struct GPUCSP::DevicePass {
    const uint8_t* block;
    size_t len;
    ParsedBlock& pb;
    BlockVerdicts& out;
    PassScratch& ps;
    BlockUpload& up;
    const PassOptions& opt;
    Dev& dv;
    const std::vector<DevIdemixMsp>& msps;
    bool want_tuples, want_digests, want_qxy, want_nym_issuer, host_counts;
    uint32_t cap_tx, cap_tuples, n_skipped;
    std::vector<uint8_t> issuer_hashes;   // 32 bytes per entry of msps, for the device-built memo
    uint32_t n_tuples = 0;
    bool too_big = false;
    // the memo the device fills: a table out of the free list (its pinned room is reused), sized once the tuple count is known
    BlockMemo* bm = nullptr;
    bool hash_index = false;              // the upload left a host copy of the block: the device builds the digest memo's index too
    std::vector<std::string> to_register;
    std::vector<uint64_t> hit_serials;    // who this block named: they stay in front of the block's newcomers
};

// the idemix MSPs whose creators the pass verifies (an MSP id registered with two different issuer keys is not among them: its
// creators stay with bccsp/idemix, as on the host route)
bool GPUCSP::ListIdemixMsps(std::vector<DevIdemixMsp>& msps) const {
    std::lock_guard<std::mutex> lk(idmu_);
    for (const auto& kv : idemix_msps_) {
        if (kv.second < 0) continue;
        if (kv.first.size() > WALK_IDEMIX_MSPID_MAX || msps.size() >= WALK_IDEMIX_MSPS_MAX) return false;
        DevIdemixMsp m;
        memset(&m, 0, sizeof(m));
        m.len = (uint32_t)kv.first.size();
        m.issuer = (int32_t)kv.second;
        memcpy(m.id, kv.first.data(), kv.first.size());
        msps.push_back(m);
    }
    return true;
}

// OPTIONAL (FABGPU_PASS_HOST_COUNTS=1; off by default): while the block is on its way up, the per-envelope counts the device walk
// starts from (tuples, prefixes, hash checks, gathered bytes - walk::walk_envelope with the counting emitter, the code
// walk_count_kernel runs) taken here, on a few threads; the device then needs neither that kernel, nor the scan behind it, nor the
// wait for the totals in between.  Measured (round 3, 10 000 tx, tools/host_walk_probe.cpp + tools/gpu_probe_sizes.sh): the device
// phase drops 0.92 -> 0.85 ms, but the host's walk is a chain of DRAM misses per envelope - 8.2 ms on one thread, 1.2-1.7 ms on
// 8-12, about the whole upload - against 0.10 ms for the count kernel: 4 % off the pass for 8 ms of the peer's CPU per block.
// Not a trade a peer wants by default; the entry stays for hosts with idle cores (and as the second source the emit kernel's
// count check is tested against).
void GPUCSP::CountEnvelopesOnHost(DevicePass& dp) {
    PassScratch& ps = dp.ps;
    const uint8_t* const block = dp.block;
    const size_t len = dp.len;
    const uint32_t n_env = (uint32_t)(ps.env_spans.size() / 2);
    ps.env_counts.resize(4 * (size_t)n_env);
    ps.env_type.resize(n_env);
    ps.env_understood.resize(n_env);
    std::atomic<uint32_t> next(0);
    auto count_some = [&](int) {
        for (;;) {
            const uint32_t lo = next.fetch_add(64, std::memory_order_relaxed);
            if (lo >= n_env) return;
            const uint32_t hi = std::min(n_env, lo + 64);
            for (uint32_t e = lo; e < hi; e++) {
                uint32_t off = ps.env_spans[2 * (size_t)e], elen = ps.env_spans[2 * (size_t)e + 1];
                if (off > len || elen > len - off) off = elen = 0;
                walk::CountEmitter em;
                uint8_t type = 255, understood = 0;
                walk::walk_envelope(block, block + off, elen, e, em, type, understood);
                uint32_t* c = &ps.env_counts[4 * (size_t)e];
                c[0] = em.nt; c[1] = em.np; c[2] = em.nc;
                c[3] = em.gb > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)em.gb;
                ps.env_type[e] = type;
                ps.env_understood[e] = understood;
            }
        }
    };
    const int nth = n_env >= 2048 ? std::min(WalkThreads(), 8) : 1;
    if (nth == 1) count_some(0);
    else run_workers(nth, count_some);
}

bool GPUCSP::WalkSizes(void* device_pass, const WalkCounts& c, WalkOut& o) {
    DevicePass& z = *(DevicePass*)device_pass;
    const size_t nt = (size_t)c.n_tuples + z.n_skipped;
    z.n_tuples = (uint32_t)nt;
    if (c.n_tx > z.cap_tx || nt > z.cap_tuples) {
        z.too_big = true;
        return false;
    }
    z.out.tx_flags.resize(c.n_tx);
    z.out.tx_type.resize(c.n_tx);
    z.pb.tx_type.resize(c.n_tx);
    z.pb.tx_understood.resize(c.n_tx);
    z.out.tuple_status.resize(nt);
    z.out.tuple_hashed.resize(nt);
    o.tx_flags = z.out.tx_flags.data();
    o.tx_type = z.out.tx_type.data();
    o.tx_understood = z.pb.tx_understood.data();
    o.tuple_status = z.out.tuple_status.data();
    o.tuple_hashed = z.out.tuple_hashed.data();
    z.ps.id_idx.resize(nt);                                          // (4 bytes per tuple: who was named, for the cache's bookkeeping)
    o.id_idx = z.ps.id_idx.data();
    if (z.want_tuples) {
        z.pb.tuples.resize(nt);
        o.tuples = z.pb.tuples.data();
    }
    if (z.want_digests) {
        z.out.tuple_digest.resize(nt * 32);
        o.tuple_digest = z.out.tuple_digest.data();
    } else {
        z.out.tuple_digest.clear();
    }
    if (z.want_nym_issuer) {                                         // which issuer an idemix creator's row was verified under (memo binding)
        z.ps.nym_issuer_rank.resize(c.n_creators);
        o.nym_issuer = z.ps.nym_issuer_rank.data();
    }
    if (z.want_qxy) {                                                // the key of every tuple's identity, as the device matched or decoded it
        z.out.tuple_qxy.resize(nt * 64);
        o.tuple_qxy = z.out.tuple_qxy.data();
    } else {
        z.out.tuple_qxy.clear();
    }
    if (z.bm && c.n_tuples) {
        // room for the memo (MemoPinLayout)
        uint32_t cap = 0;
        size_t keys_cap = 0, total = 0, at[7];
        MemoPinLayout(c.n_tuples, c.n_creators, &cap, &keys_cap, &total, at);
        const size_t a_slots = at[0], a_off = at[1], a_st = at[2], a_dig = at[3], a_keys = at[4], a_hslots = at[5], a_hspans = at[6];
        if (cap >= 2 * (uint64_t)c.n_tuples && keys_cap < 0xFFFFFFF0ull) {
            if (z.bm->pin_cap < total) {
                if (z.bm->pin) walk_pinned_free(z.bm->pin_ctx, z.bm->pin);
                z.bm->pin = walk_pinned_alloc(z.dv.ctx, total + total / 4);
                z.bm->pin_ctx = z.dv.ctx;
                z.bm->pin_cap = z.bm->pin ? total + total / 4 : 0;
            }
            if (z.bm->pin) {
                uint8_t* p = (uint8_t*)z.bm->pin;
                o.memo_slots = (uint32_t*)(p + a_slots);
                o.memo_slot_cap = cap;
                o.memo_key_off = (uint32_t*)(p + a_off);
                o.memo_status = p + a_st;
                o.memo_digests = p + a_dig;
                o.memo_keys = p + a_keys;
                o.memo_keys_cap = keys_cap;
                z.bm->mask = cap - 1;
                z.bm->slots_v = o.memo_slots;
                z.bm->key_off_v = o.memo_key_off;
                z.bm->status_v = o.memo_status;
                z.bm->digests_v = o.memo_digests;
                z.bm->keys_v = o.memo_keys;
                z.bm->hslots_v = z.bm->hspans_v = nullptr;
                if (z.hash_index) {
                    o.memo_hslots = (uint32_t*)(p + a_hslots);
                    o.memo_hspans = (uint32_t*)(p + a_hspans);
                    z.bm->hslots_v = o.memo_hslots;
                    z.bm->hspans_v = o.memo_hspans;
                }
            }
        }
    }
    return true;
}
uint8_t* GPUCSP::WalkMemoGrow(void* device_pass, size_t bytes) {
    DevicePass& z = *(DevicePass*)device_pass;
    if (!z.bm || bytes >= 0xFFFFFFF0ull) return nullptr;
    if (z.bm->pin_keys_cap < bytes) {
        if (z.bm->pin_keys) walk_pinned_free(z.bm->pin_ctx, z.bm->pin_keys);
        z.bm->pin_keys = walk_pinned_alloc(z.dv.ctx, bytes + bytes / 4);
        z.bm->pin_ctx = z.dv.ctx;
        z.bm->pin_keys_cap = z.bm->pin_keys ? bytes + bytes / 4 : 0;
    }
    if (!z.bm->pin_keys) return nullptr;
    z.bm->keys_v = (const uint8_t*)z.bm->pin_keys;
    return (uint8_t*)z.bm->pin_keys;
}

void GPUCSP::BuildWalkRequest(DevicePass& dp, WalkRequest& rq, uint64_t stage_token) const {
    PassScratch& ps = dp.ps;
    rq.stage_token = stage_token;
    rq.block_len = dp.len;
    rq.env_spans = ps.env_spans.data();
    rq.payload_spans = ps.payload_spans.data();
    rq.n_env = (uint32_t)(ps.env_spans.size() / 2);
    if (dp.host_counts && rq.n_env) {
        rq.host_counts = ps.env_counts.data();
        rq.host_tx_type = ps.env_type.data();
        rq.host_tx_understood = ps.env_understood.data();
    }
    if (dp.opt.block_sigs && !ps.block_sigs.empty()) {
        rq.block_sigs = ps.block_sigs.data();
        rq.n_block_sigs = (uint32_t)ps.block_sigs.size();
        rq.tail = dp.pb.tail.data();
        rq.tail_base = dp.pb.tail_base;
        rq.tail_len = (uint32_t)dp.pb.tail.size();
    }
    rq.user = &dp;
    rq.sizes = &GPUCSP::WalkSizes;
    rq.memo_grow = &GPUCSP::WalkMemoGrow;
    ps.learn.resize(WALK_LEARN_SLOTS);
    rq.learn_out = ps.learn.data();
    rq.idemix_msps = dp.msps.data();
    rq.n_idemix_msps = (uint32_t)dp.msps.size();
    // (a pseudonym signature's memo entry is bound to the hash of the issuer key it was verified under: without every MSP's hash at hand
    //  the device makes no entries for pseudonym signatures at all)
    if (dp.bm && !dp.msps.empty()) {
        std::lock_guard<std::mutex> lk(idmu_);
        dp.issuer_hashes.resize(32 * dp.msps.size());
        bool all = true;
        for (size_t m = 0; m < dp.msps.size(); m++) {
            auto it = idemix_issuer_hash_.find(dp.msps[m].issuer);
            if (it == idemix_issuer_hash_.end()) all = false;
            else memcpy(&dp.issuer_hashes[32 * m], it->second.data(), 32);
        }
        if (all) rq.idemix_issuer_hashes = dp.issuer_hashes.data();
    }
}

// the answers as the host route reports them: the issuer of every pseudonym signature, the skipped block signatures, tuple_tx / _kind
void GPUCSP::FinishDeviceAnswers(DevicePass& dp, const WalkRequest& rq) {
    ParsedBlock& pb = dp.pb;
    BlockVerdicts& out = dp.out;
    PassScratch& ps = dp.ps;
    const bool want_tuples = dp.want_tuples, want_digests = dp.want_digests, want_qxy = dp.want_qxy;
    const size_t nt = dp.n_tuples, nd = nt - dp.n_skipped;
    out.n_tx = pb.n_tx;
    memcpy(pb.tx_type.data(), out.tx_type.data(), pb.n_tx);
    out.distinct_identities = 0;
    out.ms_nym = out.ms_memo = 0;
    out.memo_seeded = 0;
    out.n_block_sigs = pb.n_block_sigs;
    out.block_sigs_understood = pb.block_sigs_understood ? 1 : 0;
    // tuples that went through registered comb tables, by launch class (the status kernel counted what each class decided)
    out.n_keyed = (rq.keyed_creators ? rq.summary.n_hashed_creator : 0u) + (rq.keyed_others ? rq.summary.n_hashed_other : 0u);
    out.n_device_decoded = rq.summary.n_unknown_identity;
    out.tuple_nym_issuer.clear();
    if (dp.want_nym_issuer && rq.summary.n_nym != 0 && want_tuples) {
        // the memo binds a pseudonym signature's entry to the issuer it was verified under: issuer ids come back by creator rank, and
        // creator tuples appear in rank order (every tuple-yielding envelope yields exactly one, its first)
        out.tuple_nym_issuer.assign(nt, -1);
        size_t rank = 0;
        for (size_t i = 0; i < nd; i++)
            if (pb.tuples[i].kind == TUPLE_CREATOR) {
                if (rank < ps.nym_issuer_rank.size()) out.tuple_nym_issuer[i] = ps.nym_issuer_rank[rank];
                rank++;
            }
    }
    for (size_t i = nd; i < nt; i++) {                                   // block signatures the caller asked not to verify
        out.tuple_status[i] = TUPLE_ST_SKIPPED;
        out.tuple_hashed[i] = 0;
        ps.id_idx[i] = 0xFFFFFFFFu;
        if (want_tuples) pb.tuples[i] = ps.block_sigs[i - nd];
        if (want_digests) memset(&out.tuple_digest[32 * i], 0, 32);
    }
    if (want_tuples) {
        out.tuple_tx.resize(nt);
        out.tuple_kind.resize(nt);
        for (size_t i = 0; i < nt; i++) {
            out.tuple_tx[i] = pb.tuples[i].tx;
            out.tuple_kind[i] = pb.tuples[i].kind;
        }
    } else {
        out.tuple_tx.clear();
        out.tuple_kind.clear();
    }
    if (want_qxy)
        for (size_t i = nd; i < nt; i++) memset(&out.tuple_qxy[64 * i], 0, 64);   // (skipped block signatures: as the host pass reports them)
    if (want_digests)
        for (size_t i = 0; i < nt; i++)
            if (!out.tuple_hashed[i]) memset(&out.tuple_digest[32 * i], 0, 32);   // as the host pass reports them
}

// What the host pass does per tuple for the cache - count who was named (a device comb table is earned by being named
// id_register_after_ times) and keep the LRU order fresh - from the identity indices, when they came back.
void GPUCSP::CountDeviceHits(DevicePass& dp) const {
    const std::vector<uint64_t>& idtab_host_ = dp.dv.idtab_host;
    if (idtab_host_.empty()) return;
    const size_t nd = dp.n_tuples - dp.n_skipped;
    std::vector<uint32_t> hits(idtab_host_.size(), 0);
    for (size_t i = 0; i < nd; i++)
        if (dp.ps.id_idx[i] < hits.size()) hits[dp.ps.id_idx[i]]++;
    std::lock_guard<std::mutex> lk(idmu_);
    for (size_t k = 0; k < hits.size(); k++) {
        if (!hits[k]) continue;
        auto it = idserial_.find(idtab_host_[k]);
        if (it == idserial_.end()) continue;                        // (evicted since the table was made)
        dp.hit_serials.push_back(idtab_host_[k]);
        idlru_.splice(idlru_.begin(), idlru_, it->second);
        CachedIdentity& c = it->second->second;
        c.hits += hits[k];
        if (EarnTableLocked(c)) dp.to_register.push_back(it->second->first);
    }
}

// Identities the device decoded itself (nobody had met them) enter the cache here, with the key the device read out of the
// certificate - the host route's "new identity" branch without decoding anything again.  At most WALK_LEARN_SLOTS per block; the
// LRU bounds what unvalidated blocks can make the provider remember, and a comb table is still only earned by being named often.
void GPUCSP::LearnDeviceIdentities(DevicePass& dp, const WalkRequest& rq) const {
    if (!rq.summary.n_learn) return;
    std::lock_guard<std::mutex> lk(idmu_);
    bool grew = false;
    for (const WalkLearn& l : dp.ps.learn) {
        if (!l.tag || !l.ready || (uint64_t)l.off + l.len > dp.len) continue;
        std::string key((const char*)dp.block + l.off, l.len);
        if (idcache_.find(key) != idcache_.end()) continue;
        CachedIdentity ci;
        ci.p256 = l.ready == 1;
        memcpy(ci.qx, l.qx, 32);
        memcpy(ci.qy, l.qy, 32);
        ci.hits = l.hits ? l.hits : 1;
        if (EarnTableLocked(ci)) dp.to_register.push_back(key);
        InsertIdentityLocked(std::move(key), ci, /*evict_now=*/false);
        pass_learned_.fetch_add(1, std::memory_order_relaxed);
        grew = true;
    }
    // The block's newcomers must not push out the identities the same block NAMED: with open-addressed learn slots a block can bring
    // 128 of them, and a cache bound below that (tests; an operator's choice) would otherwise drop the channel's endorsers - named
    // by every transaction, tables and all - because they were touched a moment BEFORE the newcomers were inserted in front of them.
    if (!grew) return;
    for (uint64_t serial : dp.hit_serials) {
        auto it = idserial_.find(serial);
        if (it != idserial_.end()) idlru_.splice(idlru_.begin(), idlru_, it->second);
    }
    EvictIdentitiesLocked();
    id_version_.fetch_add(1, std::memory_order_release);
}

void GPUCSP::PublishDeviceMemo(DevicePass& dp, const WalkRequest& rq, std::shared_ptr<BlockMemo>& bm) const {
    StageClock memo_clock{dp.out.ms_memo};
    bm->seq = dp.opt.block_seq;
    bm->n = rq.memo_live;
    bm->n_entries = rq.memo_n;
    dp.out.memo_seeded = rq.memo_live;
    MemoAdoptCopy(*bm, &dp.up, rq.tail, rq.tail_len, rq.tail_base);
    if (!PublishMemo(bm)) dp.out.memo_seeded = 0;
    bm.reset();                                                        // (published: not for the free list)
}

int GPUCSP::PreVerifyBlockOnDevice(const uint8_t* block, size_t len, ParsedBlock& pb, BlockVerdicts& out, BlockUpload& up, const PassOptions& opt,
                                   unsigned want, uint32_t cap_tx, uint32_t cap_tuples, uint32_t* n_tuples_out, const char** why) const {
    static const char* none = "";
    const char* dummy;
    if (!why) why = &dummy;
    *why = none;
    auto declined = [&](const char* w) {
        *why = w;
        return 1;
    };
    if (!DeviceWalkEnabled()) return declined("pass_device_walk is off");
    if (!block || !up.started) return declined("the block was not staged ahead (small block)");
    ProviderOptions po;
    {
        std::lock_guard<std::mutex> lk(opt_mu_);
        po = opts_;
    }
    if (po.pass_skip_hash_checks > 0) return declined("pass_skip_hash_checks");
    Dev& dv = *devs_[(size_t)up.dev];                       // the device the block travelled to (StartBlockUpload chose it)
    fabgpu_ctx* const ctx_ = dv.ctx;
    std::atomic<uint64_t>& idtab_version_ = dv.idtab_version;
    std::vector<DevIdemixMsp> msps;
    if (!ListIdemixMsps(msps)) return declined("more idemix MSPs (or a longer MSP id) than the device route carries");
    ScratchLease lease(this);
    PassScratch& ps = *lease.p;
    auto clk0 = std::chrono::steady_clock::now();
    if (!OutlineBlock(block, len, pb, ps.env_spans, ps.block_sigs, &ps.payload_spans)) return FABGPU_EINVAL;
    // The caller's room for per-transaction answers is checked HERE - the outline knows the transaction count - before the upload is
    // waited for and before anything is launched: a too-small array costs the caller the outline (0.15 ms for 10 000 transactions),
    // not an upload and two kernels (the Go binding used to pay exactly that for every block over 1 024 transactions).
    if (ps.env_spans.size() / 2 > cap_tx) {
        pb.n_tx = (uint32_t)(ps.env_spans.size() / 2);
        if (n_tuples_out) *n_tuples_out = 0;                // (not known yet: the device counts tuples)
        return FABGPU_ETOOBIG;
    }
    // The verdict memo of a device-route pass is built by the device (round 3: block_walk_dev.h WalkOut::memo_*) into pinned memory of a
    // BlockMemo: keys, offsets, statuses and the slot table come back as they are looked up - no tuple records, digests and keys to bring
    // back, copy out and read 40 000 signatures out of the host's copy of the block for.  FABGPU_PASS_DEVICE_MEMO=0: SeedMemo, as before.
    const bool dev_memo = opt.seed_memo && po.pass_device_memo >= 0;
    const bool host_memo = opt.seed_memo && !dev_memo;
    const bool want_digests = opt.want_digests || host_memo;
    const bool want_tuples = (want & WANT_TUPLES) || host_memo, want_qxy = (want & WANT_QXY) || host_memo;
    const uint32_t n_skipped = opt.block_sigs ? 0 : (uint32_t)ps.block_sigs.size();   // reported (TUPLE_ST_SKIPPED), not submitted
    if (pb.tail.size() > opt.tail_cap) {                             // the caller wants the tail and has no room for it: say so before anything runs
        if (n_tuples_out) *n_tuples_out = 0;
        return FABGPU_ETOOBIG;
    }
    DevicePass dp{block, len, pb, out, ps, up, opt, dv, msps, want_tuples, want_digests, want_qxy, host_memo && !msps.empty(), po.pass_host_counts > 0,
                  cap_tx, cap_tuples, n_skipped};
    if (dp.host_counts && ps.env_spans.size() >= 2) CountEnvelopesOnHost(dp);   // (the option is read per pass: tests run both ways in one process)
    int rc = SyncDeviceIdentityTable(dv);
    if (rc != FABGPU_OK) return declined("the identity cache could not be copied to the device");   // (the host walk will say what is wrong, if anything is)
    std::shared_lock<std::shared_timed_mutex> rl(dv.idtab_rw);
    if (idtab_version_ != id_version_.load(std::memory_order_acquire)) return declined("the identity cache changed under the pass");
    out.ms_gates = ms_since(clk0);   // (outline + table sync)
    auto clk1 = std::chrono::steady_clock::now();
    const uint64_t tok = up.join();
    out.ms_upload_wait = ms_since(clk1);
    if (!tok) return declined("the upload failed");
    dp.hash_index = up.copy.p != nullptr && up.copy.len == len && po.pass_hash_memo >= 0;
    std::shared_ptr<BlockMemo> dev_bm;
    if (dev_memo) {
        dev_bm = TakeMemoTable(/*prefer_pinned=*/true);
        dp.bm = dev_bm.get();
    }
    WalkRequest rq;
    BuildWalkRequest(dp, rq, tok);
    MemoReturn memo_back{this, dev_bm};
    auto clk2 = std::chrono::steady_clock::now();
    rc = walk_block_pass(ctx_, rq);
    out.ms_device = ms_since(clk2);
    StageClock post_clock{out.ms_post};
    if (n_tuples_out) *n_tuples_out = dp.n_tuples;
    if (rc == WALK_DECLINED) return declined(rq.declined_why);
    if (rc == FABGPU_ETOOBIG && dp.too_big) return FABGPU_ETOOBIG;     // pb.n_tx / *n_tuples_out say what to make room for
    if (rc == FABGPU_ETOOBIG) return declined("the block exceeds the device walk's limits");   // (not the caller's arrays: the host walk takes it)
    if (rc != FABGPU_OK) return rc;
    dv.passes.fetch_add(1, std::memory_order_relaxed);
    pass_relaunches_.fetch_add(rq.relaunched, std::memory_order_relaxed);
    pass_decoded_.fetch_add(rq.summary.n_unknown_identity, std::memory_order_relaxed);
    pass_general_der_.fetch_add(rq.summary.n_general_der, std::memory_order_relaxed);
    FinishDeviceAnswers(dp, rq);
    CountDeviceHits(dp);
    rl.unlock();
    LearnDeviceIdentities(dp, rq);
    {
        const auto tq = std::chrono::steady_clock::now();
        RegisterQueued(dp.to_register);
        if (po.pass_timing > 0 && !dp.to_register.empty())
            fprintf(stderr, "fabgpu pass: %zu identities earned their comb tables: %.2f ms\n", dp.to_register.size(), ms_since(tq));
    }
    if (host_memo) SeedMemo(block, pb, out, opt, ps.sub, kGateMax, &up);
    if (dev_memo && dev_bm && rq.memo_live && dev_bm->slots_v) PublishDeviceMemo(dp, rq, dev_bm);
    return 0;
}

// What the steps of one host-route pass share.
struct GPUCSP::HostPass {
    const uint8_t* block;
    const ParsedBlock& pb;
    BlockVerdicts& out;
    BlockUpload* up;
    const PassOptions& opt;
    PassScratch& ps;
    Dev& dv;                              // the device this pass runs on
    bool want_digests, skip_hash_checks;
    size_t n = 0;                         // ECDSA tuples the gates let through, compacted into ps.sub .. ps.s
    bool all_keyed = true;                // ... every one of them under a registered comb table
    bool hashes_done = false;             // the TxID / proposal-hash digests came back in ps.hash_digests
    bool nym_rode = false;                // the idemix creators' signatures (ps.nym_idx) rode in the ECDSA submission
    std::vector<std::string> to_register; // guarded by idmu_
};

// The answer for one pseudonym signature.  status: FABGPU_NYM_VALID = 0, BAD_PROOF = 1 (= "signature invalid"), NEEDS_SW = 6 =
// TUPLE_ST_NEEDS_SW.  NymVerifier.Verify receives the whole message, not a digest (bccsp/idemix/handlers/nymsigner.go:62-95): the memo
// entry of a pseudonym signature is keyed on SHA-256(message) - digest32, computed by the device over the bytes the nym kernel verified
// (nullptr: digests are not wanted), and by the Go wrapper over the bytes it is asked about.
static void write_nym_result(BlockVerdicts& out, size_t i, uint8_t status, const uint8_t* digest32, const uint8_t* nym_x, const uint8_t* nym_y) {
    out.tuple_status[i] = status;
    if (!digest32 || status == FABGPU_NYM_NEEDS_SW) return;
    memcpy(&out.tuple_digest[32 * i], digest32, 32);
    out.tuple_hashed[i] = 1;
    memcpy(&out.tuple_qxy[64 * i], nym_x, 32);                         // the pseudonym (Nym.x, Nym.y) in the key slot
    memcpy(&out.tuple_qxy[64 * i + 32], nym_y, 32);
}

// identities -> keys (cached across blocks), signatures -> (r, s) through the reference's gates, for the tuples lo .. hi
void GPUCSP::GateRange(HostPass& hp, const std::map<std::string, int64_t>& idemix_msps, size_t lo, size_t hi, uint32_t* fresh) const {
    typedef PassScratch::Gated Gated;
    const uint8_t* const block = hp.block;
    const ParsedBlock& pb = hp.pb;
    BlockVerdicts& out = hp.out;
    const PassOptions& opt = hp.opt;
    std::vector<Gated>& gt = hp.ps.gt;
    static const uint8_t one_digest[1] = {1};
    // a block names few identities: a per-thread front cache (memcmp against the identities already met) keeps the shared
    // map - and its 700-byte key copies - off the per-tuple path
    struct Front {
        const uint8_t* p;
        uint32_t len;
        CachedIdentity ci;
        uint32_t hits;
    };
    std::vector<Front> front;
    for (size_t i = lo; i < hi; i++) {
        const BlockTuple& tp = pb.tuples[i];
        Gated& g0 = gt[i];
        g0.submit = false;
        g0.nym = false;
        out.tuple_tx[i] = tp.tx;
        out.tuple_kind[i] = tp.kind;
        memset(&out.tuple_qxy[64 * i], 0, 64);
        if (tp.kind == TUPLE_BLOCK_SIG && !opt.block_sigs) {
            out.tuple_status[i] = TUPLE_ST_SKIPPED;
            continue;
        }
        CachedIdentity ci;
        bool hit = false;
        // An idemix creator carries a fresh pseudonym per transaction: it can be in no cache, so it is recognised first - without
        // the shared map, its lock and its key copy (2 000 such creators in a block cost the gates 1.7 ms that way).  Precedence is
        // kept: an identity that also yields a P-256 certificate key takes the certificate path below.
        if (tp.kind == TUPLE_CREATOR && !idemix_msps.empty()) {
            std::string mspid;
            uint8_t tqx[32], tqy[32];
            if (IdentityToIdemixNym(block + tp.identity.off, tp.identity.len, mspid, g0.qx, g0.qy) &&
                !IdentityToP256(block + tp.identity.off, tp.identity.len, tqx, tqy)) {
                // identity.Verify is NymSignature.Ver under the MSP's issuer key (msp/idemixmsp.go:584-599); an idemix identity is
                // never an endorser (docs/source/idemix.rst:171-176)
                auto im = idemix_msps.find(mspid);
                NymSignatureFields sf;
                if (im != idemix_msps.end() && im->second >= 0 && tp.sig.len != 0 && UnmarshalNymSignature(block + tp.sig.off, tp.sig.len, sf) &&
                    sf.len[0] == 32 && sf.len[1] == 32 && sf.len[2] == 32 && sf.len[3] == 32) {
                    memcpy(g0.r, sf.f[0], 32); memcpy(g0.s, sf.f[1], 32); memcpy(g0.srn, sf.f[2], 32); memcpy(g0.nonce, sf.f[3], 32);
                    g0.key_id = im->second;
                    g0.nym = true;
                } else {
                    out.tuple_status[i] = TUPLE_ST_NEEDS_SW;
                }
                continue;
            }
        }
        for (Front& f : front)
            if (f.len == tp.identity.len && memcmp(f.p, block + tp.identity.off, f.len) == 0) {
                ci = f.ci;
                f.hits++;
                hit = true;
                break;
            }
        if (!hit) {
            bool transient = false, found = false;
            std::string key((const char*)block + tp.identity.off, tp.identity.len);
            {
                std::lock_guard<std::mutex> lk(idmu_);
                auto it = idcache_.find(key);
                if (it != idcache_.end()) {
                    idlru_.splice(idlru_.begin(), idlru_, it->second);      // most recently used
                    ci = it->second->second;
                    found = true;
                }
            }
            if (!found) {
                // decoded outside the lock (PEM + DER walk of ~800 untrusted bytes); NO device table here - that is earned
                // by being named id_register_after_ times (flush below)
                (*fresh)++;
                ci.p256 = IdentityToP256(block + tp.identity.off, tp.identity.len, ci.qx, ci.qy) && PublicKeyOnCurve(ci.qx, ci.qy);
                // idemix identities carry a fresh pseudonym per transaction: caching them would only churn the cache
                std::string ms;
                uint8_t tnx[32], tny[32];
                transient = !ci.p256 && IdentityToIdemixNym(block + tp.identity.off, tp.identity.len, ms, tnx, tny);
                if (!transient) {
                    std::lock_guard<std::mutex> lk(idmu_);
                    auto it = idcache_.find(key);
                    if (it == idcache_.end()) {
                        InsertIdentityLocked(std::string(key), ci);          // (the least recently used goes)
                        id_version_.fetch_add(1, std::memory_order_release);   // (the device's copy of the cache is stale now)
                    } else {
                        ci = it->second->second;
                    }
                }
            }
            if (!transient && front.size() < 64) front.push_back({block + tp.identity.off, tp.identity.len, ci, 1});
        }
        if (ci.p256) {
            memcpy(&out.tuple_qxy[64 * i], ci.qx, 32);
            memcpy(&out.tuple_qxy[64 * i + 32], ci.qy, 32);
        }
        if (!ci.p256) {
            out.tuple_status[i] = TUPLE_ST_NEEDS_SW;
            continue;
        }
        if (tp.sig.len == 0) {
            out.tuple_status[i] = TUPLE_ST_EMPTY_SIG;
            continue;
        }
        ECDSAPublicKey k;
        memcpy(k.x, ci.qx, 32);
        memcpy(k.y, ci.qy, 32);
        k.on_curve = true;
        const GateT<Curve256> g = gate_item<Curve256>(&k, block + tp.sig.off, tp.sig.len, one_digest, 1);
        if (!g.submit) {
            out.tuple_status[i] = gate_tuple_status(g.res);
            continue;
        }
        memcpy(g0.qx, ci.qx, 32); memcpy(g0.qy, ci.qy, 32); memcpy(g0.r, g.r, 32); memcpy(g0.s, g.s, 32);
        g0.key_id = ci.key_id;
        g0.submit = true;
    }
    // hit counts -> the shared cache; identities that have earned a device table are queued for registration
    if (!front.empty()) {
        std::lock_guard<std::mutex> lk(idmu_);
        for (const Front& f : front) {
            auto it = idcache_.find(std::string((const char*)f.p, f.len));
            if (it == idcache_.end()) continue;
            CachedIdentity& c = it->second->second;
            c.hits += f.hits;
            if (EarnTableLocked(c)) hp.to_register.push_back(it->first);
        }
    }
}

// Tuples are independent: blocks of 4096+ tuples are gated on worker threads (contiguous ranges), then compacted in order.
Error GPUCSP::GateAndCompact(HostPass& hp) const {
    typedef PassScratch::Gated Gated;
    const ParsedBlock& pb = hp.pb;
    BlockVerdicts& out = hp.out;
    PassScratch& ps_ = hp.ps;
    const size_t nt = pb.tuples.size();
    std::map<std::string, int64_t> idemix_msps;
    {
        std::lock_guard<std::mutex> lk(idmu_);
        idemix_msps = idemix_msps_;
    }
    std::vector<Gated>& gt = ps_.gt;
    if (gt.size() < nt) gt.resize(nt);
    std::vector<uint32_t> new_ids(1, 0);
    auto clk0 = std::chrono::steady_clock::now();
    const int nthreads = std::min(kGateMax, nt >= 16384 ? 16 : (nt >= 4096 ? 8 : 1));     // all of them run at once (they meet at a barrier)
    auto in_threads = [&](const std::function<void(int, size_t, size_t)>& fn) {       // fn(worker, lo, hi) over contiguous tuple ranges
        if (nthreads == 1) {
            fn(0, 0, nt);
            return;
        }
        // all nthreads run concurrently (they meet at a spin barrier): worker_pool.h keeps 15 parked threads + the caller
        run_workers(nthreads, [&](int w) { fn(w, nt * w / nthreads, nt * (w + 1) / nthreads); });
    };
    new_ids.assign(nthreads, 0);
    // ONE round of workers (spawning 16 threads costs ~0.25 ms on the bench host, and there used to be three rounds): each gates
    // its range and counts what it submits, a spin barrier lets everybody see every count, then each compacts its range - in
    // order - into the submission arrays, which are sized for the worst case up front.
    std::vector<size_t> cnt(nthreads + 1, 0);
    std::vector<uint8_t> keyed_w(nthreads, 1);
    std::vector<uint32_t>&sub = ps_.sub, &ids = ps_.ids, &off = ps_.off, &pre_idx = ps_.pre_idx;
    std::vector<uint8_t>&qx = ps_.qx, &qy = ps_.qy, &r = ps_.r, &s = ps_.s;
    // (each on its own: the device route borrows `sub` alone - SeedMemo's selection scratch - so its size says nothing about the others)
    if (sub.size() < nt) sub.resize(nt);
    if (ids.size() < nt) ids.resize(nt);
    if (off.size() < 2 * nt) off.resize(2 * nt);
    if (pre_idx.size() < nt) pre_idx.resize(nt);
    if (qx.size() < nt * 32) qx.resize(nt * 32);
    if (qy.size() < nt * 32) qy.resize(nt * 32);
    if (r.size() < nt * 32) r.resize(nt * 32);
    if (s.size() < nt * 32) s.resize(nt * 32);
    std::atomic<int> arrived(0);
    std::atomic<bool> gate_failed(false);      // a worker that threw (bad_alloc while decoding an identity): the others do not wait for it
    double ms_gates_max = 0;
    std::mutex gm;
    in_threads([&](int w, size_t lo, size_t hi) {
        try {
            GateRange(hp, idemix_msps, lo, hi, &new_ids[w]);
        } catch (...) {
            gate_failed.store(true, std::memory_order_release);
            arrived.fetch_add(1, std::memory_order_acq_rel);
            return;
        }
        size_t c = 0;
        for (size_t i = lo; i < hi; i++)
            if (gt[i].submit) {
                c++;
                if (gt[i].key_id < 0) keyed_w[w] = 0;
            }
        cnt[w + 1] = c;
        {
            double t = ms_since(clk0);
            std::lock_guard<std::mutex> lk(gm);
            if (t > ms_gates_max) ms_gates_max = t;
        }
        arrived.fetch_add(1, std::memory_order_acq_rel);
        while (arrived.load(std::memory_order_acquire) < nthreads) std::this_thread::yield();
        if (gate_failed.load(std::memory_order_acquire)) return;
        size_t j = 0;
        for (int v = 0; v < w; v++) j += cnt[v + 1];
        for (size_t i = lo; i < hi; i++) {
            const Gated& g0 = gt[i];
            if (!g0.submit) continue;
            const BlockTuple& tp = pb.tuples[i];
            sub[j] = (uint32_t)i;
            memcpy(&qx[32 * j], g0.qx, 32);
            memcpy(&qy[32 * j], g0.qy, 32);
            memcpy(&r[32 * j], g0.r, 32);
            memcpy(&s[32 * j], g0.s, 32);
            ids[j] = g0.key_id >= 0 ? (uint32_t)g0.key_id : 0;
            off[2 * j] = tp.suffix.off;
            off[2 * j + 1] = tp.suffix.off + tp.suffix.len;
            pre_idx[j] = tp.prefix_index >= 0 ? (uint32_t)tp.prefix_index : 0xFFFFFFFFu;
            j++;
        }
    });
    if (gate_failed.load()) return Error("out of memory in the signature gates");     // an infrastructure error: never a verdict
    for (uint32_t v : new_ids) out.distinct_identities += v;
    out.ms_gates = ms_gates_max;
    size_t n = 0;
    for (int w = 0; w < nthreads; w++) n += cnt[w + 1];
    hp.n = n;
    for (uint8_t k : keyed_w) hp.all_keyed = hp.all_keyed && k;
    // One identity without a device table sends the whole block down the fresh-key kernel.  Splitting such a block into a table
    // launch and a fresh-key launch was tried (round 2): submitted one after the other the two cost what the single launch costs,
    // within +-0.3 ms on a 10 000-transaction block - the fresh-key kernel is latency-bound below 32 768 tuples, so
    // taking tuples away from it does not shorten it.
    out.n_keyed = hp.all_keyed ? n : 0;
    // the block's idemix creators, in tuple order
    std::vector<uint32_t>& ns = ps_.nym_idx;
    ns.clear();
    for (size_t i = 0; i < nt; i++)
        if (gt[i].nym) ns.push_back((uint32_t)i);
    out.tuple_nym_issuer.clear();                            // (the memo binds a pseudonym signature's entry to the issuer it was verified under)
    if (!ns.empty()) {
        out.tuple_nym_issuer.assign(nt, -1);
        for (uint32_t i : ns) out.tuple_nym_issuer[i] = gt[i].key_id;
    }
    return Error();
}

// The ECDSA tuples in one fabgpu_identity_batch, the block as their message arena.  The block's idemix creators ride along
// (fabgpu_identity_batch.n_nym) - messages read from the block where it already sits on the device, the nym kernel on a stream of
// its own next to the ECDSA kernels, the SHA-256(message) the memo wants from the same gather launch as the TxID / proposal-hash
// digests.  (As separate blocking calls with their own copy of the messages, 2 000 idemix creators cost a 10 000-tx block 2 ms.)
Error GPUCSP::SubmitIdentityBatch(HostPass& hp) const {
    typedef PassScratch::Gated Gated;
    const uint8_t* const block = hp.block;
    const ParsedBlock& pb = hp.pb;
    BlockVerdicts& out = hp.out;
    BlockUpload* const up = hp.up;
    PassScratch& ps_ = hp.ps;
    const bool want_digests = hp.want_digests, all_keyed = hp.all_keyed;
    const size_t n = hp.n;
    std::vector<uint32_t>&sub = ps_.sub, &ids = ps_.ids, &off = ps_.off, &pre_idx = ps_.pre_idx;
    std::vector<uint8_t>&qx = ps_.qx, &qy = ps_.qy, &r = ps_.r, &s = ps_.s, &hash_digests = ps_.hash_digests;
    std::vector<uint32_t>&ns = ps_.nym_idx, &nsp = ps_.nym_sp, &niss = ps_.nym_iss;
    std::vector<uint8_t>&nfields = ps_.nym_fields, &nst = ps_.nym_st;
    std::vector<uint64_t>& nbits = ps_.nym_bits;
    const std::vector<Gated>& gt = ps_.gt;
    const size_t mn = ns.size();
    if (mn) {
        nsp.resize(2 * mn);
        niss.resize(mn);
        nfields.resize(6 * 32 * mn);
        nbits.assign((mn + 63) / 64, 0);
        nst.assign(mn, 0);
        for (size_t j = 0; j < mn; j++) {
            const Gated& g0 = gt[ns[j]];
            const BlockTuple& tp = pb.tuples[ns[j]];
            nsp[2 * j] = tp.suffix.off;
            nsp[2 * j + 1] = tp.suffix.off + tp.suffix.len;
            niss[j] = (uint32_t)g0.key_id;
            const uint8_t* col[6] = {g0.qx, g0.qy, g0.r, g0.s, g0.srn, g0.nonce};
            for (int k = 0; k < 6; k++) memcpy(&nfields[32 * (mn * k + j)], col[k], 32);
        }
    }
    std::vector<uint32_t>& pre_off = ps_.pre_off;
    pre_off.resize(2 * pb.prefixes.size() + 2);
    for (size_t p = 0; p < pb.prefixes.size(); p++) {
        pre_off[2 * p] = pb.prefixes[p].off;
        pre_off[2 * p + 1] = pb.prefixes[p].off + pb.prefixes[p].len;
    }
    std::vector<uint64_t>& bits = ps_.bits;
    std::vector<uint8_t>& st = ps_.st;
    bits.assign((n + 63) / 64, 0);
    st.assign(n, 0);
    fabgpu_identity_batch d;
    memset(&d, 0, sizeof(d));
    d.n = n;
    d.arena = block;
    d.off = off.data();
    d.n_prefixes = (uint32_t)pb.prefixes.size();
    d.pre_off = pre_off.data();
    d.pre_idx = pre_idx.data();
    if (all_keyed) {
        d.key_id = ids.data();
    } else {
        d.qx = qx.data();
        d.qy = qy.data();
    }
    d.r = r.data();
    d.s = s.data();
    d.verdict_bits = bits.data();
    d.status = st.data();
    d.flags = FABGPU_IDB_SPANS;
    if (!pb.tail.empty()) {                           // the orderers' block-signature messages (block_prepass.h TUPLE_BLOCK_SIG)
        d.tail = pb.tail.data();
        d.tail_base = pb.tail_base;
        d.tail_len = (uint32_t)pb.tail.size();
    }
    std::vector<uint8_t>& dig = ps_.dig;
    if (want_digests) {
        if (dig.size() < n * 32) dig.resize(n * 32);
        d.digests = dig.data();
    }
    // the TxID and proposal-hash digests of the endorser transactions ride along (one upload of the block, one submission)
    const size_t nh = hp.skip_hash_checks ? 0 : pb.hash_checks.size();   // the switch exists for A/B timing only
    std::vector<uint32_t>& gsp = ps_.gsp;
    const size_t nhn = want_digests ? mn : 0;          // + SHA-256 of every idemix creator's message (the memo's digest)
    gsp.assign((nh + nhn) * 6, 0);
    hash_digests.assign((nh + nhn) * 32, 0);
    for (size_t j = 0; j < nh; j++)
        for (int p = 0; p < 3; p++) {
            const Span& sp = pb.hash_checks[j].piece[p];
            gsp[6 * j + 2 * p] = sp.off;
            gsp[6 * j + 2 * p + 1] = sp.off + sp.len;
        }
    for (size_t j = 0; j < nhn; j++) {
        gsp[6 * (nh + j)] = nsp[2 * j];
        gsp[6 * (nh + j) + 1] = nsp[2 * j + 1];
    }
    if (nh + nhn) {
        d.n_gather = (uint32_t)(nh + nhn);
        d.gather_spans = gsp.data();
        d.gather_digests = hash_digests.data();
        hp.hashes_done = nh != 0;
    }
    if (mn) {
        d.n_nym = (uint32_t)mn;
        d.nym_off = nsp.data();
        d.nym_issuer = niss.data();
        d.nym_fields = nfields.data();
        d.nym_verdict_bits = nbits.data();
        d.nym_status = nst.data();
    }
    auto clk1 = std::chrono::steady_clock::now();
    uint64_t tok = up ? up->join() : 0;
    out.ms_upload_wait = ms_since(clk1);
    auto clk2 = std::chrono::steady_clock::now();
    int rc = FABGPU_EINVAL;
    if (tok) {
        d.flags = FABGPU_IDB_SPANS | FABGPU_IDB_ARENA_STAGED;
        d.stage_token = tok;
        rc = fabgpu_identity_verify_batch(hp.dv.ctx, &d);      // FABGPU_EINVAL: somebody else's upload replaced ours -> resubmit with the bytes
        d.flags = FABGPU_IDB_SPANS;
    }
    if (!tok || rc == FABGPU_EINVAL) rc = fabgpu_identity_verify_batch(hp.dv.ctx, &d);
    out.ms_device = ms_since(clk2);
    if (rc != FABGPU_OK) return Error(std::string("GPU verify failed: ") + fabgpu_strerror(rc));
    hp.dv.passes.fetch_add(1, std::memory_order_relaxed);
    for (size_t j = 0; j < n; j++) {
        bool bit = (bits[j >> 6] >> (j & 63)) & 1;
        if (all_keyed && st[j] == FABGPU_ST_OFF_CURVE) {
            // (the id was retired between the cache lookup above and the launch - key_slots.h: "use bccsp/sw", never "invalid")
            out.tuple_status[sub[j]] = TUPLE_ST_NEEDS_SW;
            continue;
        }
        out.tuple_status[sub[j]] = (bit && st[j] == FABGPU_ST_VALID) ? FABGPU_ST_VALID : (st[j] == FABGPU_ST_VALID ? FABGPU_ST_BAD_MATH : st[j]);
        out.tuple_hashed[sub[j]] = 1;
        if (want_digests) memcpy(&out.tuple_digest[32 * (size_t)sub[j]], &dig[32 * j], 32);
    }
    for (size_t j = 0; j < mn; j++)
        write_nym_result(out, ns[j], nst[j], want_digests ? &hash_digests[32 * (nh + j)] : nullptr, gt[ns[j]].qx, gt[ns[j]].qy);
    hp.nym_rode = mn != 0;
    return Error();
}

// idemix creators of a block WITHOUT any ECDSA tuple (nothing to ride on): their messages (the envelope payloads) are gathered into
// one arena for the nym entry point
Error GPUCSP::VerifyNymsAlone(HostPass& hp) const {
    typedef PassScratch::Gated Gated;
    const uint8_t* const block = hp.block;
    const ParsedBlock& pb = hp.pb;
    const std::vector<uint32_t>& ns = hp.ps.nym_idx;
    const std::vector<Gated>& gt = hp.ps.gt;
    fabgpu_ctx* const ctx_ = hp.dv.ctx;
    const size_t m = ns.size();
    std::vector<uint8_t> cols[6], arena;
    std::vector<uint32_t> iss(m), noff(m + 1, 0);
    size_t total = 0;
    for (size_t j = 0; j < m; j++) total += pb.tuples[ns[j]].suffix.len;
    if (total > 0x7FFFFFFFull) return Error("idemix creator messages exceed 2 GiB");
    arena.reserve(total + 1);
    for (int k = 0; k < 6; k++) cols[k].reserve(m * 32);
    for (size_t j = 0; j < m; j++) {
        const Gated& g0 = gt[ns[j]];
        const BlockTuple& tp = pb.tuples[ns[j]];
        cols[0].insert(cols[0].end(), g0.qx, g0.qx + 32);
        cols[1].insert(cols[1].end(), g0.qy, g0.qy + 32);
        cols[2].insert(cols[2].end(), g0.r, g0.r + 32);
        cols[3].insert(cols[3].end(), g0.s, g0.s + 32);
        cols[4].insert(cols[4].end(), g0.srn, g0.srn + 32);
        cols[5].insert(cols[5].end(), g0.nonce, g0.nonce + 32);
        iss[j] = (uint32_t)g0.key_id;
        arena.insert(arena.end(), block + tp.suffix.off, block + tp.suffix.off + tp.suffix.len);
        noff[j + 1] = (uint32_t)arena.size();
    }
    if (arena.empty()) arena.push_back(0);
    std::vector<uint64_t> bits((m + 63) / 64);
    std::vector<uint8_t> st(m);
    int rc = fabgpu_idemix_nym_verify_batch(ctx_, m, arena.data(), noff.data(), iss.data(), cols[0].data(), cols[1].data(), cols[2].data(),
                                            cols[3].data(), cols[4].data(), cols[5].data(), bits.data(), st.data());
    if (rc != FABGPU_OK) return Error(std::string("GPU nym verify failed: ") + fabgpu_strerror(rc));
    std::vector<uint8_t> nd;
    if (hp.want_digests) {
        nd.resize(m * 32);
        rc = fabgpu_sha256_batch(ctx_, m, arena.data(), noff.data(), nd.data());
        if (rc != FABGPU_OK) return Error(std::string("GPU hash failed: ") + fabgpu_strerror(rc));
    }
    for (size_t j = 0; j < m; j++) write_nym_result(hp.out, ns[j], st[j], hp.want_digests ? &nd[32 * j] : nullptr, gt[ns[j]].qx, gt[ns[j]].qy);
    return Error();
}

// TxID / proposal hash: compare what the device computed with what the block claims.  (No ECDSA tuple went to the device -
// a block of idemix creators only, say - means no submission the hashes could ride on: those checks stay with the Go validators.)
void GPUCSP::CompareHashesAndSummarize(HostPass& hp) {
    const ParsedBlock& pb = hp.pb;
    BlockVerdicts& out = hp.out;
    std::vector<uint8_t> bad_txid(pb.n_tx, 0), bad_phash(pb.n_tx, 0);
    if (hp.hashes_done)
        for (size_t j = 0; j < pb.hash_checks.size(); j++) {
            const BlockHashCheck& hc = pb.hash_checks[j];
            if (HashCheckMatches(hp.block, hc, hp.ps.hash_digests.data() + 32 * j)) continue;
            if (hc.kind == HASH_TXID) bad_txid[hc.tx] = 1;
            else bad_phash[hc.tx] = 1;
        }
    SummarizeTransactions(pb.n_tx, pb.tx_understood.data(), out.tuple_status.size(), out.tuple_tx.data(), out.tuple_kind.data(), out.tuple_status.data(),
                          hp.hashes_done ? bad_txid.data() : nullptr, hp.hashes_done ? bad_phash.data() : nullptr, out.tx_flags.data());
}

Error GPUCSP::PreVerifyParsed(const uint8_t* block, const ParsedBlock& pb, BlockVerdicts& out, BlockUpload* up, const PassOptions& opt) const {
    // `out` may come back from the previous block (the C entry points keep one per calling thread): its vectors keep their capacity -
    // a fresh 3 MB of answer arrays per block is 700 page faults - and every element is (re)written below
    const bool want_digests = opt.want_digests || opt.seed_memo;
    const size_t nt = pb.tuples.size();
    out.n_tx = pb.n_tx;
    out.distinct_identities = 0;
    out.ms_gates = out.ms_upload_wait = out.ms_device = 0;
    out.memo_seeded = 0;
    out.tx_type = pb.tx_type;
    out.tx_flags.resize(pb.n_tx);                        // (written at the end: SummarizeTransactions)
    out.tuple_tx.resize(nt);
    out.tuple_kind.resize(nt);
    out.tuple_status.assign(nt, FABGPU_ST_VALID);
    out.tuple_qxy.resize(nt * 64);                       // written per tuple by the gates (key or zeros)
    out.tuple_hashed.assign(nt, 0);
    if (want_digests) out.tuple_digest.assign(nt * 32, 0);
    else out.tuple_digest.clear();
    out.n_block_sigs = pb.n_block_sigs;
    out.block_sigs_understood = pb.block_sigs_understood ? 1 : 0;
    // The scratch below (8 MB for a 40 000-tuple block) is reused from block to block instead of being allocated - and page-faulted
    // in - per call.  Passes of different callers run side by side, each on a set of its own (up to four are kept): one caller's gates
    // and flags overlap another's device call (two callers, 10 000-tx blocks: 3.2 ms per block with one pass at a time).
    ScratchLease lease(this);
    // the device this pass runs on: where its block travelled to, or - no upload - wherever the ring points
    Dev& dv = *devs_[(size_t)(up && up->routed ? up->dev : RouteBlock(opt.block_seq))];
    bool skip_hash_checks;
    {
        std::lock_guard<std::mutex> lk(opt_mu_);
        skip_hash_checks = opts_.pass_skip_hash_checks > 0;
    }
    HostPass hp{block, pb, out, up, opt, *lease.p, dv, want_digests, skip_hash_checks};
    Error e = GateAndCompact(hp);
    if (e.ok() && hp.n) e = SubmitIdentityBatch(hp);
    if (!e.ok()) return e;
    {   // idemix creators of a block WITHOUT any ECDSA tuple: nothing to ride on
        StageClock nym_clock{out.ms_nym};
        if (!hp.nym_rode && !hp.ps.nym_idx.empty()) e = VerifyNymsAlone(hp);
        if (!e.ok()) return e;
    }
    CompareHashesAndSummarize(hp);
    RegisterQueued(hp.to_register);
    if (opt.seed_memo) SeedMemo(block, pb, out, opt, hp.ps.sub, kGateMax, up);
    return Error();
}

// ------------------------------------------------------------------------------------------------
// The P-384 stage of the pass (bccsp_host.h P384PassStage): shared by the two routes
// ------------------------------------------------------------------------------------------------
void GPUCSP::P384PassStats(uint64_t out[P384_PASS_STATS]) const {
    for (int i = 0; i < P384_PASS_STATS; i++) out[i] = p384_pass_[i].load(std::memory_order_relaxed);
}

Error GPUCSP::P384PassStage(const uint8_t* block, size_t len, const ParsedBlock& parsed, BlockVerdicts& out, BlockUpload* up, const PassOptions& opt) const {
    if (!P384Enabled() || Poisoned() || !block) return Error();
    const size_t nt = out.tuple_status.size();
    if (!nt || !memchr(out.tuple_status.data(), TUPLE_ST_NEEDS_SW, nt)) return Error();   // (an all-P-256 block: 40 000 status bytes read once)
    std::vector<uint32_t> sw;                                            // the tuples the route left to bccsp/sw
    for (size_t i = 0; i < nt; i++)
        if (out.tuple_status[i] == TUPLE_ST_NEEDS_SW) sw.push_back((uint32_t)i);
    // the tuples' own records: the route's, or - the device route brings none back unless its caller asked - a host walk of the block,
    // which lists the same tuples in the same order (tests/test_device_walk.py holds the two walkers to that)
    const ParsedBlock* pb = &parsed;
    ParsedBlock walked;
    if (parsed.tuples.size() != nt) {
        if (!ParseBlock(block, len, walked, WalkThreads()) || walked.tuples.size() != nt) return Error();   // (not the route's list: leave its answers)
        pb = &walked;
    }
    // identity -> key, through the identity cache (an entry learns its P-384 answer once); idemix creators and whatever is no on-curve
    // P-384 certificate key stay NEEDS_SW
    struct Row {
        uint32_t tuple;
        ECDSAPublicKey384 key;
        bool sha3;                                                       // the identity's MSP is set SHA3 (msp_family.h)
    };
    struct Front {
        Span identity;
        CachedIdentity ci;
        bool sha3;
    };
    // what one family's rows send: key, r and s columns, and the rows they belong to
    struct Family {
        std::vector<uint32_t> row;
        std::vector<uint8_t> qx, qy, r, s;
    } fam[2];                                                            // [0] SHA2 rows, [1] SHA3 rows
    std::vector<Row> rows;
    std::vector<Front> front;                                            // a block names few identities
    static const uint8_t one_digest[1] = {1};
    const bool any_sha3 = Sha3Enabled() && msp_family_.AnySha3();        // (read once: a change holds for passes that start after it)
    uint64_t seen = 0;
    bool touched = false;
    for (uint32_t i : sw) {
        const BlockTuple& tp = pb->tuples[i];
        if ((uint64_t)tp.identity.off + tp.identity.len > len || (uint64_t)tp.sig.off + tp.sig.len > len) continue;
        const uint8_t* ident = block + tp.identity.off;
        const Front* fr = nullptr;
        for (auto& f : front)
            if (f.identity.len == tp.identity.len && memcmp(block + f.identity.off, ident, tp.identity.len) == 0) {
                fr = &f;
                break;
            }
        if (!fr) {
            CachedIdentity c;
            bool cached = false;
            std::string key((const char*)ident, tp.identity.len);
            {
                std::lock_guard<std::mutex> lk(idmu_);
                auto it = idcache_.find(key);
                if (it != idcache_.end()) {
                    c = it->second->second;
                    cached = true;
                }
            }
            if (c.p384 == 0) {                                           // decoded outside the lock, as the P-256 key was
                c.p384 = !c.p256 && IdentityToP384(ident, tp.identity.len, c.qx384, c.qy384) && p384::pubkey_on_curve(c.qx384, c.qy384) ? 1 : 2;
                if (cached) {
                    std::lock_guard<std::mutex> lk(idmu_);
                    auto it = idcache_.find(key);
                    if (it != idcache_.end() && it->second->second.p384 == 0) {
                        CachedIdentity& e = it->second->second;
                        e.p384 = c.p384;
                        memcpy(e.qx384, c.qx384, 48);
                        memcpy(e.qy384, c.qy384, 48);
                    }
                }
            }
            // the MSP's family: looked up per pass, never kept in the identity cache
            bool sha3 = false;
            const uint8_t* mspid;
            size_t mspid_len;
            if (any_sha3 && c.p384 == 1 && IdentityMspId(ident, tp.identity.len, mspid, mspid_len)) sha3 = msp_family_.Sha3(mspid, mspid_len);
            front.push_back(Front{tp.identity, c, sha3});
            fr = &front.back();
        }
        const CachedIdentity* ci = &fr->ci;
        if (ci->p384 != 1) continue;
        seen++;
        touched = true;
        if (tp.sig.len == 0) {
            out.tuple_status[i] = TUPLE_ST_EMPTY_SIG;
            continue;
        }
        Row row;
        row.tuple = i;
        row.sha3 = fr->sha3;
        memcpy(row.key.x, ci->qx384, 48);
        memcpy(row.key.y, ci->qy384, 48);
        row.key.on_curve = true;
        const GateT<Curve384> g = gate_item<Curve384>(&row.key, block + tp.sig.off, tp.sig.len, one_digest, 1);
        if (!g.submit) {
            out.tuple_status[i] = gate_tuple_status(g.res);
            continue;
        }
        Family& f = fam[row.sha3 ? 1 : 0];
        f.row.push_back((uint32_t)rows.size());
        rows.push_back(row);
        f.qx.insert(f.qx.end(), row.key.x, row.key.x + 48);
        f.qy.insert(f.qy.end(), row.key.y, row.key.y + 48);
        f.r.insert(f.r.end(), g.r, g.r + 48);
        f.s.insert(f.s.end(), g.s, g.s + 48);
    }
    if (!touched) return Error();
    p384_pass_[P384_PASS_STAGES].fetch_add(1, std::memory_order_relaxed);
    p384_pass_[P384_PASS_SEEN].fetch_add(seen, std::memory_order_relaxed);
    const size_t n = rows.size();
    std::vector<uint8_t> st(n, 0), ok(n, 0), from_keyed(n, 0);           // per row: status byte, verdict bit, answered by a keyed launch
    std::vector<uint8_t> dig;                                            // seeding: the digests as the device verified them, the memo's keys
    if (opt.seed_memo) dig.resize(32 * n);
    uint64_t tok = 0;
    bool joined = false;
    for (int sha3 = 0; sha3 < 2; sha3++) {
        // one described batch per family over the block: message spans and prefixes from the tuples' own records, the orderers' messages
        // in the tail.  A block without SHA3 rows: the one batch there always was.
        const Family& f = fam[sha3];
        const size_t fn = f.row.size();
        if (!fn) continue;
        std::vector<uint32_t> off(2 * fn), pre_idx(fn), pre_off;
        std::vector<std::pair<uint64_t, uint32_t>> pre_seen;             // (off << 32 | len) -> index, in order of first use
        for (size_t j = 0; j < fn; j++) {
            const BlockTuple& tp = pb->tuples[rows[f.row[j]].tuple];
            off[2 * j] = tp.suffix.off;
            off[2 * j + 1] = tp.suffix.off + tp.suffix.len;
            pre_idx[j] = 0xFFFFFFFFu;
            if (tp.prefix.len == 0) continue;
            const uint64_t k = (uint64_t)tp.prefix.off << 32 | tp.prefix.len;
            if (pre_seen.empty() || pre_seen.back().first != k) {        // (a transaction's endorsements follow each other)
                pre_seen.emplace_back(k, (uint32_t)(pre_off.size() / 2));
                pre_off.push_back(tp.prefix.off);
                pre_off.push_back(tp.prefix.off + tp.prefix.len);
            }
            pre_idx[j] = pre_seen.back().second;
        }
        Dev& dv = *devs_[(size_t)(up && (up->routed || up->started) ? up->dev : 0)];
        fabgpu_identity_batch_p384 d;
        memset(&d, 0, sizeof(d));
        d.n = fn;
        d.arena = block;
        d.off = off.data();
        d.n_prefixes = (uint32_t)(pre_off.size() / 2);
        d.pre_off = pre_off.data();
        d.pre_idx = pre_idx.data();
        std::vector<uint32_t> ids;
        const std::vector<uint8_t> submitted(fn, 1);
        const bool keyed = all_registered<Curve384>(dv.ctx, fn, submitted, f.qx.data(), f.qy.data(), ids);
        if (keyed) {
            d.key_id = ids.data();
        } else {
            d.qx = f.qx.data();
            d.qy = f.qy.data();
        }
        d.r = f.r.data();
        d.s = f.s.data();
        std::vector<uint8_t> fst(fn, 0), fdig;
        std::vector<uint64_t> bits((fn + 63) / 64, 0);
        d.verdict_bits = bits.data();
        d.status = fst.data();
        if (opt.seed_memo) {
            fdig.resize(32 * fn);
            d.digests = fdig.data();
        }
        if (!pb->tail.empty()) {
            d.tail = pb->tail.data();
            d.tail_base = pb->tail_base;
            d.tail_len = (uint32_t)pb->tail.size();
        }
        if (!joined) tok = up ? up->join() : 0;                          // (both batches read the same staged block)
        joined = true;
        const auto submit = sha3 ? fabgpu_identity_verify_batch_p384_sha3 : fabgpu_identity_verify_batch_p384;   // the family is the entry's
        const bool wide = keyed && ctx_p384_wide_serves(dv.ctx, fn);      // (what the context's launch site decides for a keyed batch of fn rows)
        int rc = FABGPU_EINVAL;
        if (tok) {
            d.flags = FABGPU_IDB_SPANS | FABGPU_IDB_ARENA_STAGED;
            d.stage_token = tok;
            rc = submit(dv.ctx, &d);                                     // FABGPU_EINVAL: somebody else's upload replaced ours -> resubmit with the bytes
        }
        d.flags = FABGPU_IDB_SPANS;
        if (!tok || rc == FABGPU_EINVAL) rc = submit(dv.ctx, &d);
        if (rc != FABGPU_OK) return Error(std::string("GPU verify failed: ") + fabgpu_strerror(rc));
        p384_pass_[P384_PASS_SUBMITTED].fetch_add(fn, std::memory_order_relaxed);
        p384_pass_[keyed ? P384_PASS_KEYED : P384_PASS_FRESH].fetch_add(1, std::memory_order_relaxed);
        if (sha3) p384_pass_[P384_PASS_SHA3_ROWS].fetch_add(fn, std::memory_order_relaxed);
        if (wide) p384_pass_wide_rows_.fetch_add(fn, std::memory_order_relaxed);
        for (size_t j = 0; j < fn; j++) {
            const uint32_t k = f.row[j];
            st[k] = fst[j];
            ok[k] = (uint8_t)((bits[j >> 6] >> (j & 63)) & 1);
            from_keyed[k] = keyed ? 1 : 0;
            if (opt.seed_memo) memcpy(&dig[32 * (size_t)k], &fdig[32 * j], 32);
        }
    }
    if (n) {
        std::string msg;
        for (size_t j = 0; j < n; j++) {
            const uint32_t i = rows[j].tuple;
            if (from_keyed[j] && st[j] == FABGPU_ST_OFF_CURVE) continue;  // (the id was retired under the launch: "use bccsp/sw", never "invalid")
            bool valid = ok[j] && st[j] == FABGPU_ST_VALID;
            if (!valid && st[j] == FABGPU_ST_BAD_MATH) {                 // (test hook: a corrupted verdict)
                uint32_t f = test_p384_flip_.load(std::memory_order_relaxed);
                while (f && !test_p384_flip_.compare_exchange_weak(f, f - 1)) {}
                if (f) valid = true;
            }
            out.tuple_status[i] = valid ? FABGPU_ST_VALID : (st[j] == FABGPU_ST_VALID ? FABGPU_ST_BAD_MATH : st[j]);
            if (!valid || !audit_sample_[AUDIT_DIRECT].hit(AuditPermille())) continue;
            // the audit: the message bytes of the CALLER's block, hashed (with the row's family) and verified on the CPU
            const BlockTuple& tp = pb->tuples[i];
            auto bytes_of = [&](const Span& sp) -> const uint8_t* {
                if (!pb->tail.empty() && sp.off >= pb->tail_base) return (uint64_t)sp.off - pb->tail_base + sp.len <= pb->tail.size() ? pb->tail.data() + (sp.off - pb->tail_base) : nullptr;
                return (uint64_t)sp.off + sp.len <= len ? block + sp.off : nullptr;
            };
            const uint8_t *pp = bytes_of(tp.prefix), *sp = bytes_of(tp.suffix);
            bool accept = false;
            {
                AuditClock clk{audit_count_[AUDIT_NS]};
                if (pp && sp) {
                    msg.assign((const char*)pp, tp.prefix.len);
                    msg.append((const char*)sp, tp.suffix.len);
                    uint8_t dg[32];
                    if (rows[j].sha3) audit_sha3_256((const uint8_t*)msg.data(), msg.size(), dg);
                    else audit_sha256((const uint8_t*)msg.data(), msg.size(), dg);
                    accept = audit_p384_verify(rows[j].key.x, rows[j].key.y, block + tp.sig.off, tp.sig.len, dg, 32);
                }
            }
            audit_count_[AUDIT_DIRECT].fetch_add(1, std::memory_order_relaxed);
            p384_pass_[P384_PASS_AUDITED].fetch_add(1, std::memory_order_relaxed);
            if (!accept) {
                audit_count_[AUDIT_MISMATCHES].fetch_add(1, std::memory_order_relaxed);
                Poison(std::string("block pass: the device accepted a P-384 signature that the CPU audit rejects (key X ") + hex8(rows[j].key.x) + "..)");
                return Error();                                          // (the caller answers what a poisoned pass answers)
            }
        }
        // The verdict memo of these tuples (p384_memo.h): one entry per row the device decided, with the status written above and the
        // signature bytes as they sit in the caller's block - the bytes the audit just used.  Rows skipped for a retired id get none.
        // Published whether or not the block also published a BlockMemo; a provider poisoned meanwhile publishes nothing.
        if (opt.seed_memo && !Poisoned()) {
            try {
                auto rec = std::make_shared<P384Memo::Record>(opt.block_seq, n);
                for (size_t j = 0; j < n; j++) {
                    if (from_keyed[j] && st[j] == FABGPU_ST_OFF_CURVE) continue;
                    const BlockTuple& tp = pb->tuples[rows[j].tuple];
                    rec->Add(rows[j].key.x, rows[j].key.y, block + tp.sig.off, tp.sig.len, &dig[32 * j], 32, out.tuple_status[rows[j].tuple]);
                }
                const uint32_t added = rec->size();
                if (p384_memo_.Publish(std::move(rec), &poisoned_)) {
                    out.memo_seeded += added;
                    p384_pass_[P384_PASS_MEMO_SEEDED].fetch_add(added, std::memory_order_relaxed);
                }
            } catch (const std::bad_alloc&) {                            // no entries for this block: its lookups miss
            }
        }
    }
    // The flags of the affected transactions, folded again.  What the route's fold knew and the tuples do not say - "not understood", a
    // bad TxID, a bad proposal hash - is read back from the flag it produced: each of them outranks everything below it in the fold, so
    // a flag that names one of them hides nothing the new fold needs (block_prepass.h SummarizeTransactions).
    const uint32_t n_tx = (uint32_t)out.tx_flags.size();
    std::vector<uint8_t> understood(n_tx, 1), bad_txid(n_tx, 0), bad_phash(n_tx, 0), kind(nt), flags(n_tx, 0), affected(n_tx, 0);
    std::vector<uint32_t> tx(nt);
    for (uint32_t t = 0; t < n_tx; t++) {
        understood[t] = out.tx_flags[t] != TX_NOT_UNDERSTOOD;
        bad_txid[t] = out.tx_flags[t] == TX_BAD_TXID;
        bad_phash[t] = out.tx_flags[t] == TX_BAD_PROPOSAL_HASH;
    }
    for (size_t i = 0; i < nt; i++) {
        tx[i] = pb->tuples[i].tx;
        kind[i] = pb->tuples[i].kind;
    }
    for (uint32_t i : sw)
        if (tx[i] < n_tx) affected[tx[i]] = 1;
    SummarizeTransactions(n_tx, understood.data(), nt, tx.data(), kind.data(), out.tuple_status.data(), bad_txid.data(), bad_phash.data(), flags.data());
    for (uint32_t t = 0; t < n_tx; t++)
        if (affected[t]) out.tx_flags[t] = flags[t];
    return Error();
}

}  // namespace bccsp
}  // namespace fab

// ------------------------------------------------------------------------------------------------
// C entry points of include/fabgpu.h that are pure host logic
// ------------------------------------------------------------------------------------------------
extern "C" {

int fabgpu_ecdsa_unmarshal_signature(const uint8_t* sig, size_t len, uint8_t* r32, uint8_t* s32, int* flags) {
    fab::bccsp::BigInt R, S;
    fab::bccsp::Error e = fab::bccsp::UnmarshalECDSASignature(sig, len, R, S);
    if (!e.ok()) {
        if (e.msg.find("R must be larger") != std::string::npos) return 2;
        if (e.msg.find("S must be larger") != std::string::npos) return 3;
        return 1;
    }
    if (r32) R.to_be32(r32);
    if (s32) S.to_be32(s32);
    if (flags) *flags = (R.fits256() ? 0 : 1) | (S.fits256() ? 0 : 2);
    return 0;
}
int fabgpu_ecdsa_is_low_s(const uint8_t* s32) { return memcmp(s32, fab::bccsp::HALF_N_BE, 32) <= 0 ? 1 : 0; }
int fabgpu_p256_pubkey_on_curve(const uint8_t* qx32, const uint8_t* qy32) { return fab::bccsp::PublicKeyOnCurve(qx32, qy32) ? 1 : 0; }
void fabgpu_hash_to_int(const uint8_t* digest, size_t len, uint8_t* e32) { fab::bccsp::HashToInt(digest, len, e32); }

// ... and their P-384 namesakes (p384.h compiled for the host)
int fabgpu_ecdsa_unmarshal_signature_p384(const uint8_t* sig, size_t len, uint8_t* r48, uint8_t* s48, int* flags) {
    fab::bccsp::BigInt R, S;
    fab::bccsp::Error e = fab::bccsp::UnmarshalECDSASignature(sig, len, R, S);
    if (!e.ok()) {
        if (e.msg.find("R must be larger") != std::string::npos) return 2;
        if (e.msg.find("S must be larger") != std::string::npos) return 3;
        return 1;
    }
    int fl = 0;
    const fab::bccsp::BigInt* v[2] = {&R, &S};
    uint8_t* o[2] = {r48, s48};
    for (int k = 0; k < 2; k++) {
        const std::vector<uint8_t> m = v[k]->magnitude();       // big-endian, minimal
        if (m.size() > 48) fl |= 1 << k;
        if (o[k]) {
            memset(o[k], 0, 48);
            const size_t take = m.size() < 48 ? m.size() : 48;
            memcpy(o[k] + 48 - take, m.data() + m.size() - take, take);
        }
    }
    if (flags) *flags = fl;
    return 0;
}
int fabgpu_ecdsa_is_low_s_p384(const uint8_t* s48) { return fab::p384::is_low_s(s48) ? 1 : 0; }
int fabgpu_p384_pubkey_on_curve(const uint8_t* qx48, const uint8_t* qy48) { return fab::p384::pubkey_on_curve(qx48, qy48) ? 1 : 0; }
void fabgpu_hash_to_int_p384(const uint8_t* digest, size_t len, uint8_t* e48) { fab::p384::hash_to_int(digest, len, e48); }

}  // extern "C"
