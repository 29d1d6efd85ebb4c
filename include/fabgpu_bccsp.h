/*
 * fabgpu_bccsp.h - flat C view of the C++ host mirror (fabric-mod_amd/csrc/bccsp_host.h) so that the
 * Python parity tests (and any other FFI) can drive the provider with the reference's vocabulary:
 *   bccsp/sw/impl.go:177-194   CSP.Hash        -> fabgpu_csp_hash
 *   bccsp/sw/impl.go:247-270   CSP.Verify      -> fabgpu_csp_verify / fabgpu_csp_verify_batch
 *   msp/identities.go:169-196  identity.Verify -> fabgpu_csp_identity_verify_batch
 * Error strings are the Go `error` text ("" == nil).  All functions return 0, or a negative FABGPU_E* when the
 * device failed (the caller then falls back to bccsp/sw).  The production binding is cgo over fabgpu.h
 * (INTEGRATION.md); this header adds no new capability.
 */
#ifndef FABGPU_BCCSP_H
#define FABGPU_BCCSP_H
#include "fabgpu.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct fabgpu_csp fabgpu_csp;

int fabgpu_csp_new(const fabgpu_cfg* cfg, fabgpu_csp** out, char* err, size_t errcap);
/* ONE provider over SEVERAL devices.  The reference has one process-global BCCSP (bccsp/factory/factory.go:41-55: GetDefault), handed to
 * every channel's validator (core/peer/peer.go:337-355), and validates its channels side by side (core/committer/txvalidator/v20/
 * validator.go:194-210): whatever drives more than one GPU has to sit BEHIND that one object.  fabgpu_csp_new2 makes one device context
 * per entry of `devices` (an ordinal may repeat: several contexts on one GPU); every block pass is routed to the context with the fewest
 * passes in flight (ties: round the ring from block_seq mod G), the identity cache and the verdict memo stay ONE on the host -
 * fabgpu_csp_memo_lookup does not care which device verified - and registered keys / idemix issuers get their tables on every device
 * under the same id.  Flat batches (verify_batch, identity_verify_batch, coalesced launches) take turns round the pool.
 * This struct is what `GPU:` of the BCCSP configuration carries (go/bccsp/factory/gpufactory.go GPUOpts; pattern bccsp/pkcs11/conf.go:70-84);
 * `size` = sizeof(fabgpu_csp_opts) as the caller compiled it (the struct may grow at its end). */
typedef struct fabgpu_csp_opts {
    uint32_t size;
    int32_t n_devices;             /* 0: every visible gfx950 device */
    const int32_t* devices;        /* n_devices HIP ordinals, or NULL = 0 .. n_devices-1 */
    uint32_t ctx_flags;            /* FABGPU_FLAG_* for every context */
    uint32_t concurrent_passes;    /* per device: what this many overlapping block passes need - staging slots, pinned memo tables, pass
                                      arrays, kept block copies (concurrent_passes + 2 of them), a slab of key tables - is allocated NOW, not
                                      when passes first overlap (0: on demand).  Any value > 0 makes ALL THREE staging slots of a device
                                      (3 x expect_block_bytes of device memory): uploads walk round all of them even when passes never overlap */
    uint64_t expect_block_bytes;   /* sizes that pre-allocation (0: 64 MiB) */
    uint32_t expect_tuples;        /* (0: 65 536) */
    /* switches that were environment variables through round 3: 0 = the default, > 0 on, < 0 off (a zeroed struct is all defaults) */
    int32_t pass_device_walk;      /* < 0: every block takes the host walk (default: the walk runs on the device) */
    int64_t pass_stage_min_bytes;  /* > 0: only blocks of at least this many bytes are uploaded ahead of their pass (default: every block) */
    int32_t pass_device_memo;      /* < 0: the verdict memo is seeded on the host also on the device route (default: built by the device) */
    int32_t pass_host_counts;      /* > 0: the envelopes' tuples are counted on the host while the block travels (default off) */
    int32_t pass_timing;           /* > 0: stage breakdown of every pass on stderr (default off) */
    int32_t pass_hash_memo;        /* < 0: no digest memo - memo-seeding passes keep no host copy of their block and fabgpu_csp_hash_lookup
                                      always misses (default on) */
    uint32_t hash_memo_blocks;     /* per device: host copies of blocks the digest memo keeps at a time, each as large as its block, pinned
                                      (0: 8; at most 64).  A block beyond that simply has no digest memo: its messages are hashed on the CPU */
    uint32_t audit_permille;       /* 0 .. 1000: share of what the provider hands out from the device that it re-computes on the CPU first
                                      (see "CPU audit" below; 0, the default: none).  fabgpu_csp_new2 answers FABGPU_EINVAL beyond 1000.
                                      On LP64 the field occupies what was the struct's tail padding - sizeof has not changed -, so a caller
                                      built against the older header hands over whatever its padding held: as ever, zero the struct first */
} fabgpu_csp_opts;
int fabgpu_csp_new2(const fabgpu_csp_opts* opts, fabgpu_csp** out, char* err, size_t errcap);
void fabgpu_csp_free(fabgpu_csp* csp);
fabgpu_ctx* fabgpu_csp_ctx(fabgpu_csp* csp);            /* the first device's context */
int fabgpu_csp_device_count(fabgpu_csp* csp);            /* contexts in the pool */
fabgpu_ctx* fabgpu_csp_ctx_of(fabgpu_csp* csp, int d);
/* passes[d] = block passes context d has served; returns the number of contexts (cap must be at least that) */
int fabgpu_csp_passes_per_device(fabgpu_csp* csp, uint64_t* passes, int cap);
int fabgpu_csp_route_block(fabgpu_csp* csp, uint64_t block_seq);   /* where a pass named block_seq would go right now */
/* the switches above on a living provider (tests, A/B runs): "pass_device_walk", "pass_stage_min_bytes", "pass_device_memo",
 * "pass_host_counts", "pass_skip_hash_checks", "pass_timing", "pass_hash_memo" - same convention: 0 the default, > 0 on / the threshold, < 0 off;
 * "audit_permille" (0 .. 1000, FABGPU_EINVAL outside); get also
 * answers "n_devices" and two counters: "registrations_dropped" (key / issuer tables that could not be brought onto every device of the
 * pool after three attempts - those identities verify on the fresh-key kernels / bccsp/idemix) and "registration_id_mismatches".
 * "retire_evicted_keys" (default off; > 0 on): an identity that the identity cache evicts (fabgpu_csp_identity_cache_limits) also gives
 * up its device comb table - fabgpu_p256_key_unregister on every device of the pool, the same keys in the same order everywhere, so
 * the devices keep agreeing on key ids - and a provider whose signers come and go keeps registering the hot ones for as long as it
 * lives, where it otherwise stops after FABGPU_MAX_KEYS registrations.  Keys that came in through fabgpu_csp_key_import are never
 * retired this way.
 * "hash_sha3" (default off; > 0 on): the provider serves the SHA3 hash family on the device - fabgpu_csp_hash answers "SHA3_256"
 * (bccsp.SHA3_256Opts) through fabgpu_sha3_256_batch, and fabgpu_csp_identity_verify_batch2 / _coalesced2 take hash family "SHA3",
 * what identity.Verify selects for an MSP whose SignatureHashFamily is SHA3 (msp/identities.go:216-224).  Off, every answer is what it
 * was: "Unsupported 'HashOpt' provided [SHA3_256]", and family "SHA3" answers that bccsp/sw serves it.  The block pass serves the
 * P-384 tuples of an MSP set SHA3 with fabgpu_csp_msp_hash_family (below; options hash_sha3 and p384 both on).  NOT served either way:
 * the P-256 tuples of a SHA3 MSP in the block pass (the routes hash every P-256 message with SHA-256, so such signatures come back "not
 * valid" from it and their validators' SHA3-256 digests can only miss the verdict memo, never hit a SHA-256 verdict) and the digest
 * memo (SHA-256 only).
 * "p384" (default off; > 0 on): the *_p384 calls below verify ECDSA P-384 identities on the device.  Off, each of them answers, per item,
 * "P-384 is served by bccsp/sw, not by the GPU provider" (the identity call behind identity.Verify's "could not determine the validity of
 * the signature: ") and launches nothing; fabgpu_csp_key_import_p384 answers the same text and registers nothing.  With the option on the
 * block pass verifies P-384 creators and endorsers too (fabgpu_csp_p384_pass_stats below); off, a P-384 endorser stays TX_NEEDS_SW.  A
 * pass with FABGPU_PASS_SEED_MEMO also remembers their verdicts, in a memo of their own (fabgpu_csp_memo_lookup_p384 below).  NOT
 * served either way: the digest memo for P-384 tuples - fabgpu_csp_hash_lookup misses for their messages and the validators hash
 * them on the CPU; that SHA-256 is the digest the verdict entries are keyed on.
 * "p384_wide" (default off; > 0 on): FABGPU_FLAG_P384_WIDE on every context of the pool - keyed P-384 launches of at most 8 192 rows run
 * with eight lanes per signature (fabgpu.h).  It is a context flag: a provider reads it at construction from ctx_flags; set on a living
 * provider, it switches every context for the launches queued from then on (and makes their scratch in that call).  Verdicts, statuses
 * and flags do not depend on it.
 * "p384_key_tables16" (default off; read-only on a living provider): FABGPU_FLAG_P384_KEY_TABLES_16BIT on every context of the pool, read
 * at construction from ctx_flags - every imported P-384 key also gets a 16-bit comb table (144 MiB, at most 32 per context), and the
 * keyed batches of fabgpu_csp_verify_batch_p384, the identity batches, the coalescer and the pass stage run 24 windows on the
 * wavefronts all of whose keys have one (fabgpu.h).  Verdicts, statuses and flags do not depend on it.
 * "sha3_coop" (default off; > 0 on): FABGPU_FLAG_SHA3_COOP on every context of the pool - SHA3-256 launches of at most 4 096 messages run
 * with 32 lanes on a message, larger plain ones take them for their long messages (fabgpu.h).  A context flag like "p384_wide": read at
 * construction from ctx_flags, and set on a living provider it switches every context for the launches queued from then on.  Digests,
 * verdicts and statuses do not depend on it; fabgpu_csp_sha3_coop_rows counts.
 * FABGPU_EINVAL: no such option. */
int fabgpu_csp_set_option(fabgpu_csp* csp, const char* name, int64_t value, int64_t* previous);
int fabgpu_csp_get_option(fabgpu_csp* csp, const char* name, int64_t* value);
/* fabgpu_p256_key_table_stats of device context d, followed by (out[FABGPU_KEY_TABLE_STATS]) the number of keys the provider has
 * retired for evicted identities; returns how many values there are (FABGPU_KEY_TABLE_STATS + 1; the first cap are written). */
int fabgpu_csp_key_table_stats(fabgpu_csp* csp, int d, uint64_t* out, int cap);

/* ---- CPU audit of device results, and poisoning ----
 * Digests and verdicts the provider hands out were computed by kernels; nothing outside the device checks them (a validator that takes
 * its digest from fabgpu_csp_hash_lookup no longer cross-checks the device's SHA-256 with its own).  With audit_permille > 0 the provider
 * re-computes a fixed share of them on the calling thread, in host code, before they are returned:
 *   - fabgpu_csp_hash_lookup hits: SHA-256 of the caller's message;
 *   - fabgpu_csp_memo_lookup hits: bccsp.Verify(k, sig, digest) as bccsp/sw decides it, against stored status 0 / anything else;
 *   - fabgpu_csp_memo_lookup_p384 hits (a kind and a hit counter of their own): ECDSA P-384 over the caller's key, signature and
 *     digest with csrc/p384.h compiled for the host, against stored status 0 / anything else;
 *   - "valid" answers of fabgpu_csp_verify, _verify_batch, _verify_coalesced, _identity_verify_batch, _identity_verify_coalesced
 *     (the identity calls hash the message again first - with SHA3-256, through the kernels' own sha3_256.h compiled for the host, when
 *     the call's hash family is SHA3).  Rejects are not sampled: the Go side re-checks every reject in bccsp/sw.
 *   - idemix pseudonym results, a kind with a hit counter of its own: NymSignature.Ver (idemix/nymsignature.go:74-109) in host code
 *     over FP256BN, under the issuer key's HSk, HRand and Hash as the provider imported them.
 *       fabgpu_csp_idemix_nym_verify_batch: a sampled "valid" is verified again over the caller's message;
 *       fabgpu_csp_memo_lookup_nym: the caller holds only SHA-256(message) but the proof hashes the message itself, so a sampled hit
 *       takes the message from the block copy the digest memo holds (the entry remembers its span: the creator's Envelope.payload),
 *       first checks that its SHA-256 is the digest of the entry, then verifies against stored status 0 / anything else.
 *     A sampled pseudonym result that cannot be audited - the block copy is no longer held (evicted, or the pool refused the copy), or
 *     the provider does not have the issuer's fields - is handed out as it is and counted in out[4].
 * Sampling has no randomness: one hit counter per kind, hit number h (1-based) is audited iff h*permille/1000 != (h-1)*permille/1000 -
 * 1000 audits every hit, 250 exactly every fourth, 0 none.
 * The first disagreement POISONS the provider, for good: one flag shared by every context of the pool and every thread.  The lookup
 * that found it answers a miss (the caller computes for itself); a direct call reports that item with an error text instead of
 * "valid" and returns FABGPU_EPOISONED.  From then on every memo and digest lookup misses; every verify, identity, nym, hash and
 * block-pass entry point returns FABGPU_EPOISONED without launching anything (a direct call that was in flight returns it too: its
 * outputs are not to be used); a pass already in flight finishes but seeds no memo; fabgpu_csp_free still works.  The Go provider
 * serves everything from bccsp/sw from then on.
 * fabgpu_csp_poison poisons by hand (why may be NULL); fabgpu_csp_poisoned returns 1 / 0 and the FIRST reason (why may be NULL).
 * fabgpu_csp_audit_stats: out[0] digest audits, [1] verdict audits, [2] direct-call audits, [3] mismatches, [4] skipped_nym: sampled
 * pseudonym results that could not be audited, [5] nanoseconds spent auditing, [6] pseudonym audits, [7] audits of P-384 verdict-memo
 * hits; returns how many were written (cap < 8: the first cap - a caller that asks for 6 or 7 gets the values it always got). */
int fabgpu_csp_poison(fabgpu_csp* csp, const char* why);
int fabgpu_csp_poisoned(fabgpu_csp* csp, char* why, size_t cap);
int fabgpu_csp_audit_stats(fabgpu_csp* csp, uint64_t* out, int cap);

/* BCCSP.KeyImport for a P-256 public key (bccsp/sw/keyimport.go:103-134; pattern bccsp/pkcs11/pkcs11.go:148-179): checks
 * curve membership and registers the key's comb table on the device (fabgpu_p256_key_register), so that batches whose
 * signers were all imported this way run on the keyed kernels.  err: "" or the Go error text. */
int fabgpu_csp_key_import(fabgpu_csp* csp, const uint8_t* qx32, const uint8_t* qy32, int* on_curve, char* err, size_t errcap);

/* alg == NULL mirrors opts == nil.  "SHA256"; "SHA3_256" with the hash_sha3 option on; anything else: "Unsupported 'HashOpt' provided [..]" */
int fabgpu_csp_hash(fabgpu_csp* csp, const uint8_t* msg, size_t len, const char* alg, uint8_t* digest32, char* err, size_t errcap);

/* BCCSP.Hash for bytes a memo-seeding block pass has ALREADY hashed on the device: the `digest, err := id.msp.bccsp.Hash(msg, hashOpt)` half
 * of identity.Verify (msp/identities.go:173-181 -> bccsp/sw/impl.go:177-194), which the unchanged validators call once per creator /
 * endorsement signature over bytes the pass hashed a moment earlier - 100 MB per 10 000-transaction block.  A pass with
 * FABGPU_PASS_SEED_MEMO keeps the block's bytes in host memory THE LIBRARY owns (the pinned buffer the upload went through anyway; never the
 * caller's buffer) until fabgpu_csp_memo_evict_block, and indexes every signed message by a fingerprint of a few sampled bytes.  The
 * fingerprint only chooses where to look: the stored digest is returned ONLY when every byte of `msg` equals the bytes the device hashed
 * (memcmp; piecewise for prp || endorser, validator_keylevel.go:246-258) - a flipped byte anywhere, another length, an evicted block, a
 * message the device did not hash: miss.
 * Returns 0: hit, digest32 = SHA-256(msg) as the device computed it (the digest the block's verdict-memo entries are keyed on);
 * 1: miss - the caller computes the digest itself (bccsp/sw), always a correct answer.  Never an infrastructure error.  Messages shorter
 * than 64 bytes always miss (one SHA-256 block costs less than the call).  Callers map *bccsp.SHA256Opts (what msp/identities.go:216-224
 * selects for the SHA2 family) to this entry and every other HashOpts to bccsp/sw. */
int fabgpu_csp_hash_lookup(fabgpu_csp* csp, const uint8_t* msg, size_t len, uint8_t* digest32);
/* digest memo counters since the provider was made: lookups answered / left to the CPU; host copies of blocks held right now, their
 * (pinned) bytes, and passes that wanted a copy when the pool was exhausted (any pointer may be NULL) */
int fabgpu_csp_hash_memo_stats(fabgpu_csp* csp, uint64_t* hits, uint64_t* misses, uint64_t* blocks_held, uint64_t* bytes_held, uint64_t* refused);

/* qx == NULL mirrors k == nil.  *valid = 0/1; err = Go error text or "".  *flags bit0: tuple must be decided by bccsp/sw. */
int fabgpu_csp_verify(fabgpu_csp* csp, const uint8_t* qx32, const uint8_t* qy32, const uint8_t* sig, size_t siglen,
                      const uint8_t* digest, size_t dlen, int* valid, int* flags, char* err, size_t errcap);

/* The two one-signature verbs for callers that arrive MANY AT A TIME, each on its own thread: the orderer's Broadcast handlers behind
 * SigFilter (orderer/common/msgprocessor/sigfilter.go:50-80 -> identity.Verify, msp/identities.go:169-196; one goroutine per client
 * stream), the validator pool's bccsp.Verify calls that miss the verdict memo (core/committer/txvalidator/v20/validator.go:198-208).
 * Blocking, same answers and error texts as fabgpu_csp_verify / fabgpu_csp_identity_verify_batch; calls that are in flight at the same
 * moment share ONE launch (a caller that finds the device busy queues behind the running launch and travels with the next; a caller
 * that finds it idle waits window_us - default 50 - for company).  A device failure is FABGPU_ELAUNCH for every caller of that launch,
 * never a verdict.  err == "" means nil. */
int fabgpu_csp_verify_coalesced(fabgpu_csp* csp, const uint8_t* qx32, const uint8_t* qy32, const uint8_t* sig, size_t siglen,
                                const uint8_t* digest, size_t dlen, int* valid, int* flags, char* err, size_t errcap);
int fabgpu_csp_identity_verify_coalesced(fabgpu_csp* csp, const uint8_t* qx32, const uint8_t* qy32, const uint8_t* msg, size_t msglen,
                                         const uint8_t* sig, size_t siglen, char* err, size_t errcap);
/* ... with the MSP's hash family: "SHA2" (what the entry above means) or, with the hash_sha3 option on, "SHA3".  Callers of the two
 * families never share a launch (a queue per family).  Any other string: err = "hash familiy not recognized [<family>]" - the
 * reference's text and spelling (msp/identities.go:223) -, FABGPU_OK, nothing launched. */
int fabgpu_csp_identity_verify_coalesced2(fabgpu_csp* csp, const uint8_t* qx32, const uint8_t* qy32, const uint8_t* msg, size_t msglen,
                                          const uint8_t* sig, size_t siglen, const char* hash_family, char* err, size_t errcap);
/* ---- ECDSA P-384 identities (option "p384"; bccsp/sw accepts P-384 keys exactly as P-256 keys: keyimport.go, ecdsa.go:41-57) ----
 * The argument lists, answers and error texts of fabgpu_csp_verify_coalesced, fabgpu_csp_verify_batch and
 * fabgpu_csp_identity_verify_batch2, with 48-byte key coordinates (qx[i] at qx + 48*i) and the low-S gate against P-384's half order.
 * hash_family: the MSP's ("SHA2"; "SHA3" with the hash_sha3 option on; anything else: "hash familiy not recognized [..]" per item) - the
 * identity call hashes with it (a 32-byte digest enters as a 256-bit e, Go's hashToInt), the digest call only checks it.
 * The coalesced entry has a queue of its own: P-384 callers share launches with each other only.  "valid" answers are sampled by the CPU
 * audit like the P-256 ones (re-computed with csrc/p384.h compiled for the host); a disagreement poisons the provider.
 * *flags bit0 as in fabgpu_csp_verify (the provider does not decide: an off-curve key, or the option is off). */
/* BCCSP.KeyImport for a P-384 public key: fabgpu_csp_key_import's answers and texts with 48-byte coordinates.  An on-curve key gets its
 * comb table on every device of the pool (fabgpu_p384_key_register_many), and the three calls below then take the keyed entries for a
 * batch whose submitted items ALL name imported keys (otherwise the fresh-key entries, as before); answers and texts do not change. */
int fabgpu_csp_key_import_p384(fabgpu_csp* csp, const uint8_t* qx48, const uint8_t* qy48, int* on_curve, char* err, size_t errcap);
int fabgpu_csp_verify_coalesced_p384(fabgpu_csp* csp, const uint8_t* qx48, const uint8_t* qy48, const uint8_t* sig, size_t siglen,
                                     const uint8_t* digest, size_t dlen, int* valid, int* flags, char* err, size_t errcap);
int fabgpu_csp_verify_batch_p384(fabgpu_csp* csp, size_t n, const uint8_t* qx, const uint8_t* qy, const uint8_t* sig_arena, const uint32_t* sig_off,
                                 const uint8_t* dig_arena, const uint32_t* dig_off, const char* hash_family, uint8_t* valid, char* errs,
                                 size_t errstride);
int fabgpu_csp_identity_verify_batch_p384(fabgpu_csp* csp, size_t n, const uint8_t* qx, const uint8_t* qy, const uint8_t* msg_arena,
                                          const uint32_t* msg_off, const uint8_t* sig_arena, const uint32_t* sig_off, const char* hash_family,
                                          char* errs, size_t errstride);
int fabgpu_csp_coalescer_configure(fabgpu_csp* csp, uint32_t window_us, uint32_t max_batch);
int fabgpu_csp_coalescer_stats(fabgpu_csp* csp, uint64_t* calls, uint64_t* launches, uint64_t* largest_batch);

/* n keys (n x 32), ragged signatures and digests; valid: n bytes; errs: n * errstride chars (NUL terminated, truncated). */
int fabgpu_csp_verify_batch(fabgpu_csp* csp, size_t n, const uint8_t* qx, const uint8_t* qy, const uint8_t* sig_arena,
                            const uint32_t* sig_off, const uint8_t* dig_arena, const uint32_t* dig_off, uint8_t* valid,
                            char* errs, size_t errstride);

/* identity.Verify(msg, sig) for n (key, msg, sig) triples; errs[i] == "" means nil. */
int fabgpu_csp_identity_verify_batch(fabgpu_csp* csp, size_t n, const uint8_t* qx, const uint8_t* qy, const uint8_t* msg_arena,
                                     const uint32_t* msg_off, const uint8_t* sig_arena, const uint32_t* sig_off, char* errs,
                                     size_t errstride);
/* ... for identities of an MSP whose hash family is hash_family ("SHA2", "SHA3"; see fabgpu_csp_identity_verify_coalesced2): the digest is
 * SHA3-256(msg) for "SHA3", computed by a launch of its own in front of the verify kernels; keyed when every signer is registered. */
int fabgpu_csp_identity_verify_batch2(fabgpu_csp* csp, size_t n, const uint8_t* qx, const uint8_t* qy, const uint8_t* msg_arena,
                                      const uint32_t* msg_off, const uint8_t* sig_arena, const uint32_t* sig_off, const char* hash_family,
                                      char* errs, size_t errstride);

/* ---- block-level pre-verify pass (extensions/validation/validation.go:48-64 is the hook) ----
 * One fused launch for every signature of a marshalled common.Block:
 *   creator:      SignatureHeader.creator over Envelope.payload            (core/common/validation/msgvalidation.go:258-298)
 *   endorsements: Endorsement.endorser over prp || Endorsement.endorser    (.../statebased/validator_keylevel.go:246-258)
 * Identities (PEM x509, P-256) are imported once and cached (device comb tables), the block buffer is the message arena,
 * each proposal_response_payload is hashed once.  The two other SHA-256 checks of ValidateTransaction ride along in the same
 * submission: CheckTxID (protoutil/proputils.go:366-375) and the proposal hash of every action (protoutil/txutils.go:431-447,
 * core/common/validation/msgvalidation.go:233-241).  tx_flags[t], in the order the reference would reject: 3 not understood
 * (left to the Go validators), 1 creator signature bad, 5 TxID does not match, 6 a proposal hash does not match, 2 an
 * endorsement signature bad, 4 an identity needs bccsp/sw, 0 everything checks.
 * tuple_status[i]: 0..4 as in fabgpu.h, 5 signature does not unmarshal, 6 identity needs bccsp/sw, 7 empty signature.
 * Returns FABGPU_ETOOBIG with *n_tx / *n_tuples set when the caller's arrays are too small. */
int fabgpu_csp_block_preverify(fabgpu_csp* csp, const uint8_t* block, size_t len, uint32_t* n_tx, uint8_t* tx_flags, uint8_t* tx_type,
                               uint32_t cap_tx, uint32_t* n_tuples, uint32_t* tuple_tx, uint8_t* tuple_kind, uint8_t* tuple_status,
                               uint32_t cap_tuples);
/* ---- the pass, second form: verdicts tied to the BYTES they were computed over, the orderers' block signatures, the verdict memo ----
 * Everything fabgpu_csp_block_preverify returns, plus per tuple: the spans of (identity, prefix, suffix, signature) in the virtual arena
 * block || padding || tail (see fabgpu_block_tuples), the SHA-256 digest of the signed message AS THE DEVICE COMPUTED IT, and the
 * P-256 key the identity carries.  A consumer must key on these (never on tuple position): a crafted envelope could make another
 * parser see other bytes; the walker refuses envelopes with repeated singular fields for the same reason (tx_flags = 3).
 * Tuples of kind 2 (tx = 0xFFFFFFFF, listed last) are the orderers' signatures over the block - the SignedData MCS.VerifyBlock hands
 * to the BlockValidation policy (internal/peer/gossip/mcs.go:166-193).  BlockDataHash (one serial SHA-256 over the whole BlockData,
 * protoutil/blockutils.go:65-68) stays with the caller: a single SHA-256 stream cannot be parallelised.
 * FABGPU_PASS_SEED_MEMO: every tuple the device hashed and decided is remembered under `block_seq` as
 * (key X||Y, signature bytes, digest) -> status; fabgpu_csp_memo_lookup answers the bccsp.Verify(k, sig, digest) calls the unchanged
 * validators make afterwards (msp/identities.go:188) and fabgpu_csp_memo_evict_block drops the block's entries when Validate returns. */
#define FABGPU_PASS_SEED_MEMO 1u
#define FABGPU_PASS_NO_BLOCK_SIGS 2u /* do not verify the orderers' block signatures (their tuples report status 8) */
typedef struct fabgpu_block_pass {
    /* in */
    const uint8_t* block;
    size_t len;
    uint64_t block_seq;
    uint32_t flags;              /* FABGPU_PASS_* */
    uint32_t cap_tx, cap_tuples; /* capacity of the arrays below */
    /* out: counts (always set; FABGPU_ETOOBIG when a capacity is too small - nothing was launched) */
    uint32_t n_tx, n_tuples, n_block_sigs, memo_seeded;
    uint32_t tail_base, tail_len;
    uint8_t block_sigs_understood; /* 1: metadata[SIGNATURES] parsed (kind-2 tuples are complete) */
    /* out: arrays, caller-allocated, any may be NULL */
    uint8_t* tx_flags;           /* cap_tx */
    uint8_t* tx_type;            /* cap_tx */
    uint32_t* tuple_tx;          /* cap_tuples */
    uint8_t* tuple_kind;         /* cap_tuples: 0 creator, 1 endorsement, 2 block signature */
    uint8_t* tuple_status;       /* cap_tuples */
    uint32_t* tuple_spans;       /* cap_tuples x 8 */
    uint8_t* tuple_digest;       /* cap_tuples x 32; zero where tuple_hashed[i] == 0 */
    uint8_t* tuple_hashed;       /* cap_tuples */
    uint8_t* tuple_qxy;          /* cap_tuples x 64 */
    uint8_t* tail;               /* tail_cap bytes: the block-signature messages (optional) */
    uint32_t tail_cap;
    /* out: submitted tuples that went through per-key device tables.  Host walk: all of them, or none (one identity without a table
     * sends the block down the fresh-key kernel).  Device walk: per launch class - the creators' launch and the launch of everybody
     * else each take the tables when every one of their submitted tuples has one. */
    uint32_t n_keyed;
    /* out (ABI v5), device walk: tuples whose identity the provider had never met - their certificates were decoded on the device
     * (msp/mspimpl.go:408-421 deserialization: PEM, x509 SubjectPublicKeyInfo, curve membership) and offered to its identity cache */
    uint32_t n_device_decoded;
    /* out (ABI v6): where this pass spent its time, host clock, milliseconds - [0] the outline of the block and the identity table's
     * sync (host walk: the gates), [1] waiting for the block's upload to finish, [2] the device phase (count .. finish, the verify
     * launches inside), [3] bookkeeping behind it (cache, learned identities, memo publication); [4] the device context that served it */
    float ms_stage[4];
    int32_t device_context;
} fabgpu_block_pass;
int fabgpu_csp_block_preverify2(fabgpu_csp* csp, fabgpu_block_pass* pass);
/* FABGPU_ETOOBIG and the retry (both forms of the pass).  The block's upload starts before its shape is known; when the caller's arrays
 * turn out too small the pass returns FABGPU_ETOOBIG with the counts set, NOTHING was launched, and the library keeps the finished upload
 * for the retry.  Contract:
 *  - by the time FABGPU_ETOOBIG is returned the upload has been waited for: the library never reads `block` after a call has returned
 *    (cgo: no Go pointer is retained), so the caller may free or reuse the buffer;
 *  - a retry finds the kept upload only if it passes the same pointer, length and block_seq, a fingerprint of the buffer (its first and
 *    last KiB and 64 samples between them) is unchanged, and it comes within one second; any other call uploads afresh (correct, just
 *    slower).  The caller MUST NOT modify the buffer between the attempts: the fingerprint is a guard against an allocator handing the
 *    same address to another block, not a proof that every byte is the one that was uploaded;
 *  - a caller that will not retry calls fabgpu_csp_block_pass_abandon (returns 1 if an upload was dropped, 0 if none was kept);
 *    otherwise the kept upload is dropped by the next pass that finds it older than a second, and its device counts as busy until then. */
int fabgpu_csp_block_pass_abandon(fabgpu_csp* csp);
/* 0: hit, *status = 0 valid / 1 arithmetic reject / 2 high-S / 3 r out of range (the reference rejects: ask bccsp/sw for its error
 * text); 1: miss -> bccsp/sw.  Never an infrastructure error: a miss is always a correct answer. */
int fabgpu_csp_memo_lookup(fabgpu_csp* csp, const uint8_t* qx32, const uint8_t* qy32, const uint8_t* sig, size_t siglen, const uint8_t* digest,
                           size_t dlen, uint8_t* status);
/* The same for an idemix pseudonym signature (key = Nym.x, Nym.y; digest = SHA-256(message)): entries are bound to the issuer key they
 * were verified under - issuer_hash32 = idemix.IssuerPublicKey.Hash of the key the CALLER verifies under (bccsp.IdemixNymSignerOpts.IssuerPK) -
 * so a verdict reached under one channel's issuer can never answer for another's (two channels may give their idemix MSPs the same id).
 * ECDSA entries and pseudonym entries live in separate key domains. */
int fabgpu_csp_memo_lookup_nym(fabgpu_csp* csp, const uint8_t* issuer_hash32, const uint8_t* nym_x32, const uint8_t* nym_y32, const uint8_t* sig, size_t siglen,
                               const uint8_t* digest, size_t dlen, uint8_t* status);
/* *entries = memo entries still held under block_seq (0: never seeded, evicted, or pushed out by newer blocks).  The pass may run when
 * a block ARRIVES (extensions/gossip/state AddPayload: the marshalled bytes are in hand, gossip/state/state.go:592,785-787) and the
 * validator wrapper asks this before it would marshal and submit the same block again at Validate. */
int fabgpu_csp_memo_has_block(fabgpu_csp* csp, uint64_t block_seq, uint64_t* entries);
int fabgpu_csp_memo_evict_block(fabgpu_csp* csp, uint64_t block_seq, uint64_t* evicted);
int fabgpu_csp_memo_stats(fabgpu_csp* csp, uint64_t* entries, uint64_t* hits, uint64_t* misses, uint64_t* evicted);
int fabgpu_csp_memo_set_capacity(fabgpu_csp* csp, uint64_t max_entries);
/* ---- the verdict memo of the P-384 tuples of a pass (option "p384") ----
 * A pass with FABGPU_PASS_SEED_MEMO on a provider with the option on remembers, under its block_seq, every P-384 tuple its P-384 stage
 * submitted to the device: (key X48 || Y48, signature bytes as they sit in the block, the SHA-256 digest the device verified) -> the
 * status the stage wrote (0, or 1 / 3 / 4 as in fabgpu.h).  The entries live in a table of their own, seeded on the host, beside the
 * P-256 memo: fabgpu_csp_memo_lookup and its table are unchanged and never meet 48-byte coordinates; this lookup never waits for theirs.
 * fabgpu_csp_memo_lookup_p384 answers the bccsp.Verify(k, sig, digest) call of msp/identities.go:188 for a P-384 key with the
 * conventions of fabgpu_csp_memo_lookup: 0 hit, *status set (0 valid; anything else: the reference rejects - ask bccsp/sw for its
 * text) and *block_seq (may be NULL) = the pass that seeded the entry; 1 miss -> the coalesced entry or bccsp/sw.  With the option
 * off, or on a poisoned provider, always a miss.  A key seeded twice answers with its first entry.
 * No entry, so a miss: tuples the stage's host gate decided (empty signature, DER that does not unmarshal, high S, r or s out of range -
 * bccsp/sw owns their error texts), tuples of a key id retired under the launch, identities that are no on-curve P-384 certificate.
 * Lifetime: fabgpu_csp_memo_evict_block(seq) also drops the P-384 record of seq and *evicted counts its entries too;
 * fabgpu_csp_memo_has_block adds them.  The table is bounded by a capacity of its own (default 65 536 entries; the oldest block goes
 * first while it is over; fabgpu_csp_memo_set_capacity does not touch it), and fabgpu_csp_memo_stats stays about the P-256 table:
 * fabgpu_csp_memo_stats_p384 reports this one (any pointer may be NULL).
 * NOT served: bccsp.Hash for these messages (tuple_hashed stays 0, fabgpu_csp_hash_lookup keeps missing: the validators hash them on the
 * CPU; the digest the entries are keyed on is that hash - SHA3-256 for the tuples of an MSP set SHA3, fabgpu_csp_msp_hash_family),
 * fabgpu_multi_*.  The layout of the pass's outputs does not
 * change: tuple_qxy and tuple_digest stay zero for these tuples - they are framed for 32-byte coordinates. */
int fabgpu_csp_memo_lookup_p384(fabgpu_csp* csp, const uint8_t* qx48, const uint8_t* qy48, const uint8_t* sig, size_t siglen, const uint8_t* digest,
                                size_t dlen, uint8_t* status, uint64_t* block_seq);
int fabgpu_csp_memo_stats_p384(fabgpu_csp* csp, uint64_t* entries, uint64_t* hits, uint64_t* misses, uint64_t* evicted);
int fabgpu_csp_memo_set_capacity_p384(fabgpu_csp* csp, uint64_t max_entries);
/* Bounds of the pass's identity cache (identities come out of unvalidated blocks): at most max_identities cached (LRU, like
 * msp/cache), a device comb table only for an identity named register_after_hits times, at most max_registered_keys tables. */
int fabgpu_csp_identity_cache_limits(fabgpu_csp* csp, uint64_t max_identities, uint64_t max_registered_keys, uint32_t register_after_hits);
int fabgpu_csp_identity_cache_size(fabgpu_csp* csp, uint64_t* identities);
/* Both forms of the pass walk a staged block ON THE DEVICE (envelope walk, signature gates - every DER encoding, decided as
 * bccsp/utils/ecdsa.go:43-92 decides it -, identity lookup, certificates of identities nobody has met decoded by a wavefront each,
 * submission arrays, digest comparisons and flags as kernels; block_walk_dev.h).  The host walk answers what is left: blocks that were
 * not staged, blocks on a provider with idemix MSPs, a certificate longer than the device decoder's buffer (3 KiB of DER), a block
 * without any signature for the device to decide. Same answers either way.  The provider option pass_device_walk < 0 keeps every block on the host
 * walk.  This reports how many passes went which way and why the last block was declined by the device walk. */
int fabgpu_csp_pass_routes(fabgpu_csp* csp, uint64_t* device_walks, uint64_t* host_walks, char* last_decline, size_t cap);
/* Device-route statistics since the provider was made: out4[0] verify launches repeated because the prediction "every signer of this
 * launch class has a comb table" (taken from the previous block, so that nothing waits for the gates) did not hold, [1] tuples whose
 * identity was not in the device's table (certificate decoded on the device), [2] identities that entered the cache that way,
 * [3] signatures outside the common DER shape (decided by the general parser, on the device). */
int fabgpu_csp_pass_stats(fabgpu_csp* csp, uint64_t* out4);
/* what the host route makes of a SerializedIdentity: 0 = PEM x509 certificate with an on-curve P-256 key (qxy64 = X || Y), 1 = anything else
 * (pure host; callers that hold identities as bytes - tools/go_call_replay.c - take the key bccsp.KeyImport would have remembered from it) */
int fabgpu_identity_to_p256(const uint8_t* ident, size_t len, uint8_t* qxy64);
/* ... and what the P-384 stage of the pass makes of it: 0 = PEM x509 certificate whose key is id-ecPublicKey on secp384r1 (1.3.132.0.34), a
 * 97-byte uncompressed point ON the curve (qxy96 = X || Y); 2 = such a certificate whose point is not on P-384 (qxy96 set all the same:
 * decoded, refused by the on-curve gate - its tuples stay TUPLE_ST_NEEDS_SW); 1 = anything else (another curve, a compressed point,
 * idemix, truncated bytes).  Pure host. */
int fabgpu_identity_to_p384(const uint8_t* ident, size_t len, uint8_t* qxy96);
/* The P-384 stage of the block pass (option "p384"; with the option off every counter stays 0).  After either route has written the
 * tuples' statuses, the tuples it left TUPLE_ST_NEEDS_SW whose identity is a certificate with an on-curve P-384 key are gated on the host
 * and verified in one described batch over the staged block (fabgpu_identity_verify_batch_p384: the keyed kernel when every submitted
 * key came through fabgpu_csp_key_import_p384, the fresh-key kernel otherwise), their statuses written (0-5, 7 as for P-256 tuples) and
 * the flags of their transactions folded again.  out[0 .. min(cap, 7)): [0] passes that ran the stage, [1] P-384 tuples seen,
 * [2] tuples submitted to the device, [3] keyed launches, [4] fresh-key launches, [5] tuples the CPU audit recomputed (audit_permille;
 * a disagreement poisons the provider and the pass answers FABGPU_EPOISONED), [6] entries seeded into the P-384 verdict memo
 * (FABGPU_PASS_SEED_MEMO; fabgpu_csp_memo_lookup_p384 above; fabgpu_block_pass.memo_seeded includes them), [7] tuples submitted under
 * SHA3-256 (a part of [2]).  Returns how many values there are (8); a caller that passes an older capacity of 6 or 7 still gets the
 * values it always got.
 * Hash family: the tuples of an MSP set SHA3 (fabgpu_csp_msp_hash_family) go out in a described batch of their own through
 * fabgpu_identity_verify_batch_p384_sha3, after the SHA2 tuples' batch over the same staged block - at most two batches a block, each keyed or fresh on
 * its own keys ([3] and [4] count batches); the audit hashes them with SHA3-256 and their memo entries carry the SHA3-256 digest, the
 * one the validator's bccsp.Verify presents.  A block without such a tuple launches what it always launched.
 * NOT in the stage: digest memo entries for P-384 tuples (tuple_hashed = 0, tuple_qxy and tuple_digest zero; bccsp.Hash of their
 * messages stays on the CPU), the P-256 tuples of a SHA3 MSP (hashed with SHA-256 by the routes, answered "not valid", decided in
 * bccsp/sw), fabgpu_multi_*, P-384 keys earning a table by hit count. */
int fabgpu_csp_p384_pass_stats(fabgpu_csp* csp, uint64_t* out, int cap);
/* A ninth value of the stage, read by a call of its own so that fabgpu_csp_p384_pass_stats keeps answering eight: *rows = the tuples of
 * its keyed batches that the eight-lanes-per-signature form verified (the "p384_wide" option; a part of [2]; 0 with the option off, and
 * for every fresh-key batch). */
int fabgpu_csp_p384_pass_wide_rows(fabgpu_csp* csp, uint64_t* rows);
/* *rows = fabgpu_sha3_coop_rows summed over the contexts of the pool: the rows of this provider's SHA3-256 launches (and of anyone else's
 * on its contexts) that were hashed on 32 lanes (the "sha3_coop" option; 0 with the option off). */
int fabgpu_csp_sha3_coop_rows(fabgpu_csp* csp, uint64_t* rows);
/* The hash family of an MSP, as the block pass knows it: what the MSP's setup read from its config's SignatureHashFamily
 * (msp/identities.go:216-224).  family: "SHA2" or "SHA3"; anything else answers 1 with identity.getHashOpt's text in err ("hash familiy
 * not recognized [..]"), and "SHA3" while the hash_sha3 option is off answers 1 with the text that bccsp/sw serves it; an empty mspid or
 * one longer than 1024 bytes answers 1 with "invalid mspid".  0: set (err = "").  Every MSP is SHA2 until set otherwise.  A change holds
 * for the passes that start after the call returns; an MSP set SHA3 counts as SHA3 only while hash_sha3 is on.  Only the P-384 stage
 * reads it.  _get: *sha3 = 1 for an MSP set SHA3, 0 otherwise (also for an MSP nobody has set). */
int fabgpu_csp_msp_hash_family(fabgpu_csp* csp, const char* mspid, const char* family, char* err, size_t errcap);
int fabgpu_csp_msp_hash_family_get(fabgpu_csp* csp, const char* mspid, int* sha3);

/* (An x509 chain-link batch - crypto/x509 CheckSignatureFrom for n certificates - was an entry point of rounds 2-4 WITHOUT a consumer:
 * the only caller on this path is crypto/x509's own Verify (msp/mspimpl.go:721-739), which offers no hook for a pre-computed verdict, and
 * using one as advice would have meant skipping or forking chain building, constraints and expiry.  Removed in round 5) */
/* pure host helpers of the pass (no device): block structure, and the P-256 key of an x509 certificate */
int fabgpu_block_parse(const uint8_t* block, size_t len, uint32_t* n_tx, uint32_t* n_tuples, uint32_t* n_prefixes, uint8_t* tx_type, uint32_t cap_tx,
                       char* channel_id, size_t channel_cap);
int fabgpu_x509_p256_pubkey(const uint8_t* cert, size_t len, int is_pem, uint8_t* qx32, uint8_t* qy32);
/* the hash checks of a block: kind 0 = TxID (expect = 64 hex characters), 1 = proposal hash (expect = 32 bytes); message = the
 * concatenation of the three (start, end) spans; all offsets into the block buffer.  FABGPU_ETOOBIG with *n_checks set if cap is small. */
int fabgpu_block_hash_checks(const uint8_t* block, size_t len, uint32_t cap, uint32_t* n_checks, uint32_t* tx, uint8_t* kind, uint32_t* spans6,
                             uint32_t* expect2);

/* every (identity, message, signature) tuple the pass derives from a block (pure host; tests compare it with an independent decoder
 * and verify the tuples with the CPU oracle).  spans8[8i..8i+7] = (start, length) of identity, prefix, suffix, sig; the signed message is
 * prefix || suffix.  Offsets address the virtual arena  block || zero padding up to *tail_base || tail : the orderers' signatures over the
 * block (kind 2, tx 0xFFFFFFFF; internal/peer/gossip/mcs.go:166-193) sign  Metadata.value || signature_header ||
 * protoutil.BlockHeaderBytes(header)  - bytes the walker has to build, returned in `tail` (may be NULL). kind: 0 creator, 1 endorsement. */
int fabgpu_block_tuples(const uint8_t* block, size_t len, uint32_t cap, uint32_t* n_tuples, uint32_t* tx, uint8_t* kind, uint32_t* spans8,
                        uint8_t* tail, uint32_t tail_cap, uint32_t* tail_len, uint32_t* tail_base);

/* ---- idemix pseudonym signatures (creator signatures of idemix MSPs): host mirror of bccsp/idemix/handlers ----
 * fabgpu_csp_idemix_issuer_import: IssuerPublicKeyImporter.KeyImport (bccsp/idemix/handlers/issuer.go:115-136) for the
 * accelerated part - takes the marshalled idemix.IssuerPublicKey, registers HSk / HRand / Hash on the device.
 * *issuer_id = -1 with err == "": a key the device does not take (the proof inside the key is checked by bccsp/idemix).
 * fabgpu_csp_idemix_nym_verify_batch: NymVerifier.Verify (bccsp/idemix/handlers/nymsigner.go:62-95) over n tuples under one
 * issuer: nym public keys as NymPublicKeyImporter.KeyImport receives them (x || y), marshalled idemix.NymSignature bytes,
 * messages.  valid[i] 0/1; flags[i] bit0: tuple left to bccsp/idemix; errs[i] = Go error text ("" == nil). */
/* An idemix MSP of the channel (msp/idemixmsp.go:99-173): after this call fabgpu_csp_block_preverify also verifies the pseudonym
 * signatures of creators serialized under `mspid` (tuple_status 0 valid / 1 invalid / 6 left to bccsp/idemix).  Registering one MSP id
 * with a SECOND, different issuer key (another channel's MSP of the same name) makes the pass leave that MSP id's creators to
 * bccsp/idemix (status 6): it sees MSP ids, not channels.
 * fabgpu_csp_idemix_msp_register2 names the channel whose config carries the MSP: a channel's LATEST key for an MSP id replaces its earlier
 * one (issuer-key rotation), and the MSP id is ambiguous only while two channels' current keys for it differ.  (..._register = channel "".)
 * A key whose field 10 (Hash) is not HashModOrder of the rest of the key - which is what the reference recomputes and uses,
 * idemix/issuerkey.go:171-182 - is not accelerated (*issuer_id = -1). */
int fabgpu_csp_idemix_msp_register(fabgpu_csp* csp, const char* mspid, const uint8_t* ipk_raw, size_t len, int64_t* issuer_id);
int fabgpu_csp_idemix_msp_register2(fabgpu_csp* csp, const char* channel, const char* mspid, const uint8_t* ipk_raw, size_t len, int64_t* issuer_id);
int fabgpu_csp_idemix_issuer_import(fabgpu_csp* csp, const uint8_t* ipk_raw, size_t len, int64_t* issuer_id, char* err, size_t errcap);
/* 1: the marshalled idemix.IssuerPublicKey is in the encoding golang/protobuf itself produces (known fields only, ascending, single-byte
 * tags, minimal length varints, no empty singular bytes fields; idemix.proto:18-48) - only such a key is accelerated, because only for
 * it the library's issuer hash (the given bytes minus field 10) equals SetHash's (idemix/issuerkey.go:171-182, over the RE-MARSHALLED
 * key).  0: any other encoding (the import entry points then answer *issuer_id = -1 and bccsp/idemix serves the key).  No device needed. */
int fabgpu_idemix_issuer_key_is_canonical(const uint8_t* ipk_raw, size_t len);
int fabgpu_csp_idemix_nym_verify_batch(fabgpu_csp* csp, int64_t issuer_id, size_t n, const uint8_t* nym_arena, const uint32_t* nym_off,
                                       const uint8_t* sig_arena, const uint32_t* sig_off, const uint8_t* msg_arena, const uint32_t* msg_off,
                                       uint8_t* valid, uint8_t* flags, char* errs, size_t errstride);

#ifdef __cplusplus
}
#endif
#endif
