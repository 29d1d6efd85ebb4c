/*
 * fabgpu_testhooks.h - what libfabgpu_testhooks.so exports: probes, walker-against-walker comparisons, the synthetic block generator and
 * the kernel timer.  TEST / BENCH INFRASTRUCTURE, not part of the drop-in boundary: nothing here is declared in the public headers (include/) or exported
 * by libfabgpu.so (tests/test_host_logic.py checks both), and nothing in the product path loads this library.  The functions keep the
 * names they had while they lived in the product library (rounds 1-5).
 */
#ifndef FABGPU_TESTHOOKS_H
#define FABGPU_TESTHOOKS_H
#include "../../include/fabgpu.h"
#include "../../include/fabgpu_bccsp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Duration in milliseconds of the most recent kernel launched through ctx, measured with HIP events on the
 * launch stream.  Only for contexts created with FABGPU_FLAG_TIME_KERNELS; <0 otherwise / if nothing was launched. */
float fabgpu_last_kernel_ms(fabgpu_ctx* ctx);
/* TEST HOOKS: the comb table of registered key `key_id` as it lies on the device (built there since round 6: keytab_kernels.hip), and the
 * table the host builder (p256_tables29.h) makes for a key - 32 windows x 256 entries x 20 words; the two must be byte-identical. */
int fabgpu_test_key_table(fabgpu_ctx* ctx, uint32_t key_id, int32_t* out_words, size_t cap_words);
int fabgpu_test_key_table_host(const uint8_t* qx32, const uint8_t* qy32, int32_t* out_words, size_t cap_words);
/* TEST HOOK: the context's generator comb (80 MiB, built on the device at fabgpu_init since round 6) against the host builder's: the
 * index of the first differing 32-bit word, -1 identical, -2 error */
long long fabgpu_test_gtab_compare_with_host(fabgpu_ctx* ctx);
/* FABGPU_FLAG_KEY_TABLES_16BIT: waits for the queued builds; the number of 16-bit key tables, after key_id's was checked entry for entry against
 * the key's 8-bit table where the two overlap (-1: the key has none, -2: error, -(1000 + w): window w disagrees) */
long long fabgpu_test_key_tables16(fabgpu_ctx* ctx, uint32_t key_id);
/* TEST HOOK: while on, the idemix four-lane form queues its side launch (the fixed-base terms) BEHIND the commitment launch, so that
 * every commitment wavefront gives up on its records and computes the terms itself, and every side wavefront skips its rows. */
void fabgpu_test_nym_side_after(fabgpu_ctx* ctx, int on);
/* TEST HOOK: fabgpu_sha3_256_batch_dev through the 32-lanes-per-message kernel at ANY n, whatever the context's FABGPU_FLAG_SHA3_COOP and
 * SHA3_COOP_MAX say (tools/bench_sha3_coop.py times it beyond the cap, to place the cap); counts no row. */
int fabgpu_test_sha3_coop_batch_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, void* digests, void* stream);
/* TEST HOOK: the capacities in bytes of the block pass's buffers on ctx - per-envelope arrays, per-tuple arrays, pinned staging, host-mapped
 * results, gather scratch (walk_layout.h says what a pass needs of each; walk_preallocate makes the worst case ahead of the first pass). */
void fabgpu_test_walk_buffer_caps(fabgpu_ctx* ctx, uint64_t* out5);


/* Synthetic block generator: n tuples, fresh P-256 keypair per signature, low-S, `invalid_permille`
 * of them mutated (equal parts 1: flipped digest bit, 2: wrong key, 3: s -> n-s, 4: r+1); kind[i] in 0..4 records the
 * mutation.  e_in (n x 32) gives the digests to sign (e.g. SHA-256 of synthetic messages computed by
 * fabgpu_sha256_batch); NULL draws random digests.  e_out receives the digest the verifier should be given (for kind 1
 * it differs from the signed one in one bit; callers in hash mode flip a message bit instead).  Pure host code,
 * deterministic in (seed, n, e_in). */
int fabgpu_synth_batch(size_t n, uint64_t seed, uint32_t invalid_permille, const uint8_t* e_in, uint8_t* qx, uint8_t* qy,
                       uint8_t* e_out, uint8_t* r, uint8_t* s, uint8_t* kind, int threads);


/* TEST HOOK: the device walker against the host walker on one block, record for record.  0 identical (*declined = 1: the device walk
 * declined the block, `diff` says why), 1 they differ (`diff` says where). */
int fabgpu_csp_block_walk_compare(fabgpu_csp* csp, const uint8_t* block, size_t len, int* declined, char* diff, size_t cap);
/* TEST HOOKS (pure host, no device): the device walk's two-run procedure (count, prefix sum, write) carried out serially on the host
 * and compared with the host walker (0 identical, 1 different, FABGPU_EINVAL framing refused); the device's signature gate (0 submit,
 * 1 high-S, 2 empty, 3 declined: the general parser decides); the identity-table hash. */
int fabgpu_block_walk_twopass_compare(const uint8_t* block, size_t len, char* diff, size_t cap);
int fabgpu_gate_sig_fast(const uint8_t* sig, size_t len, uint8_t* r32, uint8_t* s32);
/* ... and the gate the device route applies to every signature (the fast gate, then the general parser for what that declines):
 * 0 submit (r32 / s32 set), 1 high-S, 2 empty, 4 does not unmarshal or r, s <= 0, 5 r of more than 256 bits ((false, nil)) */
int fabgpu_gate_sig_any(const uint8_t* sig, size_t len, uint8_t* r32, uint8_t* s32);
/* TEST HOOK (device): the device route's identity decoder (one wavefront per identity) over n identities = arena[spans[2i], spans[2i+1]):
 * code 0 P-256 key (key[64 i ..] = X || Y), 1 not such an identity, 2 undecided (left to the host) */
int fabgpu_csp_idfix_probe(fabgpu_csp* csp, uint32_t n, const uint8_t* arena, size_t arena_len, const uint32_t* spans, uint8_t* code, uint8_t* key);
/* TEST HOOK (device): the same gate in the wavefront form the kernels run, over n signatures = arena[spans[2i], spans[2i+1]) */
int fabgpu_csp_gate_probe(fabgpu_csp* csp, uint32_t n, const uint8_t* arena, size_t arena_len, const uint32_t* spans, uint8_t* code, uint8_t* r, uint8_t* s);
uint64_t fabgpu_identity_table_hash(const uint8_t* p, size_t len);
/* TEST HOOKS (pure host): the provider's CPU audit (audit_host.h): its SHA-256; its bccsp.Verify over a P-256 key, a DER signature and a
 * digest of any length (1 accept, 0 reject); its sampling rule over n_hits simulated hits of one counter (audited[h - 1] = 1 where hit
 * h is audited; returns the number of audited hits) */
void fabgpu_test_audit_sha256(const uint8_t* msg, size_t len, uint8_t* out32);
int fabgpu_test_audit_p256_verify(const uint8_t* qx32, const uint8_t* qy32, const uint8_t* sig_der, size_t siglen, const uint8_t* digest, size_t dlen);
long long fabgpu_test_audit_sample(uint32_t permille, uint32_t n_hits, uint8_t* audited);
/* ... and its NymVerifier.Verify over an issuer's HSk, HRand and Hash (32-byte halves), a pseudonym, a marshalled idemix.NymSignature and
 * the message (1 accept, 0 reject) */
int fabgpu_test_audit_nym_verify(const uint8_t* hsk_x32, const uint8_t* hsk_y32, const uint8_t* hrand_x32, const uint8_t* hrand_y32, const uint8_t* ipk_hash32,
                                 const uint8_t* nym_x32, const uint8_t* nym_y32, const uint8_t* sig, size_t siglen, const uint8_t* msg, size_t msglen);
/* TEST HOOK: corrupts one entry of the memo table published under block_seq - host memory of the library, nothing is launched.  kind 0
 * flips one bit of the index-th stored digest, kind 1 toggles the index-th stored status between valid and bad-signature (a pseudonym
 * entry's: between valid and proof-invalid), kind 2 flips one bit of the first byte of the message the index-th entry remembers, in the
 * held copy of the block.  0 done, 1 nothing to corrupt (no such table, no digest memo / no held copy, a status that is neither), FABGPU_EINVAL. */
int fabgpu_csp_test_memo_corrupt(fabgpu_csp* csp, uint64_t block_seq, int kind, uint32_t index);
/* TEST HOOK: the provider reads the next `count` arithmetic rejects (status 1) the device gives in fabgpu_csp_verify_batch_p384 /
 * _verify_coalesced_p384 as "valid": a corrupted P-384 verdict, which the sampled audit has to catch. */
int fabgpu_csp_test_p384_corrupt(fabgpu_csp* csp, uint32_t count);
/* TEST HOOK: the index-th entry of the P-384 verdict memo's record under block_seq - entries are in the order the pass's P-384 stage
 * submitted their tuples - gets status 0 where it held a reject: what fabgpu_csp_memo_lookup_p384 would then hand out as "valid", and
 * what its sampled audit has to catch.  Host memory of the library, nothing is launched.  0 done, 1 nothing to corrupt (no such
 * record, or the entry is valid already), FABGPU_EINVAL. */
int fabgpu_csp_test_p384_memo_corrupt(fabgpu_csp* csp, uint64_t block_seq, uint32_t index);
/* TEST HOOK (no device, no provider): what the *_p384 calls of a provider answer per item while its p384 option is off. */
const char* fabgpu_test_p384_refusal_text(void);
/* TEST HOOK: the allocator of key slots and ids by itself (csrc/key_slots.h; no device, no context).  gen_last: the last generation a
 * slot may reach (0xFFFFF in the product).  register: the id of the next registration, or -1 when no slot can be had; a lowest slot
 * that is still draining is waited for, i.e. drained on the spot and counted.  retire: 0 retired, 1 not live.  drain: what a context
 * does once a retired slot's events have completed (1 if the slot was draining).  stats: live, draining, reused, parked, slots ever
 * used, registrations that had to wait. */
void* fabgpu_test_key_slots_new(uint32_t gen_last);
void fabgpu_test_key_slots_free(void* h);
long long fabgpu_test_key_slots_register(void* h);
int fabgpu_test_key_slots_retire(void* h, uint32_t key_id);
int fabgpu_test_key_slots_drain(void* h, uint32_t slot);
void fabgpu_test_key_slots_stats(void* h, uint64_t* out6);


/* TEST HOOKS, registered P-384 keys.  key_table: the comb table of key `key_id` (generator != 0: of the generator) as it lies on the
 * device - 48 windows x 256 entries x 24 words; key_table_host: the table the host builder (p384_tables.h) makes for a key (qx48 or
 * qy48 NULL: for the generator) - the two must be byte-identical.  verify_keyed_host: p384_tables.h verify_keyed_host over two such
 * tables in 16-byte aligned host memory (status 0 .. 4).  key_register_batch: n keys (qxy: n x 96 bytes) registered with one build. */
int fabgpu_test_p384_key_table(fabgpu_ctx* ctx, uint32_t key_id, int generator, uint32_t* out_words, size_t cap_words);
int fabgpu_test_p384_key_table_host(const uint8_t* qx48, const uint8_t* qy48, uint32_t* out_words, size_t cap_words);
int fabgpu_test_p384_verify_keyed_host(const uint32_t* gcomb, const uint32_t* qcomb, const uint8_t* e48, const uint8_t* r48, const uint8_t* s48, int key_ok);
int fabgpu_test_p384_key_register_batch(fabgpu_ctx* ctx, int n, const uint8_t* qxy, uint32_t* key_ids);
/* ... their 16-bit tables (FABGPU_FLAG_P384_KEY_TABLES_16BIT; csrc/p384_tables16.h).  tables16_wait: every queued 16-bit build is waited
 * for and published; returns the number of live 16-bit tables.  tables16_cap: the cap on live 16-bit tables (<= FABGPU_P384_MAX_TABLES16)
 * for the registrations that follow.  key_table16: after the same wait, *bad = how many of the 24 x 65 536 entries of the key's (generator
 * != 0: the generator's) 16-bit table differ from T8[2 w][lo] + T8[2 w + 1][hi], recomputed on the device by the complete Jacobian
 * addition and compared projectively; out_words (NULL, or three windows' words): windows 0, 11 and 23 as they lie on the device.
 * 1: the key has no 16-bit table.  key_table16_host: windows [w_begin, w_end) as the host builder makes them from an 8-bit table of
 * key_table_host (16-byte aligned). */
int fabgpu_test_p384_tables16_wait(fabgpu_ctx* ctx);
int fabgpu_test_p384_tables16_cap(fabgpu_ctx* ctx, uint32_t cap);
int fabgpu_test_p384_key_table16(fabgpu_ctx* ctx, uint32_t key_id, int generator, uint64_t* bad, uint32_t* out_words, size_t cap_words);
int fabgpu_test_p384_key_table16_host(const uint32_t* tab8, uint32_t w_begin, uint32_t w_end, uint32_t* out_words, size_t cap_words);
/* ... and a context's book of P-384 keys by itself (csrc/p384_keys.h; no device): register - the id of `name96` (the one it has, or
 * a new one: a slot still draining is drained on the spot; -1 when no slot can be had) with an opaque tag in the table's place; retire -
 * 0 retired (*tab_tag: the tag the slot held), 1 not live; snapshot - what a keyed launch would be handed, per slot the tag (0: none)
 * and the generation (0xFFFFFFFF: none); returns the high-water mark. */
void* fabgpu_test_p384_book_new(uint32_t gen_last);
void fabgpu_test_p384_book_free(void* h);
long long fabgpu_test_p384_book_register(void* h, const uint8_t* name96, uint64_t tab_tag);
long long fabgpu_test_p384_book_lookup(void* h, const uint8_t* name96);
int fabgpu_test_p384_book_retire(void* h, uint32_t key_id, uint64_t* tab_tag);
int fabgpu_test_p384_book_snapshot(void* h, uint64_t* tab_tags, uint32_t* gens, int cap);

#ifdef __cplusplus
}
#endif
#endif
