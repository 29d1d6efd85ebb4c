// Launch entry points of kernels.hip (host side).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace fab {
// The device's array of key tables: KTAB_STRIDE 8-byte words (one 32-byte line) per SLOT.  [4 k] the 8-bit comb of slot k's tenant (CombTab<8>,
// 640 KiB), [4 k + 1] its 16-bit comb (80 MiB) or nullptr, [4 k + 2] the tenant's generation in the low 32 bits (KTAB_GEN_NONE while the
// slot is between two tenants), [4 k + 3] unused.  A key id is generation << KEY_SLOT_BITS | slot (key_slots.h); a row whose id names a
// slot >= nkeys or another generation than the slot's answers status 4 and reads no table of the slot.
constexpr int KTAB_STRIDE = 4;
constexpr int KEY_SLOT_BITS = 12;
constexpr uint32_t KTAB_GEN_NONE = 0xFFFFFFFFu;      // no id carries it: generations have 32 - KEY_SLOT_BITS bits
constexpr int VERIFY_BLOCK = 256;         // 4 wavefronts per workgroup, one per SIMD
constexpr int VERIFY_MAX_WGS = 256;       // persistent workgroup slots: one per CU (see kernels.hip for why not two)
constexpr int VERIFY_PAIR_MAX = 32768;    // up to here two lanes per signature (one round of 256 workgroups x 128 signatures)
// workspace of the per-lane j*Q tables: 16 entries x 8 uint4 (one 128-byte line each; seven cells used) per lane or per signature
constexpr size_t QWS_UINT4_PER_LANE = (size_t)16 * 8;
constexpr size_t QWS_PAIR_UINT4_PER_SIG = (size_t)16 * 8;

// Shared message prefixes of a fused batch (device pointers): prefix p = arena[pre_off[p], pre_off[p+1]), message i continues
// prefix pre_idx[i] (0xFFFFFFFF = none); mid_scratch: m x 32 bytes for the mid-states.  m = 0 / pre_idx = nullptr: no prefixes.
struct ShaPrefixArgs {
    uint32_t m = 0;
    const void* pre_off = nullptr;
    const void* pre_idx = nullptr;
    void* mid_scratch = nullptr;
    bool spans = false;   // off / pre_off hold (start, end) pairs
    void* digests = nullptr;   // optional out (device): n x 32 bytes, the digest of every message
    bool mid_ready = false;    // the mid-states are already in mid_scratch (launch_sha256_midstates ran, e.g. on another stream)
    // Bytes of (unused) dynamic LDS to request with the launch.  More than half a CU's 160 KB keeps a second workgroup - of this or of
    // any other kernel - off the CU: two launches that run side by side on two streams then land on DISJOINT CUs instead of sharing
    // SIMDs (two waves on a SIMD take 1.5x the time each; the dispatcher fills a CU that still has room before it moves on).
    uint32_t lds_reserve = 0;
};
struct VerifyGeom {
    uint32_t block;   // threads per workgroup
    uint32_t wgs;     // workgroups launched (= workspace slots)
    bool pair;        // two lanes per signature
};
VerifyGeom verify_geom(uint32_t n, bool allow_pair);
size_t verify_workspace_bytes(uint32_t n, bool allow_pair);
int pair_table_default();
size_t pair_table_lds_bytes();        // dynamic LDS one workgroup of the LDS-table pair kernel (helper-wave form) asks for
size_t pair_table_lds_solo_bytes();   // ... of its one-wave-per-SIMD form (FABGPU_FLAG_PAIR_SOLO)
constexpr int PAIR_TABLE_LDS_FROM = 16384;   // launches of more tuples than this keep the pair kernel's per-signature table in LDS
// the mid-state kernel of a prefixed batch alone (a fused launch_verify runs it itself unless pa.mid_ready)
hipError_t launch_sha256_midstates(const void* arena, size_t arena_bytes, const ShaPrefixArgs& pa, hipStream_t st);   // honours pa.lds_reserve
hipError_t launch_sha256_batch(uint32_t n, const void* arena, size_t arena_bytes, const void* off, void* digests, hipStream_t st, uint32_t lds_spread = 0);
// n messages given as (start, end) pairs -> n x 32 digest bytes
hipError_t launch_sha256_spans(uint32_t n, const void* arena, size_t arena_bytes, const void* spans, void* digests, hipStream_t st,
                               uint32_t lds_reserve = 0, uint32_t lds_spread = 0);   // lds_spread: for the eight-lane road (n <= SHA_COOP_MAX, no lds_reserve)
// gathered messages (pieces of the arena stitched into `scratch` at out_off[j] .. out_off[j+1]) -> n x 32 digest bytes
hipError_t launch_gather_sha256(uint32_t n, const void* arena, size_t arena_bytes, const void* spans, const void* out_off, void* scratch,
                                size_t scratch_bytes, void* digests, hipStream_t st, uint32_t lds_reserve = 0, uint32_t lds_spread = 0);
// One ECDSA P-256 verify launch, by field name.  Two pairs of alternatives, exactly one of each named (launch_verify returns
// hipErrorInvalidValue otherwise): the key fresh or registered, the digest given or hashed from the message in the same kernel.
struct VerifyLaunch {
    uint32_t n = 0;
    const void *qx = nullptr, *qy = nullptr;          // fresh key: n x 32 bytes each ...
    void* qws = nullptr;                              // ... and verify_workspace_bytes(n, allow_pair) bytes for the per-signature tables
    const void *key_id = nullptr, *ktabs = nullptr;   // or registered key: n ids into the device's array of key tables (KTAB_STRIDE) ...
    uint32_t nkeys = 0;                               // ... of nkeys slots (the high-water mark: retired slots stay below it)
    const void* e = nullptr;                          // digest given: n x 32 bytes
    const void *arena = nullptr, *off = nullptr;      // or messages: arena[off[i], off[i+1]), possibly behind shared prefixes (pa; the
    size_t arena_bytes = 0;                           // mid-state kernel runs first unless pa.mid_ready)
    ShaPrefixArgs pa;
    const void *r = nullptr, *s = nullptr, *gtab = nullptr;
    void *verdict_bits = nullptr, *status = nullptr;  // status: optional
    bool allow_pair = false;                          // two lanes per signature up to VERIFY_PAIR_MAX
    uint32_t lds_reserve = 0;                         // see ShaPrefixArgs; a launch that hashes takes pa.lds_reserve instead
    // fresh key, digest given, two lanes per signature only:
    int table_lds = 0;                                // the per-signature table: 1 PairQTabLds, 0 global workspace, -1 by size (PAIR_TABLE_LDS_FROM)
    bool pair_solo = false;                           // LDS table: the one-wave form instead of the helper-wave form
    bool pair_dbl1 = false;                           // LDS table: the per-doubling loop instead of the four-doubling program
    bool pair_table_add = false;                      // LDS table, all-odd digits: the odd multiples by general additions instead of co-Z additions
    bool pair_booth4 = false;                         // LDS table: Booth digits over j*Q, 65 windows, instead of all-odd digits over odd multiples, 63
};
hipError_t launch_verify(const VerifyLaunch& v, hipStream_t st);

// ---- wide_kernels.hip: a registered key's verification on eight lanes per signature, in two phases (p256_wide29.h) ----
// For launches of at most WIDE_LAUNCH_MAX signatures (they cannot fill the chip: their time is one wavefront's instruction stream).
// pre: everything that does not need the digest (w = s^-1, u2 = r w, T = u2 Q) -> 144 bytes of scratch per signature; it can run while the
// messages are still being hashed.  post: e = the 32-byte digests by row -> verdict bits (ceil(n / 64) words, written bytewise) and status.
constexpr int WIDE_LAUNCH_MAX = 8192;
constexpr size_t WIDE_SCRATCH_BYTES = 144;
// lds_spread: how many wavefronts of the small launches a CU should take at most - spread_waves_per_cu(the wavefronts that run at the same
// time, over all launches that do) = 1, 2, 4, 8 or SPREAD_NONE; a launch turns it into unused dynamic LDS per workgroup
// (wide_kernels.hip "PLACEMENT").  0 = from this launch's own wavefront count.
constexpr uint32_t SPREAD_NONE = 0xFFFFFFFFu;
uint32_t spread_waves_per_cu(uint32_t wavefronts);
hipError_t launch_p256_wide_pre(uint32_t n, const void* key_id, uint32_t nkeys, const void* ktabs, const void* r, const void* s, const void* gtab,
                                void* scratch, hipStream_t st, uint32_t lds_spread = 0);
hipError_t launch_p256_wide_post(uint32_t n, const void* e, const void* r, const void* gtab, const void* scratch, void* verdict_bits, void* status,
                                 hipStream_t st, uint32_t lds_spread = 0);
// SHA-256 of n (possibly prefixed: pa.mid_scratch must hold the mid-states) messages -> pa.digests (n x 32 bytes), one message per lane
hipError_t launch_sha256_messages(uint32_t n, const void* arena, size_t arena_bytes, const void* off, const ShaPrefixArgs& pa, hipStream_t st);
// The same digests with eight lanes on a message (sha256_coop.h) and NO mid-states: a prefixed message is hashed whole.  For launches that
// cannot fill the chip - SHA_COOP_MAX messages are 256 wavefronts; launch_sha256_batch / _spans (without an LDS reservation) take this road
// by themselves up to that size.
constexpr uint32_t SHA_COOP_MAX = 2048;
// Larger launches: one lane per message, except that messages well above the launch's average length (a quarter above arena_bytes / n,
// at least 2 KiB) are hashed on eight lanes each - at most eight per 64 messages - by wavefronts of their own inside the same launch
// (wide_kernels.hip sha256_mixed_kernel).  pairs: off holds (start, end) pairs instead of n + 1 consecutive offsets.  lds_reserve: see
// ShaPrefixArgs.
hipError_t launch_sha256_mixed(uint32_t n, const void* arena, size_t arena_bytes, const void* off, bool pairs, void* digests, hipStream_t st,
                               uint32_t lds_reserve = 0);
hipError_t launch_sha256_messages_coop(uint32_t n, const void* arena, size_t arena_bytes, const void* off, const ShaPrefixArgs& pa, hipStream_t st,
                                       uint32_t lds_spread = 0);

// ---- sha3_kernels.hip: SHA3-256 (sha3_256.h), one message per lane at every size ----
// A mid-state is the whole 200-byte Keccak state: pa.mid_scratch must be m x SHA3_MID_BYTES (8-byte aligned) for these three.
constexpr size_t SHA3_MID_BYTES_HOST = 200;
hipError_t launch_sha3_256_midstates(const void* arena, size_t arena_bytes, const ShaPrefixArgs& pa, hipStream_t st);
// n (possibly prefixed: the mid-states must be in pa.mid_scratch) messages -> pa.digests (n x 32 bytes)
hipError_t launch_sha3_256_messages(uint32_t n, const void* arena, size_t arena_bytes, const void* off, const ShaPrefixArgs& pa, hipStream_t st);
// spans: off holds (start, end) pairs instead of n + 1 consecutive offsets
hipError_t launch_sha3_256_batch(uint32_t n, const void* arena, size_t arena_bytes, const void* off, bool spans, void* digests, hipStream_t st);
int warm_kernel_functions_sha3();

// ---- sha3_coop_kernels.hip: SHA3-256 with 32 lanes on a message (sha3_coop.h), behind FABGPU_FLAG_SHA3_COOP ----
// The contract of launch_sha3_256_messages for launches that cannot fill the chip: two messages a wavefront, a prefixed message hashed
// whole - NO mid-states are read, pa.mid_scratch may be null and is not written.  A reversed span hashes as empty.  The largest launch the
// context's call sites give it is SHA3_COOP_MAX messages: the largest power of two at which tools/bench_sha3_coop.py measured its median
// at or below the one-lane kernel's (profiles/sha3_coop.json).
constexpr uint32_t SHA3_COOP_MAX = 4096;
hipError_t launch_sha3_256_messages_coop(uint32_t n, const void* arena, size_t arena_bytes, const void* off, const ShaPrefixArgs& pa, hipStream_t st);
// Larger plain launches: one lane per message (sha3_256_stream), except that messages well above the launch's average length (a quarter
// above arena_bytes / n, at least 2 KiB, as launch_sha256_mixed) are hashed on 32 lanes each - at most two per 64 messages - by wavefronts
// of their own inside the same launch.  pairs: off holds (start, end) pairs.  coop_rows (optional, device): += the rows hashed on 32 lanes.
hipError_t launch_sha3_256_mixed(uint32_t n, const void* arena, size_t arena_bytes, const void* off, bool pairs, void* digests, void* coop_rows,
                                 hipStream_t st);
int warm_kernel_functions_sha3_coop();

// ---- p384_kernels.hip: ECDSA P-384 verification (p384.h), one signature per lane, fresh keys only ----
struct P384Launch {
    uint32_t n = 0;
    const void *qx = nullptr, *qy = nullptr, *r = nullptr, *s = nullptr;   // n x 48 bytes each, big-endian
    const void* e = nullptr;                 // n x 48 bytes (hashToInt done), or n x 32 bytes of digests of a 256-bit hash family ...
    bool e_is_digest32 = false;              // ... which Go's hashToInt takes as a 256-bit integer
    const void* gtab = nullptr;              // P384_GTAB_WORDS words: j G, j = 1 .. 15 (p384.h build_gtab)
    void* qws = nullptr;                     // p384_workspace_bytes(n) bytes for the per-signature tables
    void* verdict_bits = nullptr;            // ceil(n/64) x u64
    void* status = nullptr;                  // n bytes or nullptr
};
size_t p384_workspace_bytes(uint32_t n);
hipError_t launch_p384_verify(const P384Launch& v, hipStream_t st);

// ---- p384_keytab_kernels.hip / p384_keyed_kernels.hip: registered P-384 keys (p384_tables.h) ----
// comb tables built on the device (qxy: n_keys x 96 bytes, tabs: n_keys table addresses, both in device memory; see the unit's header)
size_t p384_keytab_scratch_bytes(uint32_t n_keys);
hipError_t launch_p384_keytab_build(uint32_t n_keys, const void* qxy, void* const* tabs, void* scratch, hipStream_t st);
// the optional 16-bit table (p384_tables16.h CombTab384x16, 144 MiB) of ONE key from its finished 8-bit table; both 16-byte aligned, on the device
hipError_t launch_p384_keytab16_build(const void* tab8, void* tab16, hipStream_t st);
// (test hooks) *bad, a zeroed u64 on the device, += the entries of tab16 that are not T8[2 w][lo] + T8[2 w + 1][hi], recomputed another way
hipError_t launch_p384_keytab16_check(const void* tab8, const void* tab16, void* bad, hipStream_t st);
struct P384SlotSnap;   // p384_keys.h: one slot of a keyed launch's snapshot of the context's P-384 keys (table, generation)
struct P384KeyedLaunch {
    uint32_t n = 0;
    const void* key_id = nullptr;            // n x u32: generation << KEY_SLOT_BITS | slot
    const void *r = nullptr, *s = nullptr;   // n x 48 bytes each, big-endian
    const void* e = nullptr;                 // n x 48 bytes, or n x 32 bytes of digests (e_is_digest32), as P384Launch takes them
    bool e_is_digest32 = false;
    const void* gcomb = nullptr;             // the generator's comb table (CombTab384)
    const P384SlotSnap* snap = nullptr;      // nkeys slots in device memory, complete before the launch is queued and never edited
    uint32_t nkeys = 0;                      // the high-water mark the snapshot was taken at
    void* verdict_bits = nullptr;            // ceil(n/64) x u64
    void* status = nullptr;                  // n bytes or nullptr
    void* wide_scratch = nullptr;            // launch_p384_verify_keyed_wide only: n x P384_WIDE_SCRATCH_BYTES, 4-byte aligned, the launch's own until it has run
    // launch_p384_verify_keyed only, all three or none (none: the 8-bit kernel, as without the option): the generator's 16-bit table, per
    // slot of the snapshot the key's finished 16-bit table or null (nkeys addresses, part of the same snapshot), and the device counter
    // (u64) that grows by the rows of the wavefronts that ran 24 windows
    const void* gcomb16 = nullptr;
    const void* const* snap16 = nullptr;
    void* rows16 = nullptr;
};
hipError_t launch_p384_verify_keyed(const P384KeyedLaunch& v, hipStream_t st);
// ---- p384_wide_kernels.hip: the same verification on eight lanes per signature, in two launches on st (p384_wide.h) ----
// For launches of at most P384_WIDE_LAUNCH_MAX rows (hipErrorInvalidValue beyond); the same rows, ids, snapshot rule, verdict words and
// status bytes as launch_p384_verify_keyed.
constexpr uint32_t P384_WIDE_LAUNCH_MAX = 8192;
constexpr size_t P384_WIDE_SCRATCH_BYTES = 100;   // per row between the phases: u1, u2, the early status
hipError_t launch_p384_verify_keyed_wide(const P384KeyedLaunch& v, hipStream_t st);

// ---- p384_described_kernels.hip: the SHA-256 digest rows of a described batch, for the E32 form of the two P-384 verify kernels ----
// Message i = prefix pa.pre_idx[i] (if any) || the span off names: arena bytes below tail_base, tail[offset - tail_base] at or above it.
// The mid-states of the prefixes (pa.mid_scratch, m x 32 bytes) are made by launch_sha256_midstates on the same stream unless pa.mid_ready.
// arena and tail are 4-byte aligned, arena_bytes is a multiple of 4 and the tail is readable up to its last dword (hipErrorInvalidValue
// otherwise for what the host can see); pa.digests is ignored, the rows go to `digests`.
struct P384DescribedLaunch {
    uint32_t n = 0;
    const void* arena = nullptr;
    size_t arena_bytes = 0;
    const void* off = nullptr;               // n + 1 offsets, or (pa.spans) n (start, end) pairs
    ShaPrefixArgs pa;
    const void* tail = nullptr;              // device memory, or nullptr: no tail
    uint32_t tail_base = 0, tail_len = 0;
    void* digests = nullptr;                 // n x 32 bytes
};
hipError_t launch_p384_described_digests(const P384DescribedLaunch& v, hipStream_t st);
// ---- p384_described_sha3_kernels.hip: the same rows under SHA3-256, for the batch of an MSP of the SHA3 hash family ----
// The same description and conditions; the mid-states (pa.mid_scratch, m x SHA3_MID_BYTES_HOST bytes, 8-byte aligned) are made by
// launch_sha3_256_midstates on the same stream unless pa.mid_ready.
hipError_t launch_p384_described_sha3_digests(const P384DescribedLaunch& v, hipStream_t st);

// ---- idemix_kernels.hip: idemix pseudonym signatures on FP256BN ----
// A registered issuer occupies one slot of idemix_issuer_dev_bytes() bytes in a device array; fill a host copy of the slot
// with idemix_issuer_dev_fill (device pointers of the two comb tables + ipk.Hash) and copy it up.
size_t idemix_issuer_dev_bytes();
void idemix_issuer_dev_fill(void* host_slot, const void* d_hsk, const void* d_hrand, const uint8_t hash32[32]);
// one signature per lane; (allow_split and n <= VERIFY_PAIR_MAX) two lanes per signature; (allow_split, allow_quad and
// n <= IDEMIX_QUAD_MAX) four lanes per signature, every point operation on a lane pair; workspace: idemix_workspace_bytes
constexpr int IDEMIX_QUAD_MAX = 16384;     // 256 workgroups x 64 signatures: one round of the chip
// a second stream for the fixed-base terms of the four-lane form (idemix_nym_comb_quad_kernel runs beside the commitment kernel) and the
// two events that fork it off the caller's stream and join it again; owned by the caller (fabgpu_ctx keeps one per workspace slot)
// The fixed-base terms of the idemix four-lane form run on a side stream BESIDE the commitment launch only while that launch leaves
// SIMDs free: at 12 288 signatures it occupies 768 of the chip's 1 024; beyond, the side launch cannot be co-resident, the commitment
// wavefronts spin for records that are not coming and then compute the terms themselves.  Measured (round 6,
// tools/bench_cfg5_mixed.py, idemix alone): 10 000 signatures 0.745 ms with the side stream / 0.810 without; 16 000: 1.010 / 0.815.
constexpr uint32_t NYM_SIDE_STREAM_MAX = 12288;
struct NymSide {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool test_side_after = false;   // TEST HOOK: order the side launch behind the commitment launch (both halves of the fallback, deterministically)
};
hipError_t launch_idemix_nym_verify(uint32_t n, const void* arena, size_t arena_bytes, const void* off, const void* issuer_id, const void* issuers,
                                    uint32_t n_issuers, const void* nym_x, const void* nym_y, const void* proof_c, const void* s_sk,
                                    const void* s_rnym, const void* nonce, void* qws, void* verdict_bits, void* status, bool allow_split,
                                    bool allow_quad, bool spans, hipStream_t st,    // spans: off = n x (start, end) instead of n + 1 running offsets
                                    const void* gather = nullptr,                 // gather: row i takes its inputs from row gather[i] (uint32; ~0 = an idle row)
                                    uint32_t lds_reserve = 0,                     // unused LDS asked for: keeps other reserving kernels off this one's CUs
                                    bool two_phase = true,                        // four-lane form: commitments, then the challenges with eight lanes on a message
                                    const NymSide* side = nullptr);               // ... and the fixed-base terms beside the commitments on this stream
// every LANE owns a 16-entry table in the one- and two-lane geometries, every lane PAIR in the four-lane one
size_t idemix_workspace_bytes(uint32_t n, bool allow_split, bool allow_quad);
// every kernel function of a translation unit resolved now instead of at its first launch (GPUCSP::Preallocate); returns how many
int warm_kernel_functions_kernels();
int warm_kernel_functions_wide();
int warm_kernel_functions_idemix();
int warm_kernel_functions_walk();
int warm_kernel_functions_keytab();
// keytab_kernels.hip: comb tables of registered P-256 keys built on the device (qxy, tabs: device memory; see the unit's header)
size_t keytab_scratch_bytes(uint32_t n_keys);
hipError_t launch_keytab_build(uint32_t n_keys, const void* qxy, void* const* tabs, void* scratch, hipStream_t st);
// ... and the generator's 16-bit comb (80 MiB) at fabgpu_init
size_t gtab_scratch_bytes();
hipError_t launch_gtab_build(void* d_tab, void* scratch, hipStream_t st);
// ... and a registered key's 16-bit comb in the same format (FABGPU_FLAG_KEY_TABLES_16BIT); scratch: keytab16_scratch_bytes() per key
size_t keytab16_scratch_bytes();
hipError_t launch_keytab16_build(uint32_t n_keys, const void* qxy, void* const* tabs, void* scratch, hipStream_t st);
}  // namespace fab
