// HIP kernels for gfx950 (MI355X / CDNA4): batched SHA-256 (with shared-prefix mid-states), batched ECDSA P-256 verify -
// one signature per lane, or two lanes per signature for batches that cannot fill the chip - for fresh and for registered
// public keys, and the fused hash+verify kernels.  64-lane wavefronts, verdicts packed with a wave ballot.  No MFMA: this is
// integer VALU work (v_mad_i64_i32 on 29-bit signed limbs for the big-number part - fe29.h, generated streams in fe29_gcn.h /
// pair29_gcn.h - and v_alignbit / v_xor / v_add for SHA-256).
//
// Replaces (reference, all CPU): bccsp/sw/hash.go:29-33, bccsp/sw/ecdsa.go:41-57 -> crypto/ecdsa.Verify,
// called per signature from msp/identities.go:169-196.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>

#include "device_common.h"
#include "kernels.h"
#include "p256_pair29.h"

namespace fab {

// (SHA-256 per lane, field loads, verdict packing and the per-lane table workspace: device_common.h)

__global__ void __launch_bounds__(256) sha256_midstate_kernel(uint32_t m, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                               const uint32_t* __restrict__ pre_off, uint32_t spans, uint32_t* __restrict__ mid) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    bool active = p < m;
    uint32_t pc = active ? p : (m - 1);
    uint32_t start = pre_off[spans ? 2 * pc : pc], len = pre_off[spans ? 2 * pc + 1 : pc + 1] - start;
    uint32_t nfull = active ? (len >> 6) : 0, maxfull = nfull;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        uint32_t other = __shfl_xor(maxfull, o, 64);
        maxfull = other > maxfull ? other : maxfull;
    }
    maxfull = __builtin_amdgcn_readfirstlane(maxfull);
    uint32_t h[8];
    sha256_iv(h);
    const uint32_t shift = start & 3u;
    const uint32_t last_word = arena_words ? arena_words - 1 : 0;
    uint32_t nxt[17];
    auto fetch = [&](uint32_t blk_, uint32_t (&dst)[17]) {
        const uint32_t wi = (start + (blk_ << 6)) >> 2;
#pragma unroll
        for (int k = 0; k < 17; k++) {
            uint32_t idx = wi + k;
            idx = idx < last_word ? idx : last_word;
            dst[k] = arena32[idx];
        }
    };
    if (maxfull) fetch(0, nxt);
    for (uint32_t blk = 0; blk < maxfull; blk++) {             // (the next block's loads are in flight while this one is compressed)
        uint32_t w[16], raw[17];
#pragma unroll
        for (int k = 0; k < 17; k++) raw[k] = nxt[k];
        if (blk + 1 < maxfull) fetch(blk + 1, nxt);
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = __builtin_bswap32(__builtin_amdgcn_alignbyte(raw[k + 1], raw[k], shift));
        if (blk < nfull) sha256_compress(h, w);
    }
    if (active) {
        uint4* o = reinterpret_cast<uint4*>(mid + 8 * (size_t)p);
        o[0] = make_uint4(h[0], h[1], h[2], h[3]);
        o[1] = make_uint4(h[4], h[5], h[6], h[7]);
    }
}
// (hash-only launches: wide_kernels.hip - eight lanes per message for small ones, sha256_mixed_kernel beyond)

// ------------------------------------------------------------------------------------------------
// ECDSA P-256 verify
// ------------------------------------------------------------------------------------------------
// Persistent workgroups: a bounded number of slots, each walking the tiles  blockIdx.x, blockIdx.x + gridDim.x, ...  of BLOCK / LANES
// signatures (the per-lane j*Q workspace is sized by slots, not by the batch).
// One 256-thread workgroup per CU = one wave per SIMD.  A second wave per SIMD was measured (BLOCK = 512, round-1 PMC runs in
// profiles/): each wave then takes 1.5x the cycles, but the chip also drops from ~2.0 to ~1.6 GHz - the integer multiplier
// array is power-limited - so whole-job throughput does not move; one wave per SIMD keeps the latency of a block minimal.
//
// Nine of the ten kernels below are verify_tiles, one loop over three choices: where the digest comes from (DigestGiven / DigestHashed),
// where the key comes from and which core runs on it (FreshKey / RegisteredKey), and with them how many lanes own a signature (TileGeom).

// Lane geometry.  LANES = 1: one signature per lane.  LANES = 2 (p256_pair29.h): lane 2k / 2k+1 of a wave own signature k of the
// tile - 128 signatures per 256-thread workgroup, for batches that cannot fill the chip with one signature per lane.
struct TileRow {
    uint32_t i;    // the row of the batch this lane stands for in this tile
    uint32_t ic;   // the row it reads: i, or the last row of the batch on a tail lane
    bool active;   // i < n
};
template <int BLOCK, int LANES>
struct TileGeom {
    static_assert(LANES == 1 || LANES == 2, "one or two lanes per signature");
    static constexpr uint32_t PER_WG = BLOCK / LANES;   // signatures per workgroup and tile
    static __device__ __forceinline__ bool odd(uint32_t lane) { return LANES == 2 && (lane & 1) != 0; }   // the second lane of a pair
    static __device__ __forceinline__ uint32_t sub(uint32_t lane) { return lane / LANES; }                // the lane's signature within a tile
    static __device__ __forceinline__ uint32_t ntiles(uint32_t n) { return (n + PER_WG - 1) / PER_WG; }
    // CONSENSUS-CRITICAL, and only here: tail lanes compute on the last tuple (every lane runs the whole instruction stream, reaches
    // every ballot and every barrier, and reads inside the batch) and write nothing; of a pair only the even lane writes.
    static __device__ __forceinline__ TileRow row(uint32_t tile, uint32_t sub, uint32_t n) {
        const uint32_t i = tile * PER_WG + sub;
        const bool active = i < n;
        return TileRow{i, active ? i : (n - 1), active};
    }
    static __device__ __forceinline__ bool writes(const TileRow& t, bool odd) { return t.active && !odd; }
    static __device__ __forceinline__ void emit(const TileRow& t, uint32_t n, bool odd, uint32_t st, uint64_t* verdict_bits, uint8_t* status) {
        if constexpr (LANES == 1) emit_verdict(t.i, t.active, st, verdict_bits, status);
        else pair_emit_verdict(t.i, n, t.active, odd, st, reinterpret_cast<uint32_t*>(verdict_bits), status);   // the even lane carries the verdict
    }
};

// Digest source: the caller's e ...
struct DigestGiven {
    static constexpr bool BEFORE_KEY = false;   // one more load, behind the key's
    const uint8_t* e;
    __device__ __forceinline__ void operator()(u256& ve, const TileRow& t, bool) const { load_be_field(ve, e, t.ic); }
};
// ... or identity.Verify fused: e = SHA-256(msg) stays in registers (and leaves the chip only if pre.digests asks).  With two lanes per
// signature both lanes of a pair hash the (same) message - the hash is 18 % of the stream and does not split across lanes.
struct DigestHashed {
    static constexpr bool BEFORE_KEY = true;    // the key is read behind the hash: nothing of it is live across the SHA-256 stream
    const uint32_t* arena32;
    uint32_t arena_words;
    const uint32_t* off;
    const sha_prefixes pre;
    __device__ __forceinline__ void operator()(u256& ve, const TileRow& t, bool writes) const {
        uint32_t h[8];
        sha256_message(arena32, arena_words, off, pre, t.ic, t.active, h);
        emit_digest(pre, t.i, writes, h);
#pragma unroll
        for (int k = 0; k < 8; k++) ve.w[k] = h[7 - k];   // digest big-endian -> integer limbs
    }
};

// Key and core.  Fresh keys: (qx, qy) by row and a table of j*Q per signature that the core builds - GlobalQTab29 (one lane),
// PairQTab (global workspace, 16 entries, 5-bit windows) or PairQTabLds (LDS, 8 entries, W = 4: the all-odd recoding over odd multiples,
// or Booth digits over j*Q for BOOTH4).
template <int LANE_COUNT, class QTab, int W = 5, bool DBL1 = false, bool BOOTH4 = false, bool TABLE_ADD = false>
struct FreshKey {
    static constexpr int LANES = LANE_COUNT;
    const uint8_t *qx, *qy;
    const int32_t* gtab;
    QTab qtab;
    struct Row { u256 x, y; };
    __device__ __forceinline__ void load(Row& k, uint32_t ic) const {
        load_be_field(k.x, qx, ic);
        load_be_field(k.y, qy, ic);
    }
    __device__ __forceinline__ uint32_t verify(const Row& k, const u256& e, const u256& r, const u256& s, bool odd) {
        if constexpr (LANES == 1) {
            GTab16 gt{gtab};
            return p256_verify_core29(k.x, k.y, e, r, s, gt, qtab);
        } else {
            return p256_verify_pair29<QTab, W, DBL1, BOOTH4, TABLE_ADD>(k.x, k.y, e, r, s, gtab, qtab, odd);
        }
    }
};
// Registered public keys (fabgpu_p256_key_register): every signature names a key whose 8-bit comb table is resident on the
// device, so u2*Q is 32 mixed additions like u1*G: no doublings, no per-lane table, no workspace.  ktabs[KTAB_STRIDE k] = table of key k,
// ktabs[KTAB_STRIDE k + 1] = its 16-bit comb or nullptr (round 6, FABGPU_FLAG_KEY_TABLES_16BIT: 16 mixed additions when a whole wavefront has them).
// An id that is out of range, or that names another generation than the slot's present tenant (a retired key: key_slots.h), reports
// status 4 ("use bccsp/sw"), never a verdict - and reads none of the slot's tables, which may be another key's by now or half way
// there: such a row runs on the generator's table and its result is dropped.
template <int LANE_COUNT>
struct RegisteredKey {
    static constexpr int LANES = LANE_COUNT;
    const uint32_t* key_id;
    uint32_t nkeys;
    const int32_t* const* ktabs;
    const int32_t* gtab;
    struct Row { const int32_t *kt, *kt16; bool kok; };
    __device__ __forceinline__ void load(Row& k, uint32_t ic) const {
        const uint32_t kid = key_id[ic], sl = kid & ((1u << KEY_SLOT_BITS) - 1u);
        const bool inr = sl < nkeys;
        const int32_t* const* slot = ktabs + KTAB_STRIDE * (size_t)(inr ? sl : 0);
        const int32_t *t8 = slot[0], *t16 = slot[1];
        k.kok = inr && (uint32_t)(uintptr_t)slot[2] == (kid >> KEY_SLOT_BITS);
        k.kt = k.kok ? t8 : gtab;              // (a 16-bit comb is larger than an 8-bit one: every index of the latter lies inside)
        k.kt16 = k.kok ? t16 : nullptr;
    }
    __device__ __forceinline__ uint32_t verify(const Row& k, const u256& e, const u256& r, const u256& s, bool odd) {
        uint32_t st;
        if constexpr (LANES == 1) {
            GTab16 gt{gtab};
            st = __all(k.kt16 != nullptr) ? p256_verify_keyed_core29(e, r, s, gt, GTab16{k.kt16}) : p256_verify_keyed_core29(e, r, s, gt, KeyTab8{k.kt});
        } else {
            st = p256_verify_keyed_pair29(e, r, s, gtab, k.kt, k.kt16, odd);
        }
        if (!k.kok) st = ST_OFF_CURVE;
        return st;
    }
};

template <int BLOCK, class Digest, class Key>
__device__ __forceinline__ void verify_tiles(uint32_t n, const Digest& digest, Key key, const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    using Geom = TileGeom<BLOCK, Key::LANES>;
    const bool odd = Geom::odd(threadIdx.x);
    const uint32_t sub = Geom::sub(threadIdx.x);
    const uint32_t ntiles = Geom::ntiles(n);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const TileRow t = Geom::row(tile, sub, n);
        u256 ve, vr, vs;
        typename Key::Row k;
        if constexpr (Digest::BEFORE_KEY) digest(ve, t, Geom::writes(t, odd));
        key.load(k, t.ic);
        if constexpr (!Digest::BEFORE_KEY) digest(ve, t, Geom::writes(t, odd));
        load_be_field(vr, r, t.ic);
        load_be_field(vs, s, t.ic);
        uint32_t st = key.verify(k, ve, vr, vs, odd);
        Geom::emit(t, n, odd, st, verdict_bits, status);
    }
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, 2) p256_verify_kernel(uint32_t n, const uint8_t* __restrict__ qx, const uint8_t* __restrict__ qy,
                                                                    const uint8_t* __restrict__ e, const uint8_t* __restrict__ r,
                                                                    const uint8_t* __restrict__ s, const int32_t* __restrict__ gtab,
                                                                    uint4* __restrict__ qws, uint64_t* __restrict__ verdict_bits,
                                                                    uint8_t* __restrict__ status) {
    using QTab = GlobalQTab29<BLOCK>;
    verify_tiles<BLOCK>(n, DigestGiven{e}, FreshKey<1, QTab>{qx, qy, gtab, QTab::of(qws + (size_t)blockIdx.x * (QWS_UINT4_PER_LANE * BLOCK), threadIdx.x)}, r, s, verdict_bits, status);
}

// Two lanes per signature, the per-signature table in the global workspace.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, 1) p256_verify_pair_kernel(uint32_t n, const uint8_t* __restrict__ qx, const uint8_t* __restrict__ qy,
                                                                         const uint8_t* __restrict__ e, const uint8_t* __restrict__ r,
                                                                         const uint8_t* __restrict__ s, const int32_t* __restrict__ gtab,
                                                                         uint4* __restrict__ qws, uint64_t* __restrict__ verdict_bits,
                                                                         uint8_t* __restrict__ status) {
    using QTab = PairQTab<BLOCK / 2>;
    verify_tiles<BLOCK>(n, DigestGiven{e}, FreshKey<2, QTab>{qx, qy, gtab, QTab::of(qws + (size_t)blockIdx.x * (QWS_PAIR_UINT4_PER_SIG * (BLOCK / 2)), threadIdx.x >> 1)}, r, s, verdict_bits, status);
}

// The same with the per-signature table in LDS (PairQTabLds: 8 entries, signed 4-bit windows) instead of the global workspace: no
// table traffic at all (p256_pair29.h says what that is worth).  Dynamic LDS: 128 signatures x 1040 bytes.  One wave per SIMD: the
// A/B form of the helper-wave kernel below (FABGPU_FLAG_PAIR_SOLO).  DBL1: the per-doubling loop instead of PAIR_DBL4 (FABGPU_FLAG_PAIR_DBL1).
// BOOTH4: Booth digits over j*Q, 65 windows, instead of the all-odd recoding over odd multiples, 63 windows (FABGPU_FLAG_PAIR_BOOTH4).
// TABLE_ADD: the table of odd multiples by general additions instead of co-Z additions (FABGPU_FLAG_PAIR_TABLE_ADD; the default instance only:
// the DBL1 instances build it that way regardless, the Booth instances have the table j*Q).
template <int BLOCK, bool DBL1 = false, bool BOOTH4 = false, bool TABLE_ADD = false>
__global__ void __launch_bounds__(BLOCK, 1) p256_verify_pair_lds_solo_kernel(uint32_t n, const uint8_t* __restrict__ qx, const uint8_t* __restrict__ qy,
                                                                             const uint8_t* __restrict__ e, const uint8_t* __restrict__ r,
                                                                             const uint8_t* __restrict__ s, const int32_t* __restrict__ gtab,
                                                                             uint64_t* __restrict__ verdict_bits, uint8_t* __restrict__ status) {
    extern __shared__ uint4 pair_lds[];
    verify_tiles<BLOCK>(n, DigestGiven{e}, FreshKey<2, PairQTabLds, 4, DBL1, BOOTH4, TABLE_ADD>{qx, qy, gtab, PairQTabLds::of(pair_lds, threadIdx.x >> 1)}, r, s, verdict_bits, status);
}

// The LDS-table pair kernel with HELPER WAVES (p256_pair29.h, "HELPER-WAVE FORM"): 2 x BLOCK threads, the same 128 signatures per
// tile.  Threads 0..BLOCK-1 (main) run the u2*Q chain and emit the verdicts; threads BLOCK..2 BLOCK-1 (helper) run s^-1, u1, u2 and
// u1*G on the same SIMDs and hand u2 and S over through LDS.  Every wave reaches both barriers of every tile (TileGeom::row).
// Two roles and two barriers: a tile loop of its own, on the same geometry.  Dynamic LDS: pair_table_lds_bytes().
template <int BLOCK, bool DBL1 = false, bool BOOTH4 = false, bool TABLE_ADD = false>
__global__ void __launch_bounds__(2 * BLOCK, 1) p256_verify_pair_lds_kernel(uint32_t n, const uint8_t* __restrict__ qx, const uint8_t* __restrict__ qy,
                                                                                 const uint8_t* __restrict__ e, const uint8_t* __restrict__ r,
                                                                                 const uint8_t* __restrict__ s, const int32_t* __restrict__ gtab,
                                                                                 uint64_t* __restrict__ verdict_bits, uint8_t* __restrict__ status) {
    extern __shared__ uint4 pair_lds[];
    using Geom = TileGeom<BLOCK, 2>;
    // wave-uniform by construction (BLOCK is a multiple of 64); readfirstlane makes the role a scalar branch for the compiler too
    const bool helper = __builtin_amdgcn_readfirstlane(threadIdx.x) >= (uint32_t)BLOCK;
    const uint32_t lane = threadIdx.x & (uint32_t)(BLOCK - 1);
    const bool odd = Geom::odd(lane);
    const uint32_t sub = Geom::sub(lane);
    PairQTabLds qtab = PairQTabLds::of(pair_lds, sub);
    const PairHandoffLds<BLOCK> hand = PairHandoffLds<BLOCK>::of(reinterpret_cast<uint32_t*>(pair_lds + Geom::PER_WG * PAIR_LDS_CELLS_PER_SIG), lane);
    const uint32_t ntiles = Geom::ntiles(n);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const TileRow t = Geom::row(tile, sub, n);
        u256 he, hw;                  // helper: e, and w = s^-1 (u1 = e w is computed behind barrier A)
        uint32_t early = 0;           // helper: range gates
        pair_pt Qp, T;                // main
        bool q_ok = false, t_inf = true;
        if (helper) {
            u256 vr, vs;
            load_be_field(he, e, t.ic);
            load_be_field(vr, r, t.ic);
            load_be_field(vs, s, t.ic);
            pair_helper_scalars29<PairHandoffLds<BLOCK>, BOOTH4>(hw, early, vr, vs, hand, odd);
        } else {
            u256 vqx, vqy;
            load_be_field(vqx, qx, t.ic);
            load_be_field(vqy, qy, t.ic);
            q_ok = pair_main_table29<PairQTabLds, BOOTH4, TABLE_ADD || DBL1>(Qp, vqx, vqy, qtab, odd);
        }
        __syncthreads();              // A: u2 in LDS
        if (helper) {
            pair_helper_comb29(he, hw, early, gtab, hand, odd);
        } else {
            u256 u2;                  // (folded by the helper unless BOOTH4)
            hand.get_u2(u2);
            if constexpr (BOOTH4) {
                pair_u2_mult29<PairQTabLds, 4, DBL1>(T, t_inf, u2, Qp, qtab, odd);
            } else {
                pair_u2_mult_odd29<PairQTabLds, DBL1>(T, u2, qtab, odd);
                t_inf = false;
            }
        }
        __syncthreads();              // B: S, s_inf and the gate status in LDS
        if (!helper) {
            u256 vr;                  // (loaded here, not kept in registers across the chain)
            load_be_field(vr, r, t.ic);
            uint32_t st = pair_main_finish29(T, t_inf, q_ok, vr, hand, odd);
            Geom::emit(t, n, odd, st, verdict_bits, status);
        }
    }
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, 2) p256_verify_keyed_kernel(uint32_t n, const uint32_t* __restrict__ key_id, uint32_t nkeys,
                                                                          const int32_t* const* __restrict__ ktabs, const uint8_t* __restrict__ e,
                                                                          const uint8_t* __restrict__ r, const uint8_t* __restrict__ s,
                                                                          const int32_t* __restrict__ gtab, uint64_t* __restrict__ verdict_bits,
                                                                          uint8_t* __restrict__ status) {
    verify_tiles<BLOCK>(n, DigestGiven{e}, RegisteredKey<1>{key_id, nkeys, ktabs, gtab}, r, s, verdict_bits, status);
}
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, 2) p256_verify_keyed_pair_kernel(uint32_t n, const uint32_t* __restrict__ key_id, uint32_t nkeys,
                                                                               const int32_t* const* __restrict__ ktabs, const uint8_t* __restrict__ e,
                                                                               const uint8_t* __restrict__ r, const uint8_t* __restrict__ s,
                                                                               const int32_t* __restrict__ gtab, uint64_t* __restrict__ verdict_bits,
                                                                               uint8_t* __restrict__ status) {
    verify_tiles<BLOCK>(n, DigestGiven{e}, RegisteredKey<2>{key_id, nkeys, ktabs, gtab}, r, s, verdict_bits, status);
}

// identity.Verify fused (SHA-256 then the core; the digest stays in registers): registered keys ...
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, 2) sha256_p256_verify_keyed_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                                                 const uint32_t* __restrict__ off, const uint32_t* __restrict__ key_id,
                                                                                 uint32_t nkeys, const int32_t* const* __restrict__ ktabs,
                                                                                 const uint8_t* __restrict__ r, const uint8_t* __restrict__ s,
                                                                                 const int32_t* __restrict__ gtab, uint64_t* __restrict__ verdict_bits,
                                                                                 uint8_t* __restrict__ status, sha_prefixes pre) {
    verify_tiles<BLOCK>(n, DigestHashed{arena32, arena_words, off, pre}, RegisteredKey<1>{key_id, nkeys, ktabs, gtab}, r, s, verdict_bits, status);
}
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, 2) sha256_p256_verify_keyed_pair_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                                                      const uint32_t* __restrict__ off, const uint32_t* __restrict__ key_id,
                                                                                      uint32_t nkeys, const int32_t* const* __restrict__ ktabs,
                                                                                      const uint8_t* __restrict__ r, const uint8_t* __restrict__ s,
                                                                                      const int32_t* __restrict__ gtab, uint64_t* __restrict__ verdict_bits,
                                                                                      uint8_t* __restrict__ status, sha_prefixes pre) {
    verify_tiles<BLOCK>(n, DigestHashed{arena32, arena_words, off, pre}, RegisteredKey<2>{key_id, nkeys, ktabs, gtab}, r, s, verdict_bits, status);
}

// ... and fresh ones, with two lanes per signature and with one
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, 1) sha256_p256_verify_pair_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                                                const uint32_t* __restrict__ off, const uint8_t* __restrict__ qx,
                                                                                const uint8_t* __restrict__ qy, const uint8_t* __restrict__ r,
                                                                                const uint8_t* __restrict__ s, const int32_t* __restrict__ gtab,
                                                                                uint4* __restrict__ qws, uint64_t* __restrict__ verdict_bits,
                                                                                uint8_t* __restrict__ status, sha_prefixes pre) {
    using QTab = PairQTab<BLOCK / 2>;
    verify_tiles<BLOCK>(n, DigestHashed{arena32, arena_words, off, pre},
                        FreshKey<2, QTab>{qx, qy, gtab, QTab::of(qws + (size_t)blockIdx.x * (QWS_PAIR_UINT4_PER_SIG * (BLOCK / 2)), threadIdx.x >> 1)}, r, s, verdict_bits, status);
}
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK, 2) sha256_p256_verify_kernel(uint32_t n, const uint32_t* __restrict__ arena32, uint32_t arena_words,
                                                                           const uint32_t* __restrict__ off, const uint8_t* __restrict__ qx,
                                                                           const uint8_t* __restrict__ qy, const uint8_t* __restrict__ r,
                                                                           const uint8_t* __restrict__ s, const int32_t* __restrict__ gtab,
                                                                           uint4* __restrict__ qws, uint64_t* __restrict__ verdict_bits,
                                                                           uint8_t* __restrict__ status, sha_prefixes pre) {
    using QTab = GlobalQTab29<BLOCK>;
    verify_tiles<BLOCK>(n, DigestHashed{arena32, arena_words, off, pre},
                        FreshKey<1, QTab>{qx, qy, gtab, QTab::of(qws + (size_t)blockIdx.x * (QWS_UINT4_PER_LANE * BLOCK), threadIdx.x)}, r, s, verdict_bits, status);
}

// Stitches the pieces of gathered messages (fabgpu_identity_batch.gather_spans) into consecutive bytes: one WAVEFRONT per message,
// lane l moving bytes l, l + 64, ... of each piece (byte granularity because the pieces sit at arbitrary offsets of the block
// buffer; coalesced 64-byte rows).  A lane-per-message byte loop was measured first: its ~1500 dependent load/store round
// trips per lane cost 2 ms per 10 000-transaction block.
__global__ void __launch_bounds__(256) gather_spans_kernel(uint32_t n, const uint8_t* __restrict__ arena, uint32_t arena_bytes,
                                                            const uint32_t* __restrict__ spans, const uint32_t* __restrict__ out_off,
                                                            uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= n) return;
    uint32_t o = out_off[i];
    const uint32_t oe = out_off[i + 1];
    for (int p = 0; p < 3; p++) {
        uint32_t s = spans[6 * (size_t)i + 2 * p], e = spans[6 * (size_t)i + 2 * p + 1];
        e = e < arena_bytes ? e : arena_bytes;
        if (e <= s) continue;
        uint32_t len = e - s;
        len = len < oe - o ? len : oe - o;
        for (uint32_t b = lane; b < len; b += 64) out[o + b] = arena[s + b];
        o += len;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers (host)
// ------------------------------------------------------------------------------------------------
static void launch_midstate_kernel(const void* arena, size_t arena_bytes, const ShaPrefixArgs& pa, uint32_t lds, hipStream_t st) {
    dim3 grid((pa.m + 255) / 256), block(256);
    hipLaunchKernelGGL(sha256_midstate_kernel, grid, block, lds, st, pa.m, (const uint32_t*)arena, (uint32_t)((arena_bytes + 3) / 4),
                       (const uint32_t*)pa.pre_off, pa.spans ? 1u : 0u, (uint32_t*)pa.mid_scratch);
}
// Runs the mid-state kernel for a prefixed batch (no-op otherwise) and returns the descriptor the fused kernels take.
static sha_prefixes launch_midstates(const void* arena, size_t arena_bytes, const ShaPrefixArgs& pa, hipStream_t st) {
    sha_prefixes pre{nullptr, nullptr, nullptr, 0, pa.spans ? 1u : 0u, (uint32_t*)pa.digests};
    if (pa.m == 0 || pa.pre_idx == nullptr) return pre;
    if (!pa.mid_ready) launch_midstate_kernel(arena, arena_bytes, pa, 0, st);
    pre.pre_idx = (const uint32_t*)pa.pre_idx;
    pre.pre_off = (const uint32_t*)pa.pre_off;
    pre.mid = (const uint32_t*)pa.mid_scratch;
    pre.m = pa.m;
    return pre;
}
hipError_t launch_sha256_midstates(const void* arena, size_t arena_bytes, const ShaPrefixArgs& pa, hipStream_t st) {
    if (pa.m == 0) return hipSuccess;
    launch_midstate_kernel(arena, arena_bytes, pa, pa.lds_reserve, st);
    return hipGetLastError();
}
hipError_t launch_sha256_batch(uint32_t n, const void* arena, size_t arena_bytes, const void* off, void* digests, hipStream_t st, uint32_t lds_spread) {
    if (n == 0) return hipSuccess;
    if (n <= SHA_COOP_MAX) {                    // a launch that cannot fill the chip: eight lanes per message (sha256_coop.h)
        ShaPrefixArgs pa;
        pa.digests = digests;
        return launch_sha256_messages_coop(n, arena, arena_bytes, off, pa, st, lds_spread);
    }
    return launch_sha256_mixed(n, arena, arena_bytes, off, false, digests, st);
}
hipError_t launch_sha256_spans(uint32_t n, const void* arena, size_t arena_bytes, const void* spans, void* digests, hipStream_t st, uint32_t lds_reserve,
                               uint32_t lds_spread) {
    if (n == 0) return hipSuccess;
    if (n <= SHA_COOP_MAX && lds_reserve == 0) {
        ShaPrefixArgs pa;
        pa.spans = true;
        pa.digests = digests;
        return launch_sha256_messages_coop(n, arena, arena_bytes, spans, pa, st, lds_spread);
    }
    return launch_sha256_mixed(n, arena, arena_bytes, spans, true, digests, st, lds_reserve);
}
hipError_t launch_gather_sha256(uint32_t n, const void* arena, size_t arena_bytes, const void* spans, const void* out_off, void* scratch,
                                size_t scratch_bytes, void* digests, hipStream_t st, uint32_t lds_reserve, uint32_t lds_spread) {
    if (n == 0) return hipSuccess;
    dim3 grid((n + 3) / 4), block(256);   // four wavefronts = four messages per workgroup
    hipLaunchKernelGGL(gather_spans_kernel, grid, block, lds_reserve, st, n, (const uint8_t*)arena, (uint32_t)arena_bytes, (const uint32_t*)spans,
                       (const uint32_t*)out_off, (uint8_t*)scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (lds_reserve) return launch_sha256_mixed(n, scratch, scratch_bytes, out_off, false, digests, st, lds_reserve);   // keeping to its own CUs
    return launch_sha256_batch(n, scratch, scratch_bytes, out_off, digests, st, lds_spread);
}

VerifyGeom verify_geom(uint32_t n, bool allow_pair) {
    VerifyGeom g;
    g.block = VERIFY_BLOCK;
    g.pair = allow_pair && n <= (uint32_t)VERIFY_PAIR_MAX;
    uint32_t per_wg = g.pair ? VERIFY_BLOCK / 2 : VERIFY_BLOCK;
    uint32_t tiles = (n + per_wg - 1) / per_wg;
    g.wgs = tiles < (uint32_t)VERIFY_MAX_WGS ? tiles : (uint32_t)VERIFY_MAX_WGS;
    return g;
}
// Where the two-lanes-per-signature verify-only kernel keeps its per-signature table when the context does not say
// (FABGPU_FLAG_PAIR_TABLE_LDS / _GLOBAL in fabgpu_cfg.flags force one; bench.py --pair-table for A/B runs): -1 = by batch size (launch_verify).
int pair_table_default() { return -1; }
// helper-wave form: the 128 tables + the handoff (PAIR_HAND_WORDS per main lane) = 133 120 + 27 648 = 160 768 bytes of the CU's 163 840
size_t pair_table_lds_bytes() { return (size_t)(VERIFY_BLOCK / 2) * PAIR_LDS_CELLS_PER_SIG * 16 + (size_t)VERIFY_BLOCK * PAIR_HAND_WORDS * 4; }
size_t pair_table_lds_solo_bytes() { return (size_t)(VERIFY_BLOCK / 2) * PAIR_LDS_CELLS_PER_SIG * 16; }
size_t verify_workspace_bytes(uint32_t n, bool allow_pair) {
    VerifyGeom g = verify_geom(n, allow_pair);
    if (g.pair) return (size_t)g.wgs * (g.block / 2) * QWS_PAIR_UINT4_PER_SIG * 16;
    return (size_t)g.wgs * g.block * QWS_UINT4_PER_LANE * 16;
}

// The LDS-table pair kernels by [one-wave form][per-doubling loop][Booth digits]: the first is the product's, the rest are A/B forms;
// and the product's two forms with the table of odd multiples by general additions (FABGPU_FLAG_PAIR_TABLE_ADD), by [one-wave form].
using PairLdsKernel = void (*)(uint32_t, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, const int32_t*, uint64_t*, uint8_t*);
static const PairLdsKernel pair_lds_kernels[2][2][2] = {
    {{p256_verify_pair_lds_kernel<VERIFY_BLOCK, false, false>, p256_verify_pair_lds_kernel<VERIFY_BLOCK, false, true>},
     {p256_verify_pair_lds_kernel<VERIFY_BLOCK, true, false>, p256_verify_pair_lds_kernel<VERIFY_BLOCK, true, true>}},
    {{p256_verify_pair_lds_solo_kernel<VERIFY_BLOCK, false, false>, p256_verify_pair_lds_solo_kernel<VERIFY_BLOCK, false, true>},
     {p256_verify_pair_lds_solo_kernel<VERIFY_BLOCK, true, false>, p256_verify_pair_lds_solo_kernel<VERIFY_BLOCK, true, true>}}};
static const PairLdsKernel pair_lds_table_add_kernels[2] = {p256_verify_pair_lds_kernel<VERIFY_BLOCK, false, false, true>,
                                                            p256_verify_pair_lds_solo_kernel<VERIFY_BLOCK, false, false, true>};

// One ECDSA P-256 verify launch (kernels.h VerifyLaunch): picks the kernel by key source, digest source, batch size and table home.
hipError_t launch_verify(const VerifyLaunch& v, hipStream_t st) {
    const uint32_t n = v.n;
    if (n == 0) return hipSuccess;
    const bool keyed = v.key_id != nullptr && v.ktabs != nullptr, fresh = v.qx != nullptr && v.qy != nullptr;
    const bool hashed = v.off != nullptr, given = v.e != nullptr;
    // exactly one of each pair of alternatives, none of them half-named, and no message bytes without an arena
    if (keyed == fresh || hashed == given || keyed != (v.key_id != nullptr || v.ktabs != nullptr) || fresh != (v.qx != nullptr || v.qy != nullptr) ||
        (hashed && v.arena == nullptr && v.arena_bytes != 0))
        return hipErrorInvalidValue;
    const uint8_t *qx = (const uint8_t*)v.qx, *qy = (const uint8_t*)v.qy, *e = (const uint8_t*)v.e, *r = (const uint8_t*)v.r, *s = (const uint8_t*)v.s;
    const uint32_t *key_id = (const uint32_t*)v.key_id, *arena32 = (const uint32_t*)v.arena, *off = (const uint32_t*)v.off;
    const uint32_t arena_words = (uint32_t)((v.arena_bytes + 3) / 4);
    const int32_t* const* ktabs = (const int32_t* const*)v.ktabs;
    const int32_t* gtab = (const int32_t*)v.gtab;
    uint4* qws = (uint4*)v.qws;
    uint64_t* verdict_bits = (uint64_t*)v.verdict_bits;
    uint8_t* status = (uint8_t*)v.status;
    sha_prefixes pre{};
    if (hashed) pre = launch_midstates(v.arena, v.arena_bytes, v.pa, st);
    VerifyGeom g = verify_geom(n, v.allow_pair);
    dim3 grid(g.wgs), block(g.block);
    const uint32_t lds_reserve = hashed ? v.pa.lds_reserve : v.lds_reserve;   // (a fused launch carries its reservation with its prefixes)
    if (!hashed && !keyed) {
        // The per-signature table of the pair kernel: in LDS when the launch is large (measured on MI355X, tools/gpu_pair_table_ab.py and
        // tools/gpu_pmc_traffic.sh: at 30 000 tuples the two forms take the same time - 0.631 / 0.629 ms back to back - and the LDS form
        // moves 94 MB through the memory system per launch instead of 279 MB); in the global workspace for smaller ones, where the LDS
        // form's 13 extra additions show as latency (10 000 tuples: 0.624 against 0.614 ms; 1 000: 0.618 against 0.603 ms).
        const bool table_lds = v.table_lds < 0 ? n > (uint32_t)PAIR_TABLE_LDS_FROM : v.table_lds != 0;
        // The LDS form with helper waves (two waves per SIMD: the scalar part and u1*G beside the u2*Q chain) unless the context asks for
        // the one-wave form (FABGPU_FLAG_PAIR_SOLO, A/B runs).
        // Either with the four doublings of a window as one program, or (FABGPU_FLAG_PAIR_DBL1, A/B runs) as the per-doubling loop.
        // And with the all-odd recoding over a table of odd multiples, 63 windows, or (FABGPU_FLAG_PAIR_BOOTH4, A/B runs) Booth digits, 65.
        if (g.pair && table_lds) {
            // The table of odd multiples by co-Z additions, or (FABGPU_FLAG_PAIR_TABLE_ADD, A/B runs) by general ones: the flag selects among
            // the default instances; the DBL1 instances build it by general additions anyway and the Booth instances have another table.
            const PairLdsKernel k = v.pair_table_add && !v.pair_dbl1 && !v.pair_booth4 ? pair_lds_table_add_kernels[v.pair_solo ? 1 : 0]
                                                                                        : pair_lds_kernels[v.pair_solo ? 1 : 0][v.pair_dbl1 ? 1 : 0][v.pair_booth4 ? 1 : 0];
            if (v.pair_solo) hipLaunchKernelGGL(k, grid, block, pair_table_lds_solo_bytes(), st, n, qx, qy, e, r, s, gtab, verdict_bits, status);
            else hipLaunchKernelGGL(k, grid, dim3(2 * VERIFY_BLOCK), pair_table_lds_bytes(), st, n, qx, qy, e, r, s, gtab, verdict_bits, status);
        } else if (g.pair)
            hipLaunchKernelGGL(p256_verify_pair_kernel<VERIFY_BLOCK>, grid, block, lds_reserve, st, n, qx, qy, e, r, s, gtab, qws, verdict_bits, status);
        else
            hipLaunchKernelGGL(p256_verify_kernel<VERIFY_BLOCK>, grid, block, lds_reserve, st, n, qx, qy, e, r, s, gtab, qws, verdict_bits, status);
        return hipGetLastError();
    }
    if (hashed && !keyed) {
        if (g.pair)
            hipLaunchKernelGGL(sha256_p256_verify_pair_kernel<VERIFY_BLOCK>, grid, block, lds_reserve, st, n, arena32, arena_words, off, qx, qy, r, s, gtab, qws,
                               verdict_bits, status, pre);
        else
            hipLaunchKernelGGL(sha256_p256_verify_kernel<VERIFY_BLOCK>, grid, block, lds_reserve, st, n, arena32, arena_words, off, qx, qy, r, s, gtab, qws,
                               verdict_bits, status, pre);
        return hipGetLastError();
    }
    if (!hashed) {
        if (g.pair)
            hipLaunchKernelGGL(p256_verify_keyed_pair_kernel<VERIFY_BLOCK>, grid, block, lds_reserve, st, n, key_id, v.nkeys, ktabs, e, r, s, gtab, verdict_bits, status);
        else
            hipLaunchKernelGGL(p256_verify_keyed_kernel<VERIFY_BLOCK>, grid, block, lds_reserve, st, n, key_id, v.nkeys, ktabs, e, r, s, gtab, verdict_bits, status);
        return hipGetLastError();
    }
    if (g.pair)
        hipLaunchKernelGGL(sha256_p256_verify_keyed_pair_kernel<VERIFY_BLOCK>, grid, block, lds_reserve, st, n, arena32, arena_words, off, key_id, v.nkeys, ktabs,
                           r, s, gtab, verdict_bits, status, pre);
    else
        hipLaunchKernelGGL(sha256_p256_verify_keyed_kernel<VERIFY_BLOCK>, grid, block, lds_reserve, st, n, arena32, arena_words, off, key_id, v.nkeys, ktabs,
                           r, s, gtab, verdict_bits, status, pre);
    return hipGetLastError();
}

// The runtime resolves a kernel FUNCTION (symbol lookup, kernel object, argument layout) at its first launch, on the launching thread -
// after the code object of its translation unit is loaded, which the provider's construction already rehearses with one launch per unit.
// The keyed kernels are first launched by the second block of a fresh provider (its identities earn their tables during the first):
// asking for every function's attributes now moves that work to construction too (GPUCSP::Preallocate).  Returns how many resolved.
int warm_kernel_functions_kernels() {
    int ok = 0;
    hipFuncAttributes a;
    const void* fns[] = {(const void*)p256_verify_kernel<VERIFY_BLOCK>, (const void*)p256_verify_pair_kernel<VERIFY_BLOCK>,
                         (const void*)p256_verify_pair_lds_kernel<VERIFY_BLOCK>, (const void*)p256_verify_pair_lds_solo_kernel<VERIFY_BLOCK>,
                         (const void*)p256_verify_pair_lds_kernel<VERIFY_BLOCK, true>, (const void*)p256_verify_pair_lds_solo_kernel<VERIFY_BLOCK, true>,
                         (const void*)p256_verify_pair_lds_kernel<VERIFY_BLOCK, false, true>, (const void*)p256_verify_pair_lds_solo_kernel<VERIFY_BLOCK, false, true>,
                         (const void*)p256_verify_pair_lds_kernel<VERIFY_BLOCK, true, true>, (const void*)p256_verify_pair_lds_solo_kernel<VERIFY_BLOCK, true, true>,
                         (const void*)p256_verify_pair_lds_kernel<VERIFY_BLOCK, false, false, true>, (const void*)p256_verify_pair_lds_solo_kernel<VERIFY_BLOCK, false, false, true>,
                         (const void*)p256_verify_keyed_kernel<VERIFY_BLOCK>,
                         (const void*)p256_verify_keyed_pair_kernel<VERIFY_BLOCK>, (const void*)sha256_p256_verify_keyed_kernel<VERIFY_BLOCK>,
                         (const void*)sha256_p256_verify_keyed_pair_kernel<VERIFY_BLOCK>, (const void*)sha256_p256_verify_pair_kernel<VERIFY_BLOCK>,
                         (const void*)sha256_p256_verify_kernel<VERIFY_BLOCK>, (const void*)sha256_midstate_kernel, (const void*)gather_spans_kernel};
    for (const void* f : fns) ok += hipFuncGetAttributes(&a, f) == hipSuccess ? 1 : 0;
    return ok;
}

}  // namespace fab
