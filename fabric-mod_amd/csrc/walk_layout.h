// Where everything lies in the four buffers of a block pass (fabgpu_api.hip walk_block_pass): the per-envelope device arrays, the
// per-tuple device arrays, the pinned staging buffer and the host-mapped results.  THE statement of that layout - the pass binds its
// pointers from these structs, walk_preallocate sizes the buffers from walk_worst_case below, and tests/test_walk_layout.py holds both
// to what earlier versions of the pass laid out by hand.  Pure arithmetic: host only, no runtime call.
//
// A layout is a run of WalkRegion members in the order they are carved, then a few scalars.  Every region starts on the buffer's
// alignment (256 bytes on the device, 64 in pinned and mapped memory); one of zero bytes takes no room.  Regions the pass fills or
// copies whole carry their byte size for that: the pass reads L.x.bytes instead of deriving the size a second time.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>

#include "block_walk_dev.h"
#include "kernels.h"

namespace fab {

struct WalkRegion {
    size_t off = 0, bytes = 0;
};
constexpr size_t WALK_DEV_ALIGN = 256, WALK_HOST_ALIGN = 64;
constexpr size_t walk_round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
struct WalkCarver {
    size_t at, align;
    constexpr WalkRegion take(size_t bytes) {
        const WalkRegion r{at, bytes};
        at = walk_round_up(at + bytes, align);
        return r;
    }
};
// true: each region starts where the room of the one before it ends - nothing else lies between the first and the last
constexpr bool walk_back_to_back(std::initializer_list<WalkRegion> rs, size_t align) {
    const WalkRegion* prev = nullptr;
    for (const WalkRegion& r : rs) {
        if (prev && r.off != walk_round_up(prev->off + prev->bytes, align)) return false;
        prev = &r;
    }
    return true;
}
// regions carved back to back as ONE region, for a single fill over all of them (their room included, as carved)
constexpr WalkRegion walk_span(std::initializer_list<WalkRegion> rs, size_t align) {
    const WalkRegion &a = *rs.begin(), &b = *(rs.end() - 1);
    return WalkRegion{a.off, walk_round_up(b.off + b.bytes, align) - a.off};
}
// the nym launch's verdict bitmap and status bytes over `rows` rows (the launch clears them for the rows it runs, the layout holds them for every creator)
constexpr size_t walk_nym_bits_bytes(size_t rows) { return (rows + 63) / 64 * 8 + 8; }
constexpr size_t walk_nym_status_bytes(size_t rows) { return rows + 64; }

// ---- per-envelope device arrays (fabgpu_ctx::walk_env) ----
struct WalkEnvShape {
    uint32_t ne = 0;                  // envelopes
    uint32_t n_msps = 0;              // idemix MSPs sent along (<= WALK_IDEMIX_MSPS_MAX)
    bool early_hash = false;          // the host's payload spans go up: the creators' hashes start before the walk
    bool host_counted = false;        // the host's per-envelope counts go up: no count kernel, no stash
    bool has_issuer_hashes = false;
};
struct WalkEnvLayout {
    // what the host sends up sits together, mirrored at the same offsets in the pinned staging buffer: ONE copy of [0, up_small), or of
    // [0, up_all) when the host counted
    WalkRegion env, pay, msps, ihash;
    WalkRegion cnt, base, cbase, type, und;
    WalkRegion tot, mask, flags, sum, learn, done, denv;
    WalkRegion stash;                 // what the count kernel keeps for the emit kernel
    size_t up_small = 0, up_all = 0, total = 0;
    static constexpr size_t N = 17;
    const WalkRegion* regions() const { return &env; }
};
constexpr WalkEnvLayout walk_env_layout(const WalkEnvShape& s) {
    WalkCarver c{0, WALK_DEV_ALIGN};
    WalkEnvLayout L;
    const size_t ne = s.ne;
    L.env = c.take(ne * 8);
    L.pay = c.take(s.early_hash ? ne * 8 : 0);
    L.msps = c.take(sizeof(DevIdemixMsp) * s.n_msps);
    L.ihash = c.take(s.has_issuer_hashes ? (size_t)32 * s.n_msps : 0);
    L.up_small = c.at;
    L.cnt = c.take(ne * 16);
    L.base = c.take(ne * 16);
    L.cbase = c.take(ne * 4);
    L.type = c.take(ne);
    L.und = c.take(ne);
    L.up_all = c.at;
    L.tot = c.take(sizeof(WalkTotals));
    L.mask = c.take(ne * 4);
    L.flags = c.take(ne);
    L.sum = c.take(sizeof(WalkSummary));
    L.learn = c.take(sizeof(WalkLearn) * WALK_LEARN_SLOTS);
    L.done = c.take(64);
    L.denv = c.take(s.early_hash ? ne * 32 : 0);
    L.stash = c.take(s.host_counted ? 0 : ne * sizeof(bccsp::walk::EnvStash));
    L.total = c.at;
    return L;
}

// ---- per-tuple device arrays (fabgpu_ctx::walk_tup), sized once the totals are known ----
struct WalkTupleShape {
    uint32_t nt = 0, np = 0, nc = 0;  // tuples (the appended block signatures included), shared prefixes, hash checks
    uint32_t creators = 0;            // envelopes that yield tuples
    uint32_t n_msps = 0;
    bool tuple_qxy = false;           // the caller wants every tuple's key
    bool memo = false, hmemo = false; // the verdict memo is built on the device; ... and the digest memo's index beside it
    uint32_t memo_slot_cap = 0;       // (memo) the caller's slot table: a power of two >= 2 nt
    size_t memo_keys_cap = 0;         // (memo) the caller's room for keys
};
struct WalkTupleLayout {
    WalkRegion tup, pre, chk, gsp, gof, gdg, idx, off, pix, kid, qx, qy, r, s, gst, bits, dst, tst, hsh, dig, mid, row, bitc, tdig, cspan, tfl;
    // idemix creators, rows by creator rank (all empty without an idemix MSP): six 32-byte columns, issuer, message span, issuer out, then
    // the nym launch's bitmap, status bytes, row -> rank list and rank -> row list
    WalkRegion nymf, nymi, nymsp, nymio, nymb, nymst, nymga, nymsl;
    WalkRegion tqxy, sparts;
    WalkRegion wide, bita;            // the wide kernels' w and u2 Q of every row between their two phases, and the one bitmap of the second
    WalkRegion ment, mslots, mkoff, mkeys, mst, mtot, mdig, mhsp, mhsl, mtiles;   // the memo; mtiles: the entry scan's tiles (walk_memo_tile_*_kernel)
    WalkRegion nym_zeroed;            // NOT a region of its own: nymf .. nymsp as one span - rows of creators that are not idemix stay all-zero
    size_t nym_col = 0;               // bytes of one column of nymf
    size_t dev_keys_cap = 0;
    size_t total = 0;
    static constexpr size_t N = 48;
    const WalkRegion* regions() const { return &tup; }
};
constexpr WalkTupleLayout walk_tuple_layout(const WalkTupleShape& s) {
    WalkCarver c{0, WALK_DEV_ALIGN};
    WalkTupleLayout L;
    const size_t nt = s.nt, np = s.np, nc = s.nc, cr = s.creators, words = (nt + 63) / 64;
    const bool nym = s.n_msps != 0, wide = s.nt <= (uint32_t)WIDE_LAUNCH_MAX, hmemo = s.memo && s.hmemo;
    L.tup = c.take(nt * sizeof(bccsp::BlockTuple));
    L.pre = c.take((np + 1) * 8);
    L.chk = c.take((nc + 1) * sizeof(bccsp::BlockHashCheck));
    L.gsp = c.take((nc + 1) * 24);
    L.gof = c.take((nc + 1) * 4);
    L.gdg = c.take((nc + 1) * 32);
    L.idx = c.take(nt * 4);
    L.off = c.take(nt * 8);
    L.pix = c.take(nt * 4);
    L.kid = c.take(nt * 4);
    L.qx = c.take(nt * 32);
    L.qy = c.take(nt * 32);
    L.r = c.take(nt * 32);
    L.s = c.take(nt * 32);
    L.gst = c.take(nt);
    L.bits = c.take(words * 8);
    L.dst = c.take(nt);
    L.tst = c.take(nt);
    L.hsh = c.take(nt);
    L.dig = c.take(nt * 32);
    L.mid = c.take((np + 1) * 32);
    L.row = c.take(nt * 4);
    L.bitc = c.take(words * 8);
    L.tdig = c.take(nt * 32);
    L.cspan = c.take((cr + 1) * 8);
    L.tfl = c.take(nt);
    L.nym_col = 32 * cr;
    L.nymf = c.take(nym ? 6 * L.nym_col : 0);
    L.nymi = c.take(nym ? cr * 4 : 0);
    L.nymsp = c.take(nym ? cr * 8 : 0);
    L.nymio = c.take(nym ? cr * 4 : 0);
    L.nymb = c.take(nym ? walk_nym_bits_bytes(cr) : 0);
    L.nymst = c.take(nym ? walk_nym_status_bytes(cr) : 0);
    L.nymga = c.take(nym ? cr * 4 + 256 : 0);
    L.nymsl = c.take(nym ? cr * 4 : 0);
    L.tqxy = c.take(s.tuple_qxy ? nt * 64 : 0);
    L.sparts = c.take((nt + 255) / 256 * sizeof(WalkSummary));
    L.wide = c.take(wide ? nt * WIDE_SCRATCH_BYTES : 0);
    L.bita = c.take(wide ? words * 8 : 0);
    // (on the device the keys have room for the longest signatures the memo takes - 1 024 bytes each; what is copied ahead is the room
    //  the caller gave, sized for ordinary signatures; a block that needs more gets the rest through WalkRequest::memo_grow at the end)
    L.dev_keys_cap = s.memo ? (size_t)std::min<uint64_t>(0xFFFFFFE0ull, std::max<uint64_t>(s.memo_keys_cap, (uint64_t)nt * (141 + 1024) + 256)) : 0;
    L.ment = c.take(s.memo ? nt * 4 : 0);
    L.mslots = c.take(s.memo ? (size_t)s.memo_slot_cap * 4 : 0);
    L.mkoff = c.take(s.memo ? (nt + 1) * 4 : 0);
    L.mkeys = c.take(L.dev_keys_cap);
    L.mst = c.take(s.memo ? nt : 0);
    L.mtot = c.take(s.memo ? sizeof(WalkMemoTotals) : 0);
    L.mdig = c.take(s.memo ? nt * 32 : 0);
    L.mhsp = c.take(hmemo ? nt * 16 : 0);
    L.mhsl = c.take(hmemo ? (size_t)s.memo_slot_cap * 4 : 0);
    L.mtiles = c.take(s.memo ? (nt / 2048 + 2) * 24 : 0);
    L.total = c.at;
    L.nym_zeroed = walk_span({L.nymf, L.nymi, L.nymsp}, WALK_DEV_ALIGN);
    return L;
}
// (nym_zeroed ends where nymio starts: one fill clears the three arrays in front of it and nothing else)
constexpr bool walk_nym_rows_adjacent(const WalkTupleLayout& L) {
    return walk_back_to_back({L.nymf, L.nymi, L.nymsp, L.nymio}, WALK_DEV_ALIGN) && L.nym_zeroed.off == L.nymf.off &&
           L.nym_zeroed.off + L.nym_zeroed.bytes == L.nymio.off;
}

// ---- pinned staging (fabgpu_ctx::walk_pin): [0, first) mirrors what goes up, the arrays that come back follow ----
struct WalkPinLayout {
    WalkRegion type, und, tup, dig, pre, chk, sigs, qxy, nymi;
    size_t first = 0, total = 0;
    static constexpr size_t N = 9;
    const WalkRegion* regions() const { return &type; }
};
constexpr size_t walk_pin_first(const WalkEnvLayout& e) { return walk_round_up(e.up_all, 256); }
constexpr WalkPinLayout walk_pin_layout(const WalkEnvLayout& e, uint32_t ne, const WalkTupleShape& s, uint32_t n_block_sigs, bool nym_issuer) {
    WalkPinLayout L;
    L.first = walk_pin_first(e);
    WalkCarver c{L.first, WALK_HOST_ALIGN};
    const size_t nt = s.nt;
    L.type = c.take(ne);
    L.und = c.take(ne);
    L.tup = c.take(nt * sizeof(bccsp::BlockTuple));
    L.dig = c.take(nt * 32);
    L.pre = c.take(((size_t)s.np + 1) * 8);
    L.chk = c.take(((size_t)s.nc + 1) * sizeof(bccsp::BlockHashCheck));
    L.sigs = c.take((size_t)n_block_sigs * sizeof(bccsp::BlockTuple) + 64);
    L.qxy = c.take(s.tuple_qxy ? nt * 64 : 0);
    L.nymi = c.take(nym_issuer ? (size_t)s.creators * 4 : 0);
    L.total = c.at;
    return L;
}

// ---- host-mapped results (fabgpu_ctx::walk_map) ----
// [0, 64) the totals' flag, [64, 128) the totals, [128, 192) the final flag, [192, 256) the summary (48 bytes), [256, 320) the memo's
// totals (24 bytes); the arrays follow
constexpr size_t WALK_MAP_TOTFLAG = 0, WALK_MAP_TOT = 64, WALK_MAP_FINFLAG = 128, WALK_MAP_SUM = 192, WALK_MAP_MTOT = 256, WALK_MAP_ARRAYS = 320;
static_assert(sizeof(WalkTotals) <= 64 && sizeof(WalkSummary) <= 64 && sizeof(WalkMemoTotals) <= 64, "one 64-byte cell each");
struct WalkMapLayout {
    WalkRegion learn, flags, type, und, tst, hsh, idx;
    size_t total = 0;
    static constexpr size_t N = 7;
    const WalkRegion* regions() const { return &learn; }
};
// what the pass makes sure of before the totals are known (they arrive in this buffer)
constexpr size_t walk_map_early_bytes(uint32_t ne) {
    return WALK_MAP_ARRAYS + sizeof(WalkLearn) * WALK_LEARN_SLOTS + 3 * walk_round_up(ne, 64) + ((size_t)8 << 10);
}
constexpr WalkMapLayout walk_map_layout(uint32_t ne, uint32_t nt) {
    WalkCarver c{WALK_MAP_ARRAYS, WALK_HOST_ALIGN};
    WalkMapLayout L;
    L.learn = c.take(sizeof(WalkLearn) * WALK_LEARN_SLOTS);
    L.flags = c.take(ne);
    L.type = c.take(ne);
    L.und = c.take(ne);
    L.tst = c.take(nt);
    L.hsh = c.take(nt);
    L.idx = c.take((size_t)nt * 4);
    L.total = c.at;
    return L;
}

static_assert(offsetof(WalkEnvLayout, stash) == (WalkEnvLayout::N - 1) * sizeof(WalkRegion) &&
                  offsetof(WalkTupleLayout, mtiles) == (WalkTupleLayout::N - 1) * sizeof(WalkRegion) &&
                  offsetof(WalkPinLayout, nymi) == (WalkPinLayout::N - 1) * sizeof(WalkRegion) &&
                  offsetof(WalkMapLayout, idx) == (WalkMapLayout::N - 1) * sizeof(WalkRegion),
              "regions() walks the N regions as an array: they come first, in carving order");

// ---- the largest pass of a given size ----
// The slot table the provider gives a pass of nt tuples (GPUCSP::MemoPinLayout takes it from here): the power of two >= 2 nt, 16 at least.
constexpr uint32_t walk_memo_slot_cap(uint32_t nt) {
    uint32_t cap = 16;
    while (cap < 2 * (uint64_t)nt && cap < (1u << 30)) cap <<= 1;
    return cap;
}
struct WalkSizes {
    size_t env = 0, tup = 0, pin = 0, map = 0;
};
// The four totals no pass over at most n_tx envelopes and n_tuples tuples exceeds: what walk_preallocate makes, so that no pass of a
// fresh provider allocates.  Every option is on, and every count is at its bound:
//   n_msps     = WALK_IDEMIX_MSPS_MAX                 (walk_block_pass clamps to it), with issuer hashes
//   early_hash = on, host_counted = off               (off keeps the stash, the largest per-envelope array; the region [0, up_all) is
//                                                      laid out either way)
//   creators  <= min(n_tx, n_tuples)                  (WalkTotals: an envelope that yields tuples yields exactly one creator tuple)
//   np        <= nt                                   (walk_envelope: add_prefix once per action, in front of that action's endorsement
//                                                      tuples.  An action WITHOUT endorsements adds a prefix and no tuple, so a crafted
//                                                      block can exceed this; no peer builds one - the gateway refuses a transaction nobody
//                                                      endorsed - and such a pass is still served: it grows its buffers as before)
//   nc        <= creators + np                        (walk_envelope: add_check once per envelope behind its creator tuple - CheckTxID -
//                                                      and once per action - GetProposalHash2; a rolled-back envelope keeps none.  The
//                                                      "4 tuples + 1 prefix + 2 hash checks" at EnvStash is the typical endorser
//                                                      transaction, not a bound)
//   n_block_sigs <= nt                                (they are among the nt tuples)
//   memo + hmemo on, the slot table the provider picks for nt tuples (walk_memo_slot_cap), memo_keys_cap at most the device's own room
//                                                     (GPUCSP::MemoPinLayout gives nt * 205 + creators * 32 + 256: below nt * 1 165 + 256)
//   tuple_qxy, nym_issuer on
// Every region grows with its counts except the wide kernels' (only for nt <= WIDE_LAUNCH_MAX): the tuple buffer is the larger of the
// layout at n_tuples and the one at WIDE_LAUNCH_MAX tuples.
constexpr WalkSizes walk_worst_case(uint32_t n_tx, uint32_t n_tuples) {
    WalkEnvShape es;
    es.ne = n_tx;
    es.n_msps = WALK_IDEMIX_MSPS_MAX;
    es.early_hash = es.has_issuer_hashes = true;
    es.host_counted = false;
    const WalkEnvLayout e = walk_env_layout(es);
    WalkSizes w;
    w.env = e.total;
    for (const uint32_t nt : {n_tuples, std::min<uint32_t>(n_tuples, (uint32_t)WIDE_LAUNCH_MAX)}) {
        WalkTupleShape ts;
        ts.nt = ts.np = nt;
        ts.creators = std::min(n_tx, nt);
        ts.nc = ts.creators + ts.np;
        ts.n_msps = WALK_IDEMIX_MSPS_MAX;
        ts.tuple_qxy = ts.memo = ts.hmemo = true;
        ts.memo_slot_cap = walk_memo_slot_cap(nt);
        ts.memo_keys_cap = 1;
        w.tup = std::max(w.tup, walk_tuple_layout(ts).total);
        w.pin = std::max(w.pin, walk_pin_layout(e, n_tx, ts, nt, true).total);
        w.map = std::max({w.map, walk_map_early_bytes(n_tx), walk_map_layout(n_tx, nt).total});
    }
    return w;
}
// The estimates walk_preallocate used before the layout was written down, kept as a FLOOR (no provider gets less than it did).
constexpr WalkSizes walk_preallocate_floor(uint32_t n_tx, uint32_t n_tuples) {
    const size_t ne = n_tx, nt = n_tuples;
    WalkSizes f;
    f.env = ne * (128 + sizeof(bccsp::walk::EnvStash)) + ((size_t)256 << 10);
    f.tup = nt * 2112 + ne * 256 + ((size_t)1 << 20);
    f.pin = nt * 256 + ne * 160 + ((size_t)256 << 10);
    f.map = nt * 8 + ne * 8 + sizeof(WalkLearn) * WALK_LEARN_SLOTS + ((size_t)64 << 10);
    return f;
}
// The gather scratch (fabgpu_ctx::gscr) holds the TxID and proposal-hash inputs stitched together: bytes of the block, which no count
// bounds.  An estimate, kept from before: a few KB per transaction.
constexpr size_t walk_gather_scratch_estimate(uint32_t n_tx) { return (size_t)n_tx * 4096 + ((size_t)64 << 10); }
constexpr WalkSizes walk_preallocate_sizes(uint32_t n_tx, uint32_t n_tuples) {
    const WalkSizes w = walk_worst_case(n_tx, n_tuples), f = walk_preallocate_floor(n_tx, n_tuples);
    return WalkSizes{std::max(w.env, f.env), std::max(w.tup, f.tup), std::max(w.pin, f.pin), std::max(w.map, f.map)};
}

namespace walk_layout_checks {
constexpr WalkTupleShape sample(uint32_t n_msps) {
    WalkTupleShape s;
    s.nt = 1000; s.np = 250; s.nc = 500; s.creators = 250; s.n_msps = n_msps;
    return s;
}
static_assert(walk_nym_rows_adjacent(walk_tuple_layout(sample(0))) && walk_nym_rows_adjacent(walk_tuple_layout(sample(3))),
              "nym_zeroed is filled with one memset: nymf, nymi, nymsp lie back to back in front of nymio");
}  // namespace walk_layout_checks

}  // namespace fab
