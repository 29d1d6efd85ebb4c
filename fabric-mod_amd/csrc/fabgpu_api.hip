// C-ABI shim (include/fabgpu.h) over the HIP kernels: context, staging, launches.
// One context = one GPU + one HIP stream; host entry points stage through pinned buffers the context
// owns (nothing of the caller's memory is retained after return - cgo pointer rules).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <initializer_list>
#include <memory>
#include <sys/mman.h>
#include <set>
#include <mutex>
#include <new>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fabgpu.h"
#include "kernels.h"
#include "key_slots.h"
#include "keyed_fence.h"
#include "block_walk_dev.h"
#include "described_plan.h"
#include "walk_layout.h"
#include "worker_pool.h"
#include "bn_tables29.h"
#include "p256_tables29.h"
#include "p384.h"
#include "p384_keys.h"
#include "p384_tables.h"
#include "p384_tables16.h"

using namespace fab;

namespace {

struct Buf {  // growable pinned-host + device pair
    void* h = nullptr;
    void* d = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return FABGPU_OK;
        release();
        size_t want = bytes + bytes / 4 + 256;
        if (hipHostMalloc(&h, want, hipHostMallocDefault) != hipSuccess) { h = nullptr; return FABGPU_ENOMEM; }
        if (hipMalloc(&d, want) != hipSuccess) { hipHostFree(h); h = nullptr; d = nullptr; return FABGPU_ENOMEM; }
        cap = want;
        return FABGPU_OK;
    }
    void release() {
        if (h) hipHostFree(h);
        if (d) hipFree(d);
        h = d = nullptr;
        cap = 0;
    }
};

struct DevBuf {  // growable device-only buffer
    void* d = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return FABGPU_OK;
        release();
        size_t want = bytes + bytes / 4 + 256;
        if (hipMalloc(&d, want) != hipSuccess) { d = nullptr; return FABGPU_ENOMEM; }
        cap = want;
        return FABGPU_OK;
    }
    void release() {
        if (d) hipFree(d);
        d = nullptr;
        cap = 0;
    }
};
// Pinned host memory on 2 MiB pages, for tables and block copies that the HOST reads at random (the verdict / digest memo: every
// validator thread, every signature): transparent huge pages where the kernel grants them on request (THP "madvise" or "always"),
// registered with the runtime so that DMA treats it like hipHostMalloc'd memory.  A memo lookup touches a handful of places in a few
// tens of MB that DMA wrote - cold in every cache AND, on 4 KiB pages, in every TLB: each touch then pays for a page walk whose
// entries are cold as well.  nullptr: not available here (the caller falls back to hipHostMalloc).
static void* pinned_huge_alloc(size_t bytes) {
    constexpr size_t huge = (size_t)2 << 20;
    const size_t want = (bytes + huge - 1) & ~(huge - 1);
    void* p = nullptr;
    if (posix_memalign(&p, huge, want) != 0 || !p) return nullptr;
    (void)madvise(p, want, MADV_HUGEPAGE);
    for (size_t o = 0; o < want; o += 4096) ((volatile uint8_t*)p)[o] = 0;      // fault the pages in now (huge ones where granted), not inside a pass
    if (hipHostRegister(p, want, hipHostRegisterPortable) != hipSuccess) {
        (void)hipGetLastError();
        free(p);
        return nullptr;
    }
    return p;
}
static void pinned_huge_free(void* p) {
    if (!p) return;
    (void)hipHostUnregister(p);
    free(p);
}

struct PinBuf {  // growable pinned host buffer
    void* h = nullptr;
    size_t cap = 0;
    unsigned flags = hipHostMallocDefault;
    bool want_huge = false;   // try 2 MiB pages first (pinned_huge_alloc)
    bool is_huge = false;
    int ensure(size_t bytes) {
        if (bytes <= cap) return FABGPU_OK;
        release();
        size_t want = bytes + bytes / 4 + 256;
        if (want_huge && (h = pinned_huge_alloc(want)) != nullptr) {
            is_huge = true;
            cap = want;
            return FABGPU_OK;
        }
        if (hipHostMalloc(&h, want, flags) != hipSuccess) { h = nullptr; return FABGPU_ENOMEM; }
        cap = want;
        return FABGPU_OK;
    }
    void release() {
        if (h && is_huge) pinned_huge_free(h);
        else if (h) hipHostFree(h);
        h = nullptr;
        cap = 0;
        is_huge = false;
    }
};

// what KeyedFence (keyed_fence.h) asks of the device
struct HipFenceDev {
    using Event = hipEvent_t;
    using Stream = hipStream_t;
    static bool ok(hipError_t e) {
        if (e != hipSuccess) (void)hipGetLastError();
        return e == hipSuccess;
    }
    static Event make_event() {
        Event e = nullptr;
        return ok(hipEventCreateWithFlags(&e, hipEventDisableTiming)) ? e : nullptr;
    }
    static void destroy_event(Event e) { hipEventDestroy(e); }
    static bool record(Event e, Stream s) { return ok(hipEventRecord(e, s)); }
    static FenceQuery query(Event e) {
        const hipError_t r = hipEventQuery(e);
        return ok(r) ? FenceQuery::DONE : r == hipErrorNotReady ? FenceQuery::NOT_READY : FenceQuery::FAILED;
    }
    static void wait(Event e) { (void)ok(hipEventSynchronize(e)); }
    static bool sync(Stream s) { return ok(hipStreamSynchronize(s)); }
};
using HipKeyedFence = KeyedFence<HipFenceDev>;

}  // namespace

struct fabgpu_ctx {
    int device = 0;
    bool allow_pair = true;   // !FABGPU_FLAG_ONE_LANE_ONLY
    bool allow_quad = true;   // !FABGPU_FLAG_NO_QUAD (idemix: four lanes per signature for batches <= IDEMIX_QUAD_MAX)
    bool nym_side_stream = true; // !FABGPU_FLAG_NYM_NO_SIDE_STREAM (idemix four-lane form: the fixed-base terms on a second stream beside the commitments)
    std::atomic<bool> test_nym_side_after{false};   // TEST HOOK (fab::ctx_test_nym_side_after; read once per nym launch, handed to the launcher as a parameter)
    bool nym_two_phase = true;   // !FABGPU_FLAG_NYM_FUSED_HASH (idemix four-lane form: commitments, then challenges with eight lanes on a message)
    bool allow_wide = true;   // !FABGPU_FLAG_NO_WIDE (registered keys: eight lanes per signature in two phases for launches <= WIDE_LAUNCH_MAX)
    int pair_table_lds = -1;       // the verify-only pair kernel's per-signature table: 1 in LDS, 0 in the global workspace, -1 by batch size (kernels.h)
    bool pair_solo = false;        // FABGPU_FLAG_PAIR_SOLO: the LDS-table pair kernel without helper waves
    bool pair_dbl1 = false;        // FABGPU_FLAG_PAIR_DBL1: the LDS-table pair kernels with the per-doubling loop
    bool pair_table_add = false;   // FABGPU_FLAG_PAIR_TABLE_ADD: the LDS-table pair kernels with the odd multiples by general additions
    bool pair_booth4 = false;      // FABGPU_FLAG_PAIR_BOOTH4: the LDS-table pair kernels with Booth digits and 65 windows
    hipStream_t stream = nullptr;
    // FABGPU_FAULT_INJECT (tests of the failure contract only): "launch" makes every kernel submission report hipErrorLaunchFailure,
    // "oom" makes every workspace / staging allocation fail.  A non-zero return must then reach the caller and no verdict may be written.
    int fault = 0;
    int32_t* d_gtab = nullptr;
    uint32_t* d_gtab384 = nullptr;   // P-384: j G, j = 1 .. 15 (p384.h build_gtab), 1 440 bytes; made by the first P-384 call (p384_gtab)
    std::mutex gtab384_mu;
    std::mutex mu;
    Buf fields;   // qx|qy|e|r|s
    Buf arena;    // message bytes
    Buf offs;     // u32 offsets
    Buf out;      // verdict words | status bytes | digests
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool time_kernels = false;   // FABGPU_FLAG_TIME_KERNELS: bracket every launch with two timing events (fabgpu_last_kernel_ms); off by
                                 // default - two more packets per launch between back-to-back kernels are not free
    // Workspaces for the verify kernels' per-lane j*Q tables.  A launch borrows one: `reserved` from acquire until release has
    // recorded an event behind the kernel, `armed` from then until that event completes - two separate flags, because between
    // acquire and release the event is stale (or was never recorded) and hipEventQuery on it would answer "done".
    // acquire hands the POINTER out under the lock: the vector may grow while the caller launches.
    struct QWs {
        void* p = nullptr;
        size_t bytes = 0;
        hipEvent_t done = nullptr;
        bool reserved = false;   // handed to a launch that has not recorded `done` yet
        bool armed = false;      // `done` was recorded behind the launch that used it
        NymSide nym_side;             // idemix four-lane form: the side stream of the fixed-base launch and its fork / join events (made on first use)
        hipStream_t last = nullptr;   // the stream of that launch: a later launch on the SAME stream runs behind it anyway and may
                                      // take the workspace without waiting (20 queued steps of a bench loop used to mean 20 workspaces
                                      // of 61 MB each, allocated inside the timed region)
    };
    std::vector<QWs> qws;
    // Registered public keys: one 640 KiB comb table each, resident on the device; d_ktabs mirrors the pointer array.
    std::mutex kmu;
    std::vector<int32_t*> ktabs;            // per SLOT (kslots.high_water() of them): the 8-bit comb d_ktabs shows for it
    std::map<std::string, uint32_t> key_ids;   // qx||qy -> id, live keys only
    const int32_t** d_ktabs = nullptr;      // KTAB_STRIDE words per slot (kernels.h): the 8-bit comb, the 16-bit comb or nullptr, the generation
    size_t d_ktabs_cap = 0;                 // (in slots)
    // Retiring keys (fabgpu_p256_key_unregister; key_slots.h has the ids).  A retirement takes the key out of key_ids and leaves the
    // device alone; the slot and its tables then pass the wait of keyed_fence.h (the launchers, the streams, the events: fence256, under
    // kmu) TWICE before anything of them is used again, because d_ktabs is edited in place, under launches that read it:
    //   phase 1  behind events recorded AT the retirement (and on the 16-bit builder's stream, if the key had a build queued): whatever
    //            was enqueued before the retirement finds the old key and answers for it;
    //   phase 2  at a quiet moment the host sets the slot's generation word to KTAB_GEN_NONE, and events recorded THEN have completed:
    //            nothing that could have seen the old generation is running.  Only now the tables go to the free lists and the slot may
    //            be handed out again - pointers first, the new generation last, both written by the host before the new id is returned.
    // Phases advance on the registration paths (kdrain_advance_locked), never on a verify call or a block pass; a registration whose
    // slot (the LOWEST reclaimable one, always) is still draining waits for that slot's drain alone.
    fab::KeySlots kslots;
    std::vector<std::string> kname;         // per slot: its tenant's qx||qy
    std::vector<uint32_t> kgen_dev;         // per slot: the generation word the device shows
    struct KeyDrain {
        uint32_t slot = 0;
        int phase = 1;
        std::vector<hipEvent_t> evs;
        int32_t* t8 = nullptr;
        void* t16 = nullptr;
        int idx16 = -1;
    };
    std::vector<KeyDrain> kdrains;          // oldest first
    HipKeyedFence fence256;                 // (its events also serve k16_pending: one of those may end up in a drain)
    hipStream_t stream_kslot = nullptr;     // the host's few-byte writes into d_ktabs
    std::vector<void*> retired;   // outgrown d_ktabs arrays, freed at shutdown
    // Round 6, FABGPU_FLAG_KEY_TABLES_16BIT: a registered key also gets a 16-bit comb (CombTab<16>, 80 MiB - the generator's own format),
    // built on stream_keytab BEHIND the registration (nobody waits for it; its pointer reaches d_ktabs[2 k + 1] by a copy queued after
    // the build, so a launch sees nullptr or a finished table).  Up to KTAB16_MAX keys: 5 GiB of a 288 GB device.  All under kmu.
    bool key_tables_16 = false;
    hipStream_t stream_keytab16 = nullptr;  // (its own: a registration waits on stream_keytab for the 8-bit table and must not find an 80 MiB build queued there)
    static constexpr size_t KTAB16_MAX = 64;
    std::vector<void*> ktab16;              // per slot: the table, or nullptr
    std::vector<int> ktab16_idx;            // per slot: which room and pinned head its build used, or -1
    std::vector<void*> ktab16_free;         // tables, rooms + heads of retired keys, drained
    std::vector<int> ktab16_idx_free;
    size_t ktab16_idx_next = 0;             // rooms + heads handed out for the first time so far
    // a REUSED slot's 16-bit pointer is not written from the builder's stream: the host writes it, under kmu, once the build's event
    // has completed (k16_publish_locked, on the next registration, retirement or stats call - never on a verify call or a pass)
    struct Pending16 { uint32_t slot; void* tab; hipEvent_t built; };
    std::vector<Pending16> k16_pending;
    std::vector<void*> ktab16_slabs;        // tables come from slabs of KTAB16_SLAB (the first one at fabgpu_init: a registration must not pay for an 80 MiB hipMalloc)
    static constexpr size_t KTAB16_SLAB = 8;
    size_t ktab16_carved = 0;               // tables handed out of the slabs so far
    void* ktab16_rooms = nullptr;           // KTAB16_MAX builders' rooms (key + pointer + scratch), one allocation
    uint8_t* ktab16_heads = nullptr;        // pinned host memory, KTAB16_MAX x 128 bytes: what each build's upload reads (reused only behind the build's drain: the copies are asynchronous)
    size_t ktab16_room_bytes = 0;
    size_t ktab16_count = 0;                // LIVE keys with a 16-bit table (built or building); KTAB16_MAX caps live + draining ones
    // Where the tables live: slabs of KTAB_SLAB tables (a table is never freed before shutdown, and hipMalloc / hipFree per table were
    // most of what a registration cost once the tables were built on the device: 4.7 ms of runtime calls around 0.8 ms of kernels for a
    // channel's six signers).  ktab_free: tables whose installation failed, and those of retired keys once drained.  All under kmu.
    static constexpr size_t KTAB_SLAB = 32;
    std::vector<void*> ktab_slabs;
    size_t ktab_slab_used = KTAB_SLAB;
    std::vector<int32_t*> ktab_free;
    // the device builder's room (keytab_kernels.hip): keys + table pointers in, the chain's and the affine bases' scratch; its own stream
    std::mutex ktab_build_mu;
    void* d_ktab_in = nullptr;
    void* d_ktab_scr = nullptr;
    size_t ktab_in_cap = 0, ktab_scr_cap = 0;
    hipStream_t stream_keytab = nullptr;
    // Registered P-384 keys (p384_keys.h has the book, p384_keytab_kernels.hip the builder, p384_keyed_kernels.hip the reader).  One comb
    // table of 1.125 MiB per key, allocated at its registration; the generator's comb is the same builder run on G at the first
    // registration or keyed call - a context that never meets a registered P-384 key allocates none of this.
    // A keyed launch is handed d_snap384: the book's snapshot, written completely (and waited for) by the registration or retirement
    // that changed the book, before it replaces the previous array, and never edited afterwards.  Nothing is published under a running
    // launch.  What a change of the book leaves behind - the previous snapshot array, and a retired key's slot and table - passes the wait
    // of keyed_fence.h (fence384, under k384_mu) ONCE before it is used again (Drain384): nobody takes the old array any more, so one
    // quiet moment and the events recorded then are all it needs.  Drains advance on the registration, retirement and stats paths, never
    // on a verify call; a registration whose slot - the lowest reclaimable one, always (key_slots.h) - is still draining waits for that slot.
    // Lock order: k384_build_mu, k384_mu, the fence's leaf.
    std::mutex k384_mu;
    fab::P384KeyBook k384;
    uint32_t* d_gcomb384 = nullptr;
    const fab::P384SlotSnap* d_snap384 = nullptr;
    uint32_t snap384_n = 0;                  // the high-water mark d_snap384 was taken at
    size_t snap384_cap = 0;                  // (slots) of d_snap384
    struct Snap384Room { void* p; size_t cap; };
    std::vector<Snap384Room> snap384_free;   // drained snapshot arrays (nothing is freed before shutdown: hipFree waits for the device)
    std::vector<void*> k384_allocs;          // every table and snapshot array ever made
    uint64_t k384_n_tables = 0, k384_snap_bytes = 0;   // ... how many of them are tables (the generator's included), and the arrays' bytes
    std::vector<uint32_t*> k384_tab_free;    // tables of retired keys, drained, and of builds that were not installed
    struct Drain384 {
        int64_t slot = -1;                   // -1: only an array to give back
        uint32_t* tab = nullptr;
        uint32_t* tab16 = nullptr;           // the tenant's 16-bit table, finished or (its event is in evs) still being built
        Snap384Room old_snap{nullptr, 0};
        bool recorded = false;
        std::vector<hipEvent_t> evs;
    };
    std::vector<Drain384> k384_drains;       // oldest first
    HipKeyedFence fence384;                  // (its events also serve k384_pending16: one of those may end up in a drain)
    std::atomic<uint64_t> k384_launches{0};  // keyed P-384 launches queued so far (fabgpu_p384_key_table_stats)
    // FABGPU_FLAG_P384_WIDE (or fab::ctx_set_p384_wide): keyed launches of at most P384_WIDE_LAUNCH_MAX rows on eight lanes per signature.
    // Their scratch is a workspace of the qws pool, always asked for at its full size and made when the switch is turned on: a launch
    // finds it there (a second one is made only when keyed launches of several streams overlap).
    std::atomic<bool> p384_wide{false};
    std::atomic<uint64_t> k384_wide_rows{0}; // rows handed to the eight-lane form so far (fabgpu_p384_wide_rows)
    // FABGPU_FLAG_SHA3_COOP (or fab::ctx_set_sha3_coop): SHA3-256 launches of at most SHA3_COOP_MAX messages on 32 lanes per message, larger
    // plain ones through the mixed kernel (sha3_coop_kernels.hip).  sha3_coop_rows: the rows of the small launches, counted when they are
    // queued; d_sha3_coop_rows: the long rows the mixed kernel picked out, counted on the device (made when the switch is first turned on).
    std::atomic<bool> sha3_coop{false};
    std::atomic<uint64_t> sha3_coop_rows{0};
    unsigned long long* d_sha3_coop_rows = nullptr;
    // FABGPU_FLAG_P384_KEY_TABLES_16BIT (DESIGN 4.2d "16-bit tables").  The generator's 16-bit table is built once, beside its 8-bit one.
    // A registration queues its key's 16-bit build on stream_k384x16 behind the finished 8-bit table and does NOT wait for it: the
    // build waits in k384_pending16 with its event.  The launch path (and the stats path) asks hipEventQuery, never a blocking wait for
    // a build; a finished table goes into the book, and the book's next snapshot - a fresh array, written whole and waited for, as
    // always - carries its address.  At most k384_tab16_cap tables are live or being built; later keys, and keys whose hipMalloc
    // failed, have none and stay on the 8-bit stream.  A retired key's 16-bit table (or unfinished build) drains with its slot.
    bool p384_tab16 = false;
    uint32_t* d_gcomb384x16 = nullptr;
    unsigned long long* d_k384_rows16 = nullptr;   // rows of the wavefronts that ran 24 windows (fabgpu_p384_tables16_rows)
    uint32_t k384_tab16_cap = FABGPU_P384_MAX_TABLES16;
    struct Pending384x16 { uint32_t id; uint32_t* tab; hipEvent_t ev; };
    std::vector<Pending384x16> k384_pending16;
    std::vector<uint32_t*> k384_tab16_free;  // 16-bit tables of retired keys, drained
    uint64_t k384_n_tables16 = 0;            // 16-bit tables ever allocated (the generator's included)
    const uint32_t* const* d_snap384x16 = nullptr;   // the second address per slot: behind the slots of d_snap384, in the same array
    hipStream_t stream_k384x16 = nullptr;
    std::mutex k384_build_mu;                // one build at a time: the builder's room and stream are one
    void *d_k384_in = nullptr, *d_k384_scr = nullptr;
    size_t k384_in_cap = 0, k384_scr_cap = 0;
    hipStream_t stream_k384 = nullptr;       // the builds, and the few bytes of a snapshot
    // Registered idemix issuers: a fixed-capacity device array of slots (idemix_kernels.hip IssuerDev); a slot is written
    // before n_issuers is raised, so launches in flight never read a half-written one.
    std::mutex imu;
    void* d_issuers = nullptr;
    std::vector<int32_t*> itabs;                  // two comb tables per issuer
    std::map<std::string, uint32_t> issuer_ids;   // hsk || hrand || hash -> id
    Buf nym;          // staging of the nym host-pointer entry point: issuer_id | six fields (| spans, when they ride in an identity batch)
    Buf nymout;       // results of the pseudonym signatures that ride in an identity batch: verdict words | status bytes
    hipStream_t stream2 = nullptr;   // the pseudonym signatures of an identity batch run here, next to the ECDSA kernels on `stream`
    hipEvent_t ev_up = nullptr;      // "the arena is on the device" (recorded on stream, awaited by stream2)
    // the device block pass runs on four streams: walk / gates / endorsements on `stream`, the creators' hashes and launch on
    // stream2, the mid-states on stream3, the TxID / proposal-hash digests on stream4
    hipStream_t stream3 = nullptr, stream4 = nullptr;
    hipEvent_t ev_w[12] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool pred_has_nym = false;       // the previous block had idemix creators: queue the nym launch without waiting for the gates
    uint32_t pred_nym_rows = 0;      // ... and how many: the launch runs over that many packed rows plus a margin
    Buf gath;         // gathered hashes of an identity batch: spans | running offsets | digests
    DevBuf gscr;      // device scratch the gather kernel stitches the messages into
    // fabgpu_arena_stage: arenas uploaded ahead of the batches that refer to them.  A few slots, so that the channels of a peer
    // validating at once do not throw each other's block out between "staged" and "submitted" (with one slot, two callers cost
    // more per block than one: the loser uploaded its 50 MB a second time inside its device call).  A slot's mutex is held while
    // it is being filled and while a batch reads it; smu only guards the choice of a slot.  Lock order: smu, slot, mu.
    struct Staged {
        std::mutex m;
        void* d = nullptr;
        size_t cap = 0, len = 0;
        std::atomic<uint64_t> token{0};
    };
    static constexpr int N_STAGED = 3;
    std::mutex smu;
    Staged staged_slots[N_STAGED];
    uint64_t stage_seq = 0;
    Buf keyed;        // staging of the keyed host-pointer entry point: key_id | e | r | s
    Buf pre;          // staging of prefixed batches: pre_off | pre_idx | mid-states
    Buf tailbuf;      // staging of an identity batch's tail when the arena itself bypasses the pinned buffer
    // the block pass on the device (block_walk_dev.h): per-envelope arrays, per-tuple arrays, pinned staging for what travels, and
    // the table of identities the provider has met (slots | entries | bytes in one allocation, swapped whole under mu)
    DevBuf walk_env, walk_tup, idtab_buf;
    PinBuf stage_pin;                // fabgpu_arena_stage: pinned staging of arenas that arrive in pageable memory
    std::mutex stage_pin_mu;
    // arena_stage_keep: staging buffers that STAY with the caller after the upload (block_walk_dev.h HostCopy - the host copy of a block
    // the provider's digest memo compares bccsp.Hash callers' bytes with, until the block's validation has returned).  A small pool:
    // buffers are made on demand up to keep_max, handed back by host_copy_release, and reused (pinning 64 MiB costs milliseconds).
    struct KeepBuf {
        PinBuf pin;
        bool in_use = false;
        KeepBuf() {
            pin.flags = hipHostMallocPortable;
            pin.want_huge = true;                 // read by the validators' threads, a few KB at 40 000 random places per block
        }
    };
    std::mutex keep_mu;
    std::vector<std::unique_ptr<KeepBuf>> keep_pool;
    uint32_t keep_max = 8;
    uint64_t keep_refused = 0;
    // The copiers of this context's uploads: threads of its own (made with the first big upload), so that the uploads of a provider's G
    // devices - each behind its own PCIe link - run side by side instead of taking turns on the process-wide pool of the host passes.
    std::unique_ptr<WorkerPool> stage_pool;
    hipStream_t stream_copy = nullptr;
    hipStream_t stream_copy_more[3] = {nullptr, nullptr, nullptr};   // further upload queues: pieces alternate between DMA engines
    PinBuf walk_pin;
    // what the pass's kernels write for the HOST (block_walk_dev.h WalkHostOut): pinned, mapped, coherent - the host polls flags in it
    PinBuf walk_map;
    uint32_t walk_seq = 0;
    void* d_idtab = nullptr;
    uint32_t idtab_n = 0, idtab_mask = 0;
    uint64_t idtab_seed = 0;
    // Which verify kernels the pass queues BEFORE it knows what the gates found (one host round trip less): the keyed ones for a launch
    // class (creators / everybody else) whose tuples all had comb tables in the previous pass, the fresh-key ones - always correct, the
    // key travels in the row - otherwise.  A wrong "keyed" guess is repaired by launching that class again (walk_block_pass).
    bool pred_keyed_creators = false, pred_keyed_others = false;
    size_t idtab_entries_off = 0, idtab_bytes_off = 0;
    std::mutex qmu;   // guards qws only (the host-pointer entry points call the _dev ones while holding mu)
    int acquire_qws(size_t bytes, size_t* idx, void** p, hipStream_t st);
    void release_qws(size_t idx, hipStream_t st) {
        std::lock_guard<std::mutex> lk(qmu);
        QWs& w = qws[idx];
        if (hipEventRecord(w.done, st) == hipSuccess) {
            w.armed = true;
            w.reserved = false;
            w.last = st;
        } else if (hipStreamSynchronize(st) == hipSuccess) {
            // no event to watch: wait the launch out, then the workspace is simply free again (a flapping device must not eat one per failure)
            w.armed = false;
            w.reserved = false;
        }
        // (neither worked: the workspace stays reserved - never shared with a launch that may still be reading it)
    }
};

int fabgpu_ctx::acquire_qws(size_t bytes, size_t* idx, void** p, hipStream_t st) {
    if (fault == 2) return FABGPU_ENOMEM;
    std::lock_guard<std::mutex> lk(qmu);
    for (size_t i = 0; i < qws.size(); i++) {
        QWs& w = qws[i];
        if (w.reserved) continue;                                          // somebody is between acquire and release
        const bool same_stream = w.armed && w.last == st;                  // stream order serialises the two launches
        if (w.armed && !same_stream && hipEventQuery(w.done) != hipSuccess) continue;      // still in flight on another stream
        if (w.bytes < bytes) {
            if (same_stream && hipEventQuery(w.done) != hipSuccess) continue;              // cannot free what a queued launch still reads
            if (w.p) hipFree(w.p);
            w.p = nullptr;
            w.bytes = 0;
            if (hipMalloc(&w.p, bytes) != hipSuccess) return FABGPU_ENOMEM;
            w.bytes = bytes;
        }
        w.armed = false;
        w.reserved = true;
        *idx = i;
        *p = w.p;
        return FABGPU_OK;
    }
    QWs w;
    if (hipEventCreateWithFlags(&w.done, hipEventDisableTiming) != hipSuccess) return FABGPU_ENODEV;
    if (hipMalloc(&w.p, bytes) != hipSuccess) {
        hipEventDestroy(w.done);
        return FABGPU_ENOMEM;
    }
    w.bytes = bytes;
    w.reserved = true;
    qws.push_back(w);
    *idx = qws.size() - 1;
    *p = w.p;
    return FABGPU_OK;
}

namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        hipGetDevice(&prev);
        if (prev != dev) hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) hipSetDevice(prev);
    }
};

int hip_to_rc(hipError_t e) { return e == hipSuccess ? FABGPU_OK : (e == hipErrorOutOfMemory ? FABGPU_ENOMEM : FABGPU_ELAUNCH); }
// the launch result an entry point reports: the real one, or the injected failure
inline hipError_t launched(const fabgpu_ctx* ctx, hipError_t e) { return ctx->fault == 1 ? hipErrorLaunchFailure : e; }

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the scratch of an eight-lane keyed P-384 launch, whatever its row count: one size, so that the pool's workspace always fits
constexpr size_t P384_WIDE_WS_BYTES = (size_t)P384_WIDE_LAUNCH_MAX * P384_WIDE_SCRATCH_BYTES;

// what the _dev entry points refuse: more rows or arena bytes than the kernels' 32-bit indices hold
inline bool dev_too_big(size_t n, size_t arena_bytes = 0) { return n > 0xFFFFFFF0ull || arena_bytes > 0xFFFFFFFFull; }

// The bracket around what a _dev entry point queues on st: a pooled workspace of ws_bytes (0: none) handed to launch(wsp) and given
// back behind it, the two timing events of FABGPU_FLAG_TIME_KERNELS (what fabgpu_last_kernel_ms reports), and the launch's result -
// or the injected failure - as a return code.
template <class Launch>
int timed_launch(fabgpu_ctx* ctx, hipStream_t st, size_t ws_bytes, Launch&& launch) {
    size_t wi = 0;
    void* wsp = nullptr;
    if (ws_bytes) {
        int rc = ctx->acquire_qws(ws_bytes, &wi, &wsp, st);
        if (rc != FABGPU_OK) return rc;
    }
    if (ctx->time_kernels) hipEventRecord(ctx->ev0, st);
    hipError_t err = launch(wsp);
    if (ctx->time_kernels) hipEventRecord(ctx->ev1, st);
    if (ws_bytes) ctx->release_qws(wi, st);
    ctx->timed = ctx->time_kernels;
    return hip_to_rc(launched(ctx, err));
}

// the fields every form of the verify launch shares; the caller names its key source and its digest source
VerifyLaunch verify_launch_common(const fabgpu_ctx* ctx, size_t n, const void* r, const void* s, void* verdict_bits, void* status) {
    VerifyLaunch v;
    v.n = (uint32_t)n;
    v.r = r; v.s = s;
    v.gtab = ctx->d_gtab;
    v.verdict_bits = verdict_bits; v.status = status;
    v.allow_pair = ctx->allow_pair;
    return v;
}

}  // namespace

extern "C" {

int fabgpu_abi_version(void) { return FABGPU_ABI_VERSION; }

const char* fabgpu_strerror(int code) {
    switch (code) {
        case FABGPU_OK: return "ok";
        case FABGPU_EINVAL: return "invalid argument";
        case FABGPU_ENODEV: return "no usable gfx950 device (HIP runtime/device unavailable); fall back to bccsp/sw";
        case FABGPU_ENOMEM: return "host or device allocation failed";
        case FABGPU_ELAUNCH: return "HIP launch/copy/execution failure";
        case FABGPU_ETOOBIG: return "batch or arena exceeds 32-bit offsets";
        case FABGPU_EPOISONED: return "provider poisoned: a CPU audit disagreed with the device; fall back to bccsp/sw";
        default: return "unknown fabgpu error";
    }
}

int fabgpu_device_count(fabgpu_ctx*) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return FABGPU_ENODEV;
    return n;
}

int fabgpu_init(const fabgpu_cfg* cfg, fabgpu_ctx** out) {
    if (!out) return FABGPU_EINVAL;
    *out = nullptr;
    if (cfg && (cfg->flags & ~(uint32_t)(FABGPU_FLAG_ONE_LANE_ONLY | FABGPU_FLAG_TIME_KERNELS | FABGPU_FLAG_NO_QUAD | FABGPU_FLAG_PAIR_TABLE_LDS |
                                          FABGPU_FLAG_PAIR_TABLE_GLOBAL | FABGPU_FLAG_NO_WIDE | FABGPU_FLAG_NYM_FUSED_HASH | FABGPU_FLAG_NYM_NO_SIDE_STREAM |
                                          FABGPU_FLAG_KEY_TABLES_16BIT | FABGPU_FLAG_PAIR_SOLO | FABGPU_FLAG_PAIR_DBL1 | FABGPU_FLAG_PAIR_BOOTH4 | FABGPU_FLAG_PAIR_TABLE_ADD | FABGPU_FLAG_P384_WIDE |
                                          FABGPU_FLAG_P384_KEY_TABLES_16BIT | FABGPU_FLAG_SHA3_COOP)) != 0) return FABGPU_EINVAL;
    if (cfg && (cfg->flags & FABGPU_FLAG_PAIR_TABLE_LDS) && (cfg->flags & FABGPU_FLAG_PAIR_TABLE_GLOBAL)) return FABGPU_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FABGPU_ENODEV;
    int dev = cfg ? cfg->device : -1;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) return FABGPU_ENODEV;
    }
    if (dev >= ndev) return FABGPU_EINVAL;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return FABGPU_ENODEV;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FABGPU_ENODEV;  // the code object is gfx950-only
    fabgpu_ctx* ctx = new (std::nothrow) fabgpu_ctx();
    if (!ctx) return FABGPU_ENOMEM;
    ctx->device = dev;
    ctx->walk_map.flags = hipHostMallocMapped | hipHostMallocCoherent;
    ctx->allow_pair = !(cfg && (cfg->flags & FABGPU_FLAG_ONE_LANE_ONLY));
    ctx->allow_quad = !(cfg && (cfg->flags & FABGPU_FLAG_NO_QUAD));
    ctx->nym_two_phase = !(cfg && (cfg->flags & FABGPU_FLAG_NYM_FUSED_HASH));
    ctx->nym_side_stream = !(cfg && (cfg->flags & FABGPU_FLAG_NYM_NO_SIDE_STREAM));
    ctx->key_tables_16 = cfg && (cfg->flags & FABGPU_FLAG_KEY_TABLES_16BIT);
    // (the wide form is built from the two-lane form's reasons: a context that may not use two lanes per signature does not use eight)
    ctx->allow_wide = ctx->allow_pair && !(cfg && (cfg->flags & FABGPU_FLAG_NO_WIDE));
    ctx->pair_table_lds = cfg && (cfg->flags & FABGPU_FLAG_PAIR_TABLE_LDS) ? 1 : (cfg && (cfg->flags & FABGPU_FLAG_PAIR_TABLE_GLOBAL) ? 0 : pair_table_default());
    ctx->pair_solo = cfg && (cfg->flags & FABGPU_FLAG_PAIR_SOLO);
    ctx->pair_dbl1 = cfg && (cfg->flags & FABGPU_FLAG_PAIR_DBL1);
    ctx->pair_booth4 = cfg && (cfg->flags & FABGPU_FLAG_PAIR_BOOTH4);
    ctx->pair_table_add = cfg && (cfg->flags & FABGPU_FLAG_PAIR_TABLE_ADD);
    // The LDS form of the pair kernel asks for 157 KiB of dynamic LDS per workgroup (130 KiB of tables, p256_pair29.h PAIR_LDS_CELLS_PER_SIG,
    // and the helper waves' handoff, PAIR_HAND_WORDS; 130 KiB in the one-wave form): a device that grants less keeps the table in the
    // global workspace instead of failing every large launch.  (That allocation is also what keeps other kernels off the
    // launch's CUs - more than the 84 KiB the pass reserves for that purpose.)
    if (std::max<size_t>(prop.sharedMemPerBlock, prop.maxSharedMemoryPerMultiProcessor) < (ctx->pair_solo ? pair_table_lds_solo_bytes() : pair_table_lds_bytes()))
        ctx->pair_table_lds = 0;
    ctx->time_kernels = cfg && (cfg->flags & FABGPU_FLAG_TIME_KERNELS);
    DeviceGuard g(dev);
    int rc = FABGPU_OK;
    do {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { rc = FABGPU_ENODEV; break; }
        if (hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess) { rc = FABGPU_ENODEV; break; }
        if (hipEventCreateWithFlags(&ctx->ev_up, hipEventDisableTiming) != hipSuccess) { rc = FABGPU_ENODEV; break; }
        if (hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking) != hipSuccess) { rc = FABGPU_ENODEV; break; }
        if (hipStreamCreateWithFlags(&ctx->stream4, hipStreamNonBlocking) != hipSuccess) { rc = FABGPU_ENODEV; break; }
        if (hipStreamCreateWithFlags(&ctx->stream_copy, hipStreamNonBlocking) != hipSuccess) { rc = FABGPU_ENODEV; break; }
        {
            bool ok = true;
            for (auto& sc : ctx->stream_copy_more) ok = ok && hipStreamCreateWithFlags(&sc, hipStreamNonBlocking) == hipSuccess;
            if (!ok) { rc = FABGPU_ENODEV; break; }
        }
        {
            bool ok = true;
            for (auto& e : ctx->ev_w) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
            if (!ok) { rc = FABGPU_ENODEV; break; }
        }
        if (const char* fi = getenv("FABGPU_FAULT_INJECT")) ctx->fault = !strcmp(fi, "launch") ? 1 : (!strcmp(fi, "oom") ? 2 : 0);
        if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) { rc = FABGPU_ENODEV; break; }
        if (hipMalloc((void**)&ctx->d_gtab, sizeof(int32_t) * GTab16::TABLE_WORDS) != hipSuccess) { rc = FABGPU_ENOMEM; break; }
        // The generator's comb (80 MiB) is built on the device since round 6 (keytab_kernels.hip launch_gtab_build: one million lanes, a
        // few milliseconds) - byte-identical to p256_tables29.h's, which took 0.2 s on sixteen host threads plus the upload and which is
        // what a failed device build falls back to.  FABGPU_GTAB_HOST=1 (tests, A/B) takes the host builder.
        bool built = false;
        if (!getenv("FABGPU_GTAB_HOST") && ctx->fault == 0) {
            void* scr = nullptr;
            if (hipMalloc(&scr, gtab_scratch_bytes()) == hipSuccess) {
                built = launch_gtab_build(ctx->d_gtab, scr, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
                hipFree(scr);
            }
            if (!built) (void)hipGetLastError();
        }
        if (!built) {
            std::vector<int32_t> tab(GTab16::TABLE_WORDS);   // 80 MiB, ~0.2 s on 16 host threads
            build_g_comb_table16(tab.data());
            if (hipMemcpy(ctx->d_gtab, tab.data(), sizeof(int32_t) * GTab16::TABLE_WORDS, hipMemcpyHostToDevice) != hipSuccess) { rc = FABGPU_ELAUNCH; break; }
        }
        if (ctx->key_tables_16) {
            // FABGPU_FLAG_KEY_TABLES_16BIT: the first slab of 16-bit key tables (8 x 80 MiB), the builders' rooms and their stream now, so that a
            // registration only queues launches (best effort: without them the keys are served by their 8-bit combs)
            void* slab = nullptr;
            if (hipMalloc(&slab, sizeof(int32_t) * GTab16::TABLE_WORDS * fabgpu_ctx::KTAB16_SLAB) == hipSuccess) ctx->ktab16_slabs.push_back(slab);
            else (void)hipGetLastError();
            ctx->ktab16_room_bytes = (keytab16_scratch_bytes() + 128 + 255) & ~(size_t)255;
            if (hipMalloc(&ctx->ktab16_rooms, ctx->ktab16_room_bytes * fabgpu_ctx::KTAB16_MAX) != hipSuccess) {
                (void)hipGetLastError();
                ctx->ktab16_rooms = nullptr;
            }
            if (hipStreamCreateWithFlags(&ctx->stream_keytab16, hipStreamNonBlocking) != hipSuccess) {
                (void)hipGetLastError();
                ctx->stream_keytab16 = nullptr;
            }
        }
        if (cfg && (cfg->flags & FABGPU_FLAG_P384_WIDE) && (rc = fab::ctx_set_p384_wide(ctx, true))) break;
        if (cfg && (cfg->flags & FABGPU_FLAG_SHA3_COOP) && (rc = fab::ctx_set_sha3_coop(ctx, true))) break;
        ctx->p384_tab16 = cfg && (cfg->flags & FABGPU_FLAG_P384_KEY_TABLES_16BIT);      // (nothing is allocated before the first registered P-384 key)
        if (cfg && cfg->max_batch) {
            size_t n = cfg->max_batch;
            if ((rc = ctx->fields.ensure(n * 160)) || (rc = ctx->offs.ensure((n + 1) * 4)) || (rc = ctx->out.ensure(n * 41 + 64))) break;
        }
        if (cfg && cfg->max_arena) {
            if ((rc = ctx->arena.ensure((size_t)cfg->max_arena + 128))) break;
        }
    } while (0);
    if (rc != FABGPU_OK) {
        fabgpu_shutdown(ctx);
        return rc;
    }
    *out = ctx;
    return FABGPU_OK;
}

void fabgpu_shutdown(fabgpu_ctx* ctx) {
    if (!ctx) return;
    ctx->stage_pool.reset();
    {
        DeviceGuard g(ctx->device);
        if (ctx->stream) hipStreamSynchronize(ctx->stream);
        ctx->fields.release();
        ctx->arena.release();
        ctx->offs.release();
        ctx->out.release();
        if (ctx->d_gtab) hipFree(ctx->d_gtab);
        if (ctx->d_gtab384) hipFree(ctx->d_gtab384);
        for (auto* t : ctx->ktab_slabs) hipFree(t);              // (every key table lies in a slab)
        for (auto* t : ctx->retired) hipFree(t);
        if (ctx->d_ktab_in) hipFree(ctx->d_ktab_in);
        if (ctx->d_ktab_scr) hipFree(ctx->d_ktab_scr);
        if (ctx->stream_keytab) hipStreamDestroy(ctx->stream_keytab);
        if (ctx->stream_kslot) hipStreamDestroy(ctx->stream_kslot);
        if (ctx->stream_k384) { hipStreamSynchronize(ctx->stream_k384); hipStreamDestroy(ctx->stream_k384); }
        if (ctx->stream_k384x16) { hipStreamSynchronize(ctx->stream_k384x16); hipStreamDestroy(ctx->stream_k384x16); }
        for (auto& q : ctx->k384_pending16) hipEventDestroy(q.ev);
        if (ctx->d_sha3_coop_rows) hipFree(ctx->d_sha3_coop_rows);
        for (void* t : ctx->k384_allocs) hipFree(t);                 // (P-384 key tables, the generator's comb, snapshot arrays)
        if (ctx->d_k384_in) hipFree(ctx->d_k384_in);
        if (ctx->d_k384_scr) hipFree(ctx->d_k384_scr);
        for (auto& d : ctx->k384_drains)
            for (hipEvent_t e : d.evs) hipEventDestroy(e);
        ctx->fence384.destroy_all();
        for (auto* t : ctx->itabs) hipFree(t);
        if (ctx->d_issuers) hipFree(ctx->d_issuers);
        ctx->nym.release();
        ctx->nymout.release();
        if (ctx->stream2) hipStreamDestroy(ctx->stream2);
        if (ctx->ev_up) hipEventDestroy(ctx->ev_up);
        if (ctx->stream3) hipStreamDestroy(ctx->stream3);
        if (ctx->stream4) hipStreamDestroy(ctx->stream4);
        if (ctx->stream_copy) hipStreamDestroy(ctx->stream_copy);
        for (auto sc : ctx->stream_copy_more)
            if (sc) hipStreamDestroy(sc);
        ctx->stage_pin.release();
        for (auto& k : ctx->keep_pool) k->pin.release();
        ctx->keep_pool.clear();
        for (auto& e : ctx->ev_w)
            if (e) hipEventDestroy(e);
        ctx->gath.release();
        ctx->tailbuf.release();
        ctx->keyed.release();
        ctx->pre.release();
        ctx->gscr.release();
        ctx->walk_env.release();
        ctx->walk_tup.release();
        ctx->walk_pin.release();
        ctx->walk_map.release();
        ctx->idtab_buf.release();
        for (auto& sl : ctx->staged_slots)
            if (sl.d) hipFree(sl.d);
        if (ctx->stream_keytab16) { hipStreamSynchronize(ctx->stream_keytab16); hipStreamDestroy(ctx->stream_keytab16); }       // (16-bit key tables may still be building)
        if (ctx->d_ktabs) hipFree((void*)ctx->d_ktabs);
        for (auto& d : ctx->kdrains)
            for (hipEvent_t e : d.evs) hipEventDestroy(e);
        for (auto& p : ctx->k16_pending) hipEventDestroy(p.built);
        ctx->fence256.destroy_all();
        for (void* t : ctx->ktab16_slabs)
            if (t) hipFree(t);
        if (ctx->ktab16_rooms) hipFree(ctx->ktab16_rooms);
        if (ctx->ktab16_heads) hipHostFree(ctx->ktab16_heads);
        for (auto& w : ctx->qws) {
            if (w.p) hipFree(w.p);
            if (w.done) hipEventDestroy(w.done);
            if (w.nym_side.stream) { hipStreamSynchronize(w.nym_side.stream); hipStreamDestroy(w.nym_side.stream); }
            if (w.nym_side.fork) hipEventDestroy(w.nym_side.fork);
            if (w.nym_side.join) hipEventDestroy(w.nym_side.join);
        }
        if (ctx->ev0) hipEventDestroy(ctx->ev0);
        if (ctx->ev1) hipEventDestroy(ctx->ev1);
        if (ctx->stream) hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

}  // extern "C"
// The eight-lane form of the keyed P-384 launches, on or off, for the launches queued after the call (block_walk_dev.h).  On: the
// scratch between its two launches joins the workspace pool now, so that no launch has to make it.
int fab::ctx_set_p384_wide(fabgpu_ctx* ctx, bool on) {
    if (!ctx) return FABGPU_EINVAL;
    if (on && !ctx->p384_wide.load(std::memory_order_relaxed)) {
        DeviceGuard g(ctx->device);
        size_t wi = 0;
        void* wsp = nullptr;
        if (int rc = ctx->acquire_qws(P384_WIDE_WS_BYTES, &wi, &wsp, ctx->stream)) return rc;
        ctx->release_qws(wi, ctx->stream);
    }
    ctx->p384_wide.store(on, std::memory_order_relaxed);
    return FABGPU_OK;
}
bool fab::ctx_p384_wide_serves(fabgpu_ctx* ctx, size_t n) {
    return ctx && n != 0 && n <= (size_t)P384_WIDE_LAUNCH_MAX && ctx->p384_wide.load(std::memory_order_relaxed);
}
// The 32-lanes-per-message SHA3-256 roads, on or off, for the launches queued after the call (block_walk_dev.h).  On for the first
// time: the device-side row counter of the mixed kernel is made and zeroed.
int fab::ctx_set_sha3_coop(fabgpu_ctx* ctx, bool on) {
    if (!ctx) return FABGPU_EINVAL;
    if (on && !ctx->d_sha3_coop_rows) {
        if (ctx->fault == 2) return FABGPU_ENOMEM;
        DeviceGuard g(ctx->device);
        void* ctr = nullptr;
        if (hipMalloc(&ctr, 16) != hipSuccess) {
            (void)hipGetLastError();
            return FABGPU_ENOMEM;
        }
        if (hipMemset(ctr, 0, 16) != hipSuccess) {
            (void)hipGetLastError();
            hipFree(ctr);
            return FABGPU_ELAUNCH;
        }
        ctx->d_sha3_coop_rows = (unsigned long long*)ctr;
    }
    ctx->sha3_coop.store(on, std::memory_order_relaxed);
    return FABGPU_OK;
}
int fab::sha3_coop_batch_uncapped(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, void* digests, void* stream) {
    if (!ctx || (n && (!arena || !off || !digests))) return FABGPU_EINVAL;
    if (n > 0xFFFFFFF0ull || arena_bytes > 0xFFFFFFFFull) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    ShaPrefixArgs pa;
    pa.digests = digests;
    return hip_to_rc(launch_sha3_256_messages_coop((uint32_t)n, arena, arena_bytes, off, pa, (hipStream_t)stream));
}
void fab::ctx_test_nym_side_after(fabgpu_ctx* ctx, bool on) {
    if (ctx) ctx->test_nym_side_after.store(on);
}
// TEST HOOK support: the capacities of the block pass's buffers - per-envelope, per-tuple, pinned, mapped, gather scratch
void fab::walk_buffer_caps(fabgpu_ctx* ctx, uint64_t out[5]) {
    for (int k = 0; k < 5; k++) out[k] = 0;
    if (!ctx) return;
    std::lock_guard<std::mutex> lk(ctx->mu);
    out[0] = ctx->walk_env.cap; out[1] = ctx->walk_tup.cap; out[2] = ctx->walk_pin.cap; out[3] = ctx->walk_map.cap; out[4] = ctx->gscr.cap;
}
// what the test-hook library's fabgpu_last_kernel_ms reads (FABGPU_FLAG_TIME_KERNELS contexts; block_walk_dev.h)
float fab::ctx_last_kernel_ms(fabgpu_ctx* ctx) {
    if (!ctx || !ctx->timed) return -1.0f;
    DeviceGuard g(ctx->device);
    if (hipEventSynchronize(ctx->ev1) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) != hipSuccess) return -1.0f;
    return ms;
}
extern "C" {

// ---- device-resident entry points ----------------------------------------------------------------
int fabgpu_p256_verify_batch_dev(fabgpu_ctx* ctx, size_t n, const void* qx, const void* qy, const void* e, const void* r,
                                 const void* s, void* verdict_bits, void* status, void* stream) {
    if (!ctx || (n && (!qx || !qy || !e || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (dev_too_big(n)) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    VerifyLaunch v = verify_launch_common(ctx, n, r, s, verdict_bits, status);
    v.qx = qx; v.qy = qy;
    v.e = e;
    v.table_lds = ctx->pair_table_lds; v.pair_solo = ctx->pair_solo; v.pair_dbl1 = ctx->pair_dbl1; v.pair_booth4 = ctx->pair_booth4; v.pair_table_add = ctx->pair_table_add;   // (the verify-only fresh-key form alone has the two table homes)
    return timed_launch(ctx, st, verify_workspace_bytes((uint32_t)n, ctx->allow_pair), [&](void* wsp) {
        v.qws = wsp;
        return launch_verify(v, st);
    });
}

int fabgpu_sha256_batch_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, void* digests,
                            void* stream) {
    if (!ctx || (n && (!arena || !off || !digests))) return FABGPU_EINVAL;
    if (dev_too_big(n, arena_bytes)) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    return timed_launch(ctx, st, 0, [&](void*) { return launch_sha256_batch((uint32_t)n, arena, arena_bytes, off, digests, st); });
}

int fabgpu_sha256_p256_verify_batch_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off,
                                        const void* qx, const void* qy, const void* r, const void* s, void* verdict_bits,
                                        void* status, void* stream) {
    if (!ctx || (n && (!arena || !off || !qx || !qy || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (dev_too_big(n, arena_bytes)) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    VerifyLaunch v = verify_launch_common(ctx, n, r, s, verdict_bits, status);
    v.qx = qx; v.qy = qy;
    v.arena = arena; v.arena_bytes = arena_bytes; v.off = off;
    return timed_launch(ctx, st, verify_workspace_bytes((uint32_t)n, ctx->allow_pair), [&](void* wsp) {
        v.qws = wsp;
        return launch_verify(v, st);
    });
}

// ---- idemix pseudonym signatures --------------------------------------------------------------------
int fabgpu_bn256_g1_on_curve(const uint8_t* x32, const uint8_t* y32) {
    if (!x32 || !y32) return 0;
    const u256 P = FAB_BN_P;
    u256 x, y;
    from_be32(x, x32);
    from_be32(y, y32);
    if (!lt256(x, P) || !lt256(y, P)) return 0;
    fbn fx, fy;
    fe_to_mont(fx, x);
    fe_to_mont(fy, y);
    return bn_on_curve29(fx, fy) ? 1 : 0;
}

int fabgpu_idemix_issuer_register(fabgpu_ctx* ctx, const uint8_t* hsk_x32, const uint8_t* hsk_y32, const uint8_t* hrand_x32,
                                  const uint8_t* hrand_y32, const uint8_t* ipk_hash32, uint32_t* issuer_id) {
    if (!ctx || !hsk_x32 || !hsk_y32 || !hrand_x32 || !hrand_y32 || !ipk_hash32 || !issuer_id) return FABGPU_EINVAL;
    if (!fabgpu_bn256_g1_on_curve(hsk_x32, hsk_y32) || !fabgpu_bn256_g1_on_curve(hrand_x32, hrand_y32)) return FABGPU_EINVAL;
    std::string k((const char*)hsk_x32, 32);
    k.append((const char*)hsk_y32, 32);
    k.append((const char*)hrand_x32, 32);
    k.append((const char*)hrand_y32, 32);
    k.append((const char*)ipk_hash32, 32);
    std::lock_guard<std::mutex> lk(ctx->imu);
    auto it = ctx->issuer_ids.find(k);
    if (it != ctx->issuer_ids.end()) {
        *issuer_id = it->second;
        return FABGPU_OK;
    }
    const size_t cur = ctx->itabs.size() / 2;
    if (cur >= FABGPU_MAX_ISSUERS) return FABGPU_ENOMEM;
    DeviceGuard g(ctx->device);
    const size_t slot = idemix_issuer_dev_bytes();
    if (!ctx->d_issuers && hipMalloc(&ctx->d_issuers, slot * FABGPU_MAX_ISSUERS) != hipSuccess) {
        ctx->d_issuers = nullptr;
        return FABGPU_ENOMEM;
    }
    const size_t tb = sizeof(int32_t) * KeyTab8::TABLE_WORDS;
    std::vector<int32_t> tab(KeyTab8::TABLE_WORDS);
    int32_t* d[2] = {nullptr, nullptr};
    const uint8_t* bx[2] = {hsk_x32, hrand_x32};
    const uint8_t* by[2] = {hsk_y32, hrand_y32};
    for (int b = 0; b < 2; b++) {
        u256 x, y;
        from_be32(x, bx[b]);
        from_be32(y, by[b]);
        build_bn_comb_table<8>(tab.data(), x, y);
        if (hipMalloc((void**)&d[b], tb) != hipSuccess || hipMemcpy(d[b], tab.data(), tb, hipMemcpyHostToDevice) != hipSuccess) {
            if (d[0]) hipFree(d[0]);
            if (d[1]) hipFree(d[1]);
            return FABGPU_ENOMEM;
        }
    }
    std::vector<uint8_t> hs(slot);
    idemix_issuer_dev_fill(hs.data(), d[0], d[1], ipk_hash32);
    if (hipMemcpy((uint8_t*)ctx->d_issuers + cur * slot, hs.data(), slot, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(d[0]);
        hipFree(d[1]);
        return FABGPU_ELAUNCH;
    }
    ctx->itabs.push_back(d[0]);
    ctx->itabs.push_back(d[1]);
    *issuer_id = (uint32_t)cur;
    ctx->issuer_ids[k] = *issuer_id;
    return FABGPU_OK;
}

int fabgpu_idemix_issuer_count(fabgpu_ctx* ctx) {
    if (!ctx) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->imu);
    return (int)(ctx->itabs.size() / 2);
}

// spans: off holds n (start, end) pairs instead of n + 1 running offsets; timed: this launch is what fabgpu_last_kernel_ms reports
static int nym_verify_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, bool spans, const void* issuer_id,
                          const void* nym_x, const void* nym_y, const void* proof_c, const void* proof_s_sk, const void* proof_s_r_nym,
                          const void* nonce, void* verdict_bits, void* status, void* stream, bool timed, const void* gather = nullptr, uint32_t lds_reserve = 0) {
    if (!ctx || (n && (!arena || !off || !nym_x || !nym_y || !proof_c || !proof_s_sk || !proof_s_r_nym || !nonce || !verdict_bits)))
        return FABGPU_EINVAL;
    if (n > 0xFFFFFFF0ull || arena_bytes > 0xFFFFFFFFull) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    uint32_t n_issuers;
    const void* issuers;
    {
        std::lock_guard<std::mutex> lk(ctx->imu);
        n_issuers = (uint32_t)(ctx->itabs.size() / 2);
        issuers = ctx->d_issuers;
    }
    if (n_issuers == 0) return FABGPU_EINVAL;   // nothing registered: every tuple would need bccsp/sw
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    size_t wi = 0;
    void* wsp = nullptr;
    int rc = ctx->acquire_qws(idemix_workspace_bytes((uint32_t)n, ctx->allow_pair, ctx->allow_quad), &wi, &wsp, st);
    if (rc != FABGPU_OK) return rc;
    // the side stream of this workspace slot (the slot is ours until release_qws: nobody else touches its entry)
    NymSide side;
    if (ctx->nym_two_phase && ctx->nym_side_stream && n <= (size_t)NYM_SIDE_STREAM_MAX) {
        std::lock_guard<std::mutex> lk(ctx->qmu);
        NymSide& sd = ctx->qws[wi].nym_side;
        if (!sd.stream) {
            NymSide made;
            if (hipStreamCreateWithFlags(&made.stream, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&made.fork, hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&made.join, hipEventDisableTiming) == hipSuccess)
                sd = made;
            else {
                if (made.fork) hipEventDestroy(made.fork);
                if (made.stream) hipStreamDestroy(made.stream);
            }
        }
        side = sd;
        side.test_side_after = ctx->test_nym_side_after;
    }
    timed = timed && ctx->time_kernels;
    if (timed) hipEventRecord(ctx->ev0, st);
    hipError_t err = launch_idemix_nym_verify((uint32_t)n, arena, arena_bytes, off, issuer_id, issuers, n_issuers, nym_x, nym_y, proof_c,
                                              proof_s_sk, proof_s_r_nym, nonce, wsp, verdict_bits, status, ctx->allow_pair, ctx->allow_quad, spans, st, gather, lds_reserve,
                                              ctx->nym_two_phase, side.stream ? &side : nullptr);
    if (timed) hipEventRecord(ctx->ev1, st);
    ctx->release_qws(wi, st);
    if (timed) ctx->timed = true;
    return hip_to_rc(launched(ctx, err));
}

int fabgpu_idemix_nym_verify_batch_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off,
                                       const void* issuer_id, const void* nym_x, const void* nym_y, const void* proof_c,
                                       const void* proof_s_sk, const void* proof_s_r_nym, const void* nonce, void* verdict_bits,
                                       void* status, void* stream) {
    return nym_verify_dev(ctx, n, arena, arena_bytes, off, false, issuer_id, nym_x, nym_y, proof_c, proof_s_sk, proof_s_r_nym, nonce, verdict_bits,
                          status, stream, true);
}

// ---- registered public keys -------------------------------------------------------------------------
// one key's comb table into one context: id of the key there (idempotent per (qx, qy)); `tab` = the table, built by the caller
static int key_install_table_locked(fabgpu_ctx* ctx, const std::string& k, int32_t* d, uint32_t* key_id);
static void key_queue_table16_locked(fabgpu_ctx* ctx, const std::string& k, uint32_t id);

// ---- retiring keys: the two waits between a retirement and the reuse of its slot and tables (fabgpu_ctx::kslots has the story) ----
// (kmu held, the context's device current) a few bytes of the host's into d_ktabs, complete on return.  Not with hipMemcpy: that one
// runs on the null stream and waits for every blocking stream of the process.
static bool kslot_write_locked(fabgpu_ctx* ctx, size_t word, const void* src, size_t bytes) {
    if (!ctx->stream_kslot && hipStreamCreateWithFlags(&ctx->stream_kslot, hipStreamNonBlocking) != hipSuccess) return false;
    hipError_t e = hipMemcpyAsync((void*)(ctx->d_ktabs + word), src, bytes, hipMemcpyHostToDevice, ctx->stream_kslot);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream_kslot);      // (a stream of its own: the copy is all that is ever queued there)
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess;
}
// The streams of the context's own that carry keyed launches of either curve (the block pass runs on all four): one of them that
// refuses an event is waited for, never forgotten (keyed_fence.h, rule 3).  What record() answers is not asked for: where the
// stream could not be waited for either, the device has failed and runs nothing more.
struct KeyedStreamOwned {
    const fabgpu_ctx* ctx;
    bool operator()(hipStream_t s) const { return s == ctx->stream || s == ctx->stream2 || s == ctx->stream3 || s == ctx->stream4; }
};
// One retired slot as far as it goes without waiting for a launch or a launcher (wait: all the way).  true: drained - tables on the
// free lists, slot reclaimable.  kmu is held, so no new snapshot is taken while the generation word is written and the second set of
// events recorded: whoever took a snapshot earlier has enqueued (the events cover it), whoever takes one later finds KTAB_GEN_NONE.
static bool kdrain_step_locked(fabgpu_ctx* ctx, fabgpu_ctx::KeyDrain& d, bool wait) {
    if (d.phase == 1) {
        if (!ctx->fence256.done(d.evs, wait) || !ctx->fence256.quiet(wait)) return false;
        const uint64_t none = KTAB_GEN_NONE;
        if (!kslot_write_locked(ctx, KTAB_STRIDE * (size_t)d.slot + 2, &none, sizeof(none))) return false;   // (stays in phase 1: tried again)
        ctx->kgen_dev[d.slot] = KTAB_GEN_NONE;
        (void)ctx->fence256.record(d.evs, KeyedStreamOwned{ctx});
        d.phase = 2;
    }
    if (!ctx->fence256.done(d.evs, wait)) return false;
    if (d.t8) ctx->ktab_free.push_back(d.t8);
    if (d.t16) ctx->ktab16_free.push_back(d.t16);
    if (d.idx16 >= 0) ctx->ktab16_idx_free.push_back(d.idx16);
    ctx->kslots.drained(d.slot);                    // (a parked slot stays parked)
    return true;
}
static void kdrain_advance_locked(fabgpu_ctx* ctx) {
    HipKeyedFence::advance(ctx->kdrains, [ctx](fabgpu_ctx::KeyDrain& d, bool wait) { return kdrain_step_locked(ctx, d, wait); });
}
static bool kdrain_wait_slot_locked(fabgpu_ctx* ctx, uint32_t slot) {
    return HipKeyedFence::wait_for(ctx->kdrains, [slot](const fabgpu_ctx::KeyDrain& d) { return d.slot == slot; },
                                   [ctx](fabgpu_ctx::KeyDrain& d, bool wait) { return kdrain_step_locked(ctx, d, wait); }) &&
           !ctx->kslots.draining(slot);
}
// 16-bit combs of reused slots whose build has finished: the host writes their pointers
static void k16_publish_locked(fabgpu_ctx* ctx) {
    for (size_t i = 0; i < ctx->k16_pending.size();) {
        auto& p = ctx->k16_pending[i];
        hipError_t e = hipEventQuery(p.built);
        if (e == hipErrorNotReady) {
            (void)hipGetLastError();
            i++;
            continue;
        }
        if (e == hipSuccess && ctx->ktab16[p.slot] == p.tab) {
            DeviceGuard g(ctx->device);
            (void)kslot_write_locked(ctx, KTAB_STRIDE * (size_t)p.slot + 1, &p.tab, sizeof(void*));     // (not written: served by the 8-bit comb)
        }
        ctx->fence256.put(p.built);
        ctx->k16_pending.erase(ctx->k16_pending.begin() + (long)i);
    }
}
// What a keyed launch site needs of the key table, taken under kmu, and the launcher's ticket of fence256, held until its last keyed
// launch is queued (the destructor).  Nothing between the constructor and the destructor may take kmu.
static_assert(KEY_SLOT_BITS == (int)fab::KeySlots::SLOT_BITS && FABGPU_MAX_KEYS == (1 << KEY_SLOT_BITS) && fab::KeySlots::MAX_SLOTS == FABGPU_MAX_KEYS,
              "the kernels' slot bits (kernels.h), the allocator's (key_slots.h) and the public cap on live keys (fabgpu.h) are one number");
static_assert(KTAB_GEN_NONE > fab::KeySlots::GEN_LAST, "no id may carry the generation word of a slot between two tenants");
struct KeyedSnap {
    uint32_t nkeys = 0;
    const int32_t** kt = nullptr;
    HipKeyedFence::Ticket ticket;
    KeyedSnap(fabgpu_ctx* ctx, std::initializer_list<hipStream_t> streams) {
        std::lock_guard<std::mutex> lk(ctx->kmu);
        nkeys = ctx->kslots.high_water();
        kt = ctx->d_ktabs;
        ticket = ctx->fence256.enter(streams);
    }
};
// (kmu held, the context's device current) room for one table: out of the current slab, a new slab when that is used up
static int32_t* ktab_alloc_locked(fabgpu_ctx* ctx) {
    if (!ctx->ktab_free.empty()) {
        int32_t* d = ctx->ktab_free.back();
        ctx->ktab_free.pop_back();
        return d;
    }
    constexpr size_t table_bytes = sizeof(int32_t) * KeyTab8::TABLE_WORDS;
    if (ctx->ktab_slab_used >= fabgpu_ctx::KTAB_SLAB) {
        if (ctx->fault == 2) return nullptr;
        void* slab = nullptr;
        if (hipMalloc(&slab, table_bytes * fabgpu_ctx::KTAB_SLAB) != hipSuccess) return nullptr;
        ctx->ktab_slabs.push_back(slab);
        ctx->ktab_slab_used = 0;
    }
    return (int32_t*)((uint8_t*)ctx->ktab_slabs.back() + table_bytes * ctx->ktab_slab_used++);
}
static int key_install(fabgpu_ctx* ctx, const std::string& k, const std::vector<int32_t>* tab_in, const uint8_t* qx32, const uint8_t* qy32, uint32_t* key_id) {
    std::lock_guard<std::mutex> lk(ctx->kmu);
    auto it = ctx->key_ids.find(k);
    if (it != ctx->key_ids.end()) {
        *key_id = it->second;
        return FABGPU_OK;
    }
    if (ctx->kslots.next_slot() < 0) return FABGPU_ENOMEM;
    DeviceGuard g(ctx->device);
    kdrain_advance_locked(ctx);
    std::vector<int32_t> own;
    if (!tab_in) {
        u256 qx, qy;
        from_be32(qx, qx32);
        from_be32(qy, qy32);
        own.resize(KeyTab8::TABLE_WORDS);
        build_key_comb_table8(own.data(), qx, qy);
        tab_in = &own;
    }
    const std::vector<int32_t>& tab = *tab_in;
    int32_t* d = ktab_alloc_locked(ctx);
    if (!d) return FABGPU_ENOMEM;
    if (hipMemcpy(d, tab.data(), sizeof(int32_t) * KeyTab8::TABLE_WORDS, hipMemcpyHostToDevice) != hipSuccess) {
        ctx->ktab_free.push_back(d);
        return FABGPU_ELAUNCH;
    }
    return key_install_table_locked(ctx, k, d, key_id);
}
// (kmu held, the context's device current) a finished table in device memory becomes key number ktabs.size(); takes ownership of d
// FABGPU_FLAG_KEY_TABLES_16BIT: queue the build of key `id`'s 16-bit comb on stream_keytab and, behind it, the copy of its pointer into
// d_ktabs[2 id + 1].  Nothing waits: the registration returns, launches on other streams use the 8-bit comb until the pointer is there.
// kmu is held.  Failures (memory, a launch) leave the key without a 16-bit comb.
static void key_queue_table16_locked(fabgpu_ctx* ctx, const std::string& k, uint32_t id) {
    const uint32_t slot = fab::KeySlots::slot_of(id);
    const bool first_tenant = fab::KeySlots::gen_of(id) == 0;
    if (ctx->ktab16_count >= fabgpu_ctx::KTAB16_MAX || ctx->fault) return;
    if (ctx->ktab16_idx_free.empty() && ctx->ktab16_idx_next >= fabgpu_ctx::KTAB16_MAX) return;      // (every room is live or draining)
    if (ctx->ktab16.size() <= slot) ctx->ktab16.resize((size_t)slot + 1, nullptr);
    if (ctx->ktab16_idx.size() <= slot) ctx->ktab16_idx.resize((size_t)slot + 1, -1);
    if (!ctx->stream_keytab16 && hipStreamCreateWithFlags(&ctx->stream_keytab16, hipStreamNonBlocking) != hipSuccess) return;
    const size_t tab_bytes = sizeof(int32_t) * GTab16::TABLE_WORDS;
    if (!ctx->ktab16_rooms) {
        ctx->ktab16_room_bytes = (keytab16_scratch_bytes() + 128 + 255) & ~(size_t)255;
        if (hipMalloc(&ctx->ktab16_rooms, ctx->ktab16_room_bytes * fabgpu_ctx::KTAB16_MAX) != hipSuccess) {
            (void)hipGetLastError();
            ctx->ktab16_rooms = nullptr;
            return;
        }
    }
    const bool tab_reused = !ctx->ktab16_free.empty();
    if (!tab_reused && ctx->ktab16_carved == ctx->ktab16_slabs.size() * fabgpu_ctx::KTAB16_SLAB) {
        void* slab = nullptr;
        if (hipMalloc(&slab, tab_bytes * fabgpu_ctx::KTAB16_SLAB) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        ctx->ktab16_slabs.push_back(slab);
    }
    void* tab = tab_reused ? ctx->ktab16_free.back() : (uint8_t*)ctx->ktab16_slabs.back() + tab_bytes * (ctx->ktab16_carved % fabgpu_ctx::KTAB16_SLAB);
    const bool idx_reused = !ctx->ktab16_idx_free.empty();
    const size_t idx = idx_reused ? (size_t)ctx->ktab16_idx_free.back() : ctx->ktab16_idx_next;
    void* room = (uint8_t*)ctx->ktab16_rooms + ctx->ktab16_room_bytes * idx;
    hipStream_t st = ctx->stream_keytab16;
    // room: [0, 64) the key, [64, 72) the table's address (what the entries kernel reads), [128, ...) scratch
    if (!ctx->ktab16_heads && hipHostMalloc((void**)&ctx->ktab16_heads, 128 * fabgpu_ctx::KTAB16_MAX, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        ctx->ktab16_heads = nullptr;
        return;
    }
    uint8_t* head = ctx->ktab16_heads + 128 * idx;
    memcpy(head, k.data(), 64);
    memcpy(head + 64, &tab, sizeof(void*));
    hipEvent_t built = first_tenant ? nullptr : ctx->fence256.get();
    if (!first_tenant && !built) return;
    hipError_t e = hipMemcpyAsync(room, head, 72, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_keytab16_build(1, room, (void* const*)((uint8_t*)room + 64), (uint8_t*)room + 128, st);
    // a slot's first tenant: the pointer follows the build on the builder's stream, as ever.  A reused slot: the host writes it (k16_publish_locked)
    if (e == hipSuccess && first_tenant) e = hipMemcpyAsync((void*)(ctx->d_ktabs + KTAB_STRIDE * (size_t)slot + 1), (uint8_t*)room + 64, sizeof(void*), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && !first_tenant) e = hipEventRecord(built, st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        hipStreamSynchronize(st);                       // (the table and the room are simply used again by the next key)
        if (built) ctx->fence256.put(built);
        return;
    }
    if (built) ctx->k16_pending.push_back({slot, tab, built});
    ctx->ktab16[slot] = tab;
    ctx->ktab16_idx[slot] = (int)idx;
    if (tab_reused) ctx->ktab16_free.pop_back();
    else ctx->ktab16_carved++;
    if (idx_reused) ctx->ktab16_idx_free.pop_back();
    else ctx->ktab16_idx_next++;
    ctx->ktab16_count++;
}

static int key_install_table_locked(fabgpu_ctx* ctx, const std::string& k, int32_t* d, uint32_t* key_id) {
    kdrain_advance_locked(ctx);
    if (!ctx->k16_pending.empty()) k16_publish_locked(ctx);
    const int64_t next = ctx->kslots.next_slot();
    if (next < 0) {
        ctx->ktab_free.push_back(d);
        return FABGPU_ENOMEM;
    }
    const uint32_t slot = (uint32_t)next;
    if (slot < ctx->ktabs.size()) {
        // A retired key's slot, the lowest there is.  Still draining: wait for ITS events (key_slots.h: never another slot).  Then nothing
        // on the device can name the slot with a generation it shows (KTAB_GEN_NONE): the pointers first, the new generation last.
        if (!kdrain_wait_slot_locked(ctx, slot)) {
            ctx->ktab_free.push_back(d);
            return FABGPU_ELAUNCH;
        }
        const int32_t* ptrs[2] = {d, nullptr};
        const uint64_t gen = (uint64_t)ctx->kslots.generation(slot) + 1;
        if (!kslot_write_locked(ctx, KTAB_STRIDE * (size_t)slot, ptrs, sizeof(ptrs)) || !kslot_write_locked(ctx, KTAB_STRIDE * (size_t)slot + 2, &gen, sizeof(gen))) {
            ctx->ktab_free.push_back(d);
            return FABGPU_ELAUNCH;
        }
        ctx->ktabs[slot] = d;
        if (slot < ctx->ktab16.size()) ctx->ktab16[slot] = nullptr;
        if (slot < ctx->ktab16_idx.size()) ctx->ktab16_idx[slot] = -1;
        ctx->kgen_dev[slot] = (uint32_t)gen;
        ctx->kname[slot] = k;
        *key_id = ctx->kslots.take(slot);
        ctx->key_ids[k] = *key_id;
        if (ctx->key_tables_16) key_queue_table16_locked(ctx, k, *key_id);
        return FABGPU_OK;
    }
    // grow the device-side array by doubling; the old array is only released at shutdown, so launches already in
    // flight on other streams keep reading a valid (shorter) array
    if (ctx->ktabs.size() + 1 > ctx->d_ktabs_cap) {
        size_t cap = ctx->d_ktabs_cap ? ctx->d_ktabs_cap * 2 : 64;
        const int32_t** nd = nullptr;
        if (hipMalloc((void**)&nd, cap * KTAB_STRIDE * sizeof(int32_t*)) != hipSuccess) {
            ctx->ktab_free.push_back(d);
            return FABGPU_ENOMEM;
        }
        if (!ctx->ktabs.empty()) {
            // (the 16-bit builds queued on stream_keytab write their pointers into the OLD array: let them land before it is copied.
            //  A launcher that still holds the old array holds a ticket of fence256 like any other: a slot retired from now on waits
            //  for it, and an id handed out from now on is simply out of its range)
            if (ctx->stream_keytab16) hipStreamSynchronize(ctx->stream_keytab16);
            std::vector<const int32_t*> both(ctx->ktabs.size() * KTAB_STRIDE, nullptr);
            for (size_t i = 0; i < ctx->ktabs.size(); i++) {
                both[KTAB_STRIDE * i] = ctx->ktabs[i];
                both[KTAB_STRIDE * i + 1] = i < ctx->ktab16.size() ? (const int32_t*)ctx->ktab16[i] : nullptr;
                both[KTAB_STRIDE * i + 2] = (const int32_t*)(uintptr_t)ctx->kgen_dev[i];
            }
            hipMemcpy((void*)nd, both.data(), both.size() * sizeof(int32_t*), hipMemcpyHostToDevice);
        }
        if (ctx->d_ktabs) ctx->retired.push_back((void*)ctx->d_ktabs);
        ctx->d_ktabs = nd;
        ctx->d_ktabs_cap = cap;
    }
    const int32_t* slotw[KTAB_STRIDE] = {d, nullptr, nullptr, nullptr};      // (generation 0)
    if (hipMemcpy((void*)(ctx->d_ktabs + KTAB_STRIDE * ctx->ktabs.size()), slotw, sizeof(slotw), hipMemcpyHostToDevice) != hipSuccess) {
        ctx->ktab_free.push_back(d);
        return FABGPU_ELAUNCH;
    }
    ctx->ktabs.push_back(d);
    ctx->kgen_dev.push_back(0);
    ctx->kname.push_back(k);
    *key_id = ctx->kslots.take(slot);
    ctx->key_ids[k] = *key_id;
    if (ctx->key_tables_16) key_queue_table16_locked(ctx, k, *key_id);    // (best effort: a key without one is served by its 8-bit comb)
    return FABGPU_OK;
}

// n keys (qxy: n x 64 bytes, X || Y; every one an affine point of the curve - the caller's gate) registered on ONE context with their
// comb tables built ON THE DEVICE (keytab_kernels.hip: three launches for the whole batch, 0.7-0.9 ms, against 6 ms of host arithmetic
// per key).  key_ids[i] = the key's id (keys the context already has keep theirs); ids are handed out in the order of qxy.  Any failure:
// nothing was installed by this call that is not complete, the error is returned and the caller may fall back to the host builder.
static int key_register_batch_dev(fabgpu_ctx* ctx, int n, const uint8_t* qxy, uint32_t* key_ids) {
    if (!ctx || n <= 0 || !qxy || !key_ids) return FABGPU_EINVAL;
    if (ctx->fault) return ctx->fault == 2 ? FABGPU_ENOMEM : FABGPU_ELAUNCH;
    static const bool timing = getenv("FABGPU_PASS_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    std::lock_guard<std::mutex> blk(ctx->ktab_build_mu);        // one batch at a time per context: the builder's room and stream are one
    DeviceGuard g(ctx->device);
    std::vector<int> todo;                                     // indices into qxy that need a table (first occurrence of a key only)
    std::vector<std::string> names((size_t)n);
    std::vector<int32_t*> tabs;
    {
        std::lock_guard<std::mutex> lk(ctx->kmu);
        for (int i = 0; i < n; i++) {
            names[(size_t)i].assign((const char*)qxy + 64 * (size_t)i, 64);
            bool dup = false;
            for (int j : todo) dup = dup || names[(size_t)j] == names[(size_t)i];
            if (!dup && ctx->key_ids.find(names[(size_t)i]) == ctx->key_ids.end()) todo.push_back(i);
        }
        if (todo.size() > ctx->kslots.room()) return FABGPU_ENOMEM;
        kdrain_advance_locked(ctx);
        for (size_t t = 0; t < todo.size(); t++) {
            int32_t* d = ktab_alloc_locked(ctx);
            if (!d) {
                for (auto* x : tabs) ctx->ktab_free.push_back(x);
                return FABGPU_ENOMEM;
            }
            tabs.push_back(d);
        }
    }
    const uint32_t m = (uint32_t)todo.size();
    auto give_back = [&](int code) {
        std::lock_guard<std::mutex> lk(ctx->kmu);
        for (auto* x : tabs)
            if (x) ctx->ktab_free.push_back(x);
        return code;
    };
    double t_room = 0, t_build = 0;
    if (m) {
        // one small upload: the keys, then the table pointers; the builder's room grows with the largest batch so far
        const size_t in_bytes = (size_t)64 * m + sizeof(void*) * m, scr_bytes = keytab_scratch_bytes(m);
        if (ctx->ktab_in_cap < in_bytes) {
            if (ctx->d_ktab_in) hipFree(ctx->d_ktab_in);
            ctx->d_ktab_in = nullptr;
            ctx->ktab_in_cap = 0;
            if (hipMalloc(&ctx->d_ktab_in, in_bytes * 2) != hipSuccess) return give_back(FABGPU_ENOMEM);
            ctx->ktab_in_cap = in_bytes * 2;
        }
        if (ctx->ktab_scr_cap < scr_bytes) {
            if (ctx->d_ktab_scr) hipFree(ctx->d_ktab_scr);
            ctx->d_ktab_scr = nullptr;
            ctx->ktab_scr_cap = 0;
            if (hipMalloc(&ctx->d_ktab_scr, scr_bytes * 2) != hipSuccess) return give_back(FABGPU_ENOMEM);
            ctx->ktab_scr_cap = scr_bytes * 2;
        }
        if (!ctx->stream_keytab && hipStreamCreateWithFlags(&ctx->stream_keytab, hipStreamNonBlocking) != hipSuccess) return give_back(FABGPU_ELAUNCH);
        std::vector<uint8_t> in(in_bytes);
        for (uint32_t t = 0; t < m; t++) memcpy(&in[64 * (size_t)t], qxy + 64 * (size_t)todo[t], 64);
        memcpy(&in[(size_t)64 * m], tabs.data(), sizeof(void*) * m);
        t_room = since();
        hipStream_t st = ctx->stream_keytab;
        hipError_t e = hipMemcpyAsync(ctx->d_ktab_in, in.data(), in_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = launch_keytab_build(m, ctx->d_ktab_in, (void* const*)((uint8_t*)ctx->d_ktab_in + (size_t)64 * m), ctx->d_ktab_scr, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return give_back(hip_to_rc(e));
        t_build = since();
    }
    int rc = FABGPU_OK;
    {
        std::lock_guard<std::mutex> lk(ctx->kmu);
        for (uint32_t t = 0; t < m; t++) {
            const std::string& k = names[(size_t)todo[t]];
            uint32_t id = 0;
            if (rc == FABGPU_OK && ctx->key_ids.find(k) == ctx->key_ids.end()) rc = key_install_table_locked(ctx, k, tabs[t], &id);   // (takes the table, also on failure)
            else ctx->ktab_free.push_back(tabs[t]);             // (somebody registered it meanwhile, or an earlier install failed)
            tabs[t] = nullptr;
        }
        if (rc == FABGPU_OK)
            for (int i = 0; i < n; i++) {
                auto it = ctx->key_ids.find(names[(size_t)i]);
                if (it == ctx->key_ids.end()) {
                    rc = FABGPU_ELAUNCH;
                    break;
                }
                key_ids[i] = it->second;
            }
    }
    if (timing && m) fprintf(stderr, "fabgpu: %u key tables on the device: room %.2f ms, build %.2f ms, installed after %.2f ms\n", m, t_room, t_build - t_room, since());
    return rc;
}

int fabgpu_p256_key_register(fabgpu_ctx* ctx, const uint8_t* qx32, const uint8_t* qy32, uint32_t* key_id) {
    if (!ctx || !qx32 || !qy32 || !key_id) return FABGPU_EINVAL;
    if (!fabgpu_p256_pubkey_on_curve(qx32, qy32)) return FABGPU_EINVAL;   // KeyImport gate: such keys stay with bccsp/sw
    std::string k((const char*)qx32, 32);
    k.append((const char*)qy32, 32);
    // the table is built on the device; should that fail (memory, a launch), by the host builder as before round 6
    if (key_register_batch_dev(ctx, 1, (const uint8_t*)k.data(), key_id) == FABGPU_OK) return FABGPU_OK;
    return key_install(ctx, k, nullptr, qx32, qy32, key_id);
}

// The same key on n contexts (a provider that owns every GPU of the node): the 640 KiB comb table is built ONCE on the host (~6 ms)
// and uploaded to each context that does not have the key yet.  key_ids[g] = the key's id on ctxs[g].  The first failure is returned
// (contexts before it keep the key: registration is idempotent).
static int key_register_many_impl(fabgpu_ctx* const* ctxs, int n, const uint8_t* qx32, const uint8_t* qy32, const int32_t* prebuilt, uint32_t* key_ids) {
    if (!ctxs || n <= 0 || !qx32 || !qy32 || !key_ids) return FABGPU_EINVAL;
    for (int g = 0; g < n; g++)
        if (!ctxs[g]) return FABGPU_EINVAL;
    if (!fabgpu_p256_pubkey_on_curve(qx32, qy32)) return FABGPU_EINVAL;
    std::string k((const char*)qx32, 32);
    k.append((const char*)qy32, 32);
    std::vector<int32_t> tab;                              // built when the first context turns out to need it (unless the caller brought one)
    if (prebuilt) tab.assign(prebuilt, prebuilt + KeyTab8::TABLE_WORDS);
    for (int g = 0; g < n; g++) {
        bool have;
        {
            std::lock_guard<std::mutex> lk(ctxs[g]->kmu);
            auto it = ctxs[g]->key_ids.find(k);
            have = it != ctxs[g]->key_ids.end();
            if (have) key_ids[g] = it->second;
        }
        if (have) continue;
        if (tab.empty() && key_register_batch_dev(ctxs[g], 1, (const uint8_t*)k.data(), &key_ids[g]) == FABGPU_OK) continue;   // built on that device
        if (tab.empty()) {
            u256 qx, qy;
            from_be32(qx, qx32);
            from_be32(qy, qy32);
            tab.resize(KeyTab8::TABLE_WORDS);
            build_key_comb_table8(tab.data(), qx, qy);
        }
        const int rc = key_install(ctxs[g], k, &tab, qx32, qy32, &key_ids[g]);
        if (rc != FABGPU_OK) return rc;
    }
    return FABGPU_OK;
}
int fabgpu_p256_key_register_many(fabgpu_ctx* const* ctxs, int n, const uint8_t* qx32, const uint8_t* qy32, uint32_t* key_ids) {
    return key_register_many_impl(ctxs, n, qx32, qy32, nullptr, key_ids);
}

int fabgpu_p256_key_lookup(fabgpu_ctx* ctx, const uint8_t* qx32, const uint8_t* qy32, uint32_t* key_id) {
    if (!ctx || !qx32 || !qy32 || !key_id) return FABGPU_EINVAL;
    std::string k((const char*)qx32, 32);
    k.append((const char*)qy32, 32);
    std::lock_guard<std::mutex> lk(ctx->kmu);
    auto it = ctx->key_ids.find(k);
    if (it == ctx->key_ids.end()) return 1;
    *key_id = it->second;
    return FABGPU_OK;
}

int fabgpu_p256_key_count(fabgpu_ctx* ctx) {
    if (!ctx) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->kmu);
    return (int)ctx->kslots.n_live();
}

int fabgpu_p256_key_unregister(fabgpu_ctx* ctx, uint32_t key_id) {
    if (!ctx) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->kmu);
    if (!ctx->kslots.live(key_id)) return 1;
    const uint32_t slot = fab::KeySlots::slot_of(key_id);
    DeviceGuard g(ctx->device);
    if (!ctx->k16_pending.empty()) k16_publish_locked(ctx);
    ctx->key_ids.erase(ctx->kname[slot]);
    ctx->kslots.retire(key_id);
    // the device keeps showing the key: what is queued already answers for it.  The slot and its tables wait (fabgpu_ctx::kslots)
    fabgpu_ctx::KeyDrain d;
    d.slot = slot;
    d.t8 = ctx->ktabs[slot];
    d.t16 = slot < ctx->ktab16.size() ? ctx->ktab16[slot] : nullptr;
    d.idx16 = slot < ctx->ktab16_idx.size() ? ctx->ktab16_idx[slot] : -1;
    if (d.t16) {
        ctx->ktab16_count--;
        for (size_t i = 0; i < ctx->k16_pending.size(); i++)
            if (ctx->k16_pending[i].slot == slot) {      // (a build still queued: its pointer is never published; the builder's stream is among the events)
                d.evs.push_back(ctx->k16_pending[i].built);
                ctx->k16_pending.erase(ctx->k16_pending.begin() + (long)i);
                break;
            }
    }
    std::vector<hipStream_t> builder;                    // (phase 1 also waits for the 16-bit builder's stream, if the key had a table)
    if (d.t16 && ctx->stream_keytab16) builder.push_back(ctx->stream_keytab16);
    (void)ctx->fence256.record(d.evs, KeyedStreamOwned{ctx}, builder);
    ctx->kdrains.push_back(std::move(d));
    return FABGPU_OK;
}

int fabgpu_p256_key_unregister_many(fabgpu_ctx* const* ctxs, int n, const uint8_t* qx32, const uint8_t* qy32) {
    if (!ctxs || n <= 0 || !qx32 || !qy32) return FABGPU_EINVAL;
    for (int g = 0; g < n; g++)
        if (!ctxs[g]) return FABGPU_EINVAL;
    int had = 0;
    for (int g = 0; g < n; g++) {
        uint32_t id = 0;
        if (fabgpu_p256_key_lookup(ctxs[g], qx32, qy32, &id) == FABGPU_OK && fabgpu_p256_key_unregister(ctxs[g], id) == FABGPU_OK) had++;
    }
    return had == n ? FABGPU_OK : (had == 0 ? 1 : 2);
}

int fabgpu_p256_key_table_stats(fabgpu_ctx* ctx, uint64_t* out, int cap) {
    if (!ctx || (cap > 0 && !out)) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->kmu);
    if (!ctx->k16_pending.empty()) k16_publish_locked(ctx);
    uint64_t bytes = (uint64_t)ctx->ktab_slabs.size() * fabgpu_ctx::KTAB_SLAB * sizeof(int32_t) * KeyTab8::TABLE_WORDS +
                     (uint64_t)ctx->ktab16_slabs.size() * fabgpu_ctx::KTAB16_SLAB * sizeof(int32_t) * GTab16::TABLE_WORDS +
                     (ctx->ktab16_rooms ? (uint64_t)ctx->ktab16_room_bytes * fabgpu_ctx::KTAB16_MAX : 0) +
                     (uint64_t)ctx->d_ktabs_cap * KTAB_STRIDE * sizeof(void*);
    const uint64_t v[FABGPU_KEY_TABLE_STATS] = {ctx->kslots.n_live(), ctx->kslots.n_draining(), ctx->kslots.n_reused(), ctx->kslots.n_parked(),
                                                (uint64_t)ctx->ktab16_count, bytes, ctx->kslots.high_water()};
    for (int i = 0; i < cap && i < FABGPU_KEY_TABLE_STATS; i++) out[i] = v[i];
    return FABGPU_KEY_TABLE_STATS;
}

int fabgpu_p256_verify_batch_keyed_dev(fabgpu_ctx* ctx, size_t n, const void* key_id, const void* e, const void* r, const void* s,
                                       void* verdict_bits, void* status, void* stream) {
    if (!ctx || (n && (!key_id || !e || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (dev_too_big(n)) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    hipStream_t st = (hipStream_t)stream;
    KeyedSnap snap(ctx, {st});
    if (snap.nkeys == 0) return FABGPU_EINVAL;
    DeviceGuard g(ctx->device);
    if (ctx->allow_wide && n <= (size_t)WIDE_LAUNCH_MAX)
        // a launch that cannot fill the chip: eight lanes per signature, the digest-independent half first (kernels.h, p256_wide29.h)
        return timed_launch(ctx, st, n * WIDE_SCRATCH_BYTES, [&](void* wsp) {
            hipError_t err = launch_p256_wide_pre((uint32_t)n, key_id, snap.nkeys, (const void*)snap.kt, r, s, ctx->d_gtab, wsp, st);
            if (err == hipSuccess) err = launch_p256_wide_post((uint32_t)n, e, r, ctx->d_gtab, wsp, verdict_bits, status, st);
            return err;
        });
    VerifyLaunch v = verify_launch_common(ctx, n, r, s, verdict_bits, status);
    v.key_id = key_id; v.nkeys = snap.nkeys; v.ktabs = (const void*)snap.kt;
    v.e = e;
    return timed_launch(ctx, st, 0, [&](void*) { return launch_verify(v, st); });
}

// identity.Verify for registered keys on a launch that cannot fill the chip: the digest-independent half of the verification, the
// hashes (mid-states of shared prefixes first, unless the caller has them), then the half behind the digest.  One stream here - the
// block pass runs the first two side by side (walk_block_pass).  digests_out: the caller's n x 32 bytes, or nullptr (scratch is used).
static int keyed_wide_identity_dev(fabgpu_ctx* ctx, uint32_t n, const void* arena, size_t arena_bytes, const void* off, const void* key_id, uint32_t nkeys,
                                   const void* kt, const void* r, const void* s, void* verdict_bits, void* status, ShaPrefixArgs pa, hipStream_t st) {
    size_t wi = 0;
    void* wsp = nullptr;
    int rc = ctx->acquire_qws((size_t)n * (WIDE_SCRATCH_BYTES + 32), &wi, &wsp, st);
    if (rc != FABGPU_OK) return rc;
    void* dig = pa.digests ? pa.digests : (void*)((uint8_t*)wsp + (size_t)n * WIDE_SCRATCH_BYTES);
    if (ctx->time_kernels) hipEventRecord(ctx->ev0, st);
    hipError_t err = launch_p256_wide_pre(n, key_id, nkeys, kt, r, s, ctx->d_gtab, wsp, st);
    const bool coop = n <= SHA_COOP_MAX;                 // eight lanes per message, prefixed ones hashed whole: no mid-states (sha256_coop.h)
    if (err == hipSuccess && !coop && pa.m && pa.pre_idx && !pa.mid_ready) err = launch_sha256_midstates(arena, arena_bytes, pa, st);
    pa.digests = dig;
    if (err == hipSuccess) err = coop ? launch_sha256_messages_coop(n, arena, arena_bytes, off, pa, st) : launch_sha256_messages(n, arena, arena_bytes, off, pa, st);
    if (err == hipSuccess) err = launch_p256_wide_post(n, dig, r, ctx->d_gtab, wsp, verdict_bits, status, st);
    if (ctx->time_kernels) hipEventRecord(ctx->ev1, st);
    ctx->release_qws(wi, st);
    ctx->timed = ctx->time_kernels;
    return hip_to_rc(launched(ctx, err));
}

int fabgpu_sha256_p256_verify_batch_keyed_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off,
                                              const void* key_id, const void* r, const void* s, void* verdict_bits, void* status, void* stream) {
    if (!ctx || (n && (!arena || !off || !key_id || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (dev_too_big(n, arena_bytes)) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    hipStream_t st = (hipStream_t)stream;
    KeyedSnap snap(ctx, {st});
    if (snap.nkeys == 0) return FABGPU_EINVAL;
    DeviceGuard g(ctx->device);
    if (ctx->allow_wide && n <= (size_t)WIDE_LAUNCH_MAX)
        return keyed_wide_identity_dev(ctx, (uint32_t)n, arena, arena_bytes, off, key_id, snap.nkeys, (const void*)snap.kt, r, s, verdict_bits, status, ShaPrefixArgs(), st);
    VerifyLaunch v = verify_launch_common(ctx, n, r, s, verdict_bits, status);
    v.key_id = key_id; v.nkeys = snap.nkeys; v.ktabs = (const void*)snap.kt;
    v.arena = arena; v.arena_bytes = arena_bytes; v.off = off;
    return timed_launch(ctx, st, 0, [&](void*) { return launch_verify(v, st); });
}

// ---- host-pointer entry points (what the cgo provider binds) -----------------------------------------
// copy the span of the arena the offsets reference; returns rebased offsets in ctx->offs.h
static int stage_messages(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, size_t* arena_bytes_out) {
    DescribedPlan p(DescribedPlan::OWN_BUFFER, false, nullptr, 0, 0);
    p.see_rows(off, n, false);
    if (p.close()) return p.rc;
    const size_t span = p.span(), ab = round_up(span, 4) + 64;
    int rc;
    if ((rc = ctx->arena.ensure(ab + 64)) || (rc = ctx->offs.ensure((n + 1) * 4))) return rc;
    if (span) memcpy(ctx->arena.h, arena + p.lo, span);
    memset((uint8_t*)ctx->arena.h + span, 0, ab - span);
    p.rebase((uint32_t*)ctx->offs.h, off, n + 1, false);
    hipError_t err = hipMemcpyAsync(ctx->arena.d, ctx->arena.h, ab, hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(ctx->offs.d, ctx->offs.h, (n + 1) * 4, hipMemcpyHostToDevice, ctx->stream);
    *arena_bytes_out = ab;
    return hip_to_rc(err);
}

// What one host-pointer call stages through the context's pinned buffers, ctx->mu held: its messages (ctx->arena, ctx->offs), its
// n x 32 byte (P-384: n x 48 byte) fields behind an optional column of u32 ids (one Buf), and room in ctx->out for what comes back - verdict words, then
// status bytes at st_off; or n digests.  A step is skipped once one before it has failed (rc), and every call returns through fetch().
// THE FAILURE RULE, here and nowhere else: whatever failed - an allocation, an upload, the _dev call, the download - fetch() drains
// ctx->stream before it returns and nothing is copied to the caller.  Non-zero return, the caller's arrays untouched, nothing in
// flight: no transfer may still be reading a staging buffer when the next call refills it.
struct HostStage {
    fabgpu_ctx* ctx;
    const size_t n, fb, words, st_off;   // rows; bytes of one field; verdict words; where the status bytes start in ctx->out
    size_t kb = 0;                       // bytes of the id column in front of the fields: n ids padded to 64
    size_t ab = 0;                       // bytes of the staged arena
    uint8_t* d = nullptr;                // device base of ids | fields
    const size_t out_bytes;              // what comes back at most: n digests, or the verdict words and the status bytes
    int rc = FABGPU_OK;

    HostStage(fabgpu_ctx* c, size_t rows, bool digests = false, size_t field_bytes = 32)   // field_bytes: 32, or 48 for the P-384 calls
        : ctx(c), n(rows), fb(rows * field_bytes), words((rows + 63) / 64), st_off(round_up(words * 8, 64)), out_bytes(digests ? n * 32 : st_off + n) {}
    int room(Buf& b, size_t bytes) const { return ctx->fault == 2 ? FABGPU_ENOMEM : b.ensure(bytes); }   // FABGPU_FAULT_INJECT=oom: no staging either
    int room(DevBuf& b, size_t bytes) const { return ctx->fault == 2 ? FABGPU_ENOMEM : b.ensure(bytes); }
    void messages(const uint8_t* arena, const uint32_t* off) {
        if (rc == FABGPU_OK) rc = stage_messages(ctx, n, arena, off, &ab);
    }
    // ID_COLUMN: the fields sit behind an id column; ids may still be nullptr (the nym form's issuer ids are optional, their room is not).
    // OVERLAP: for fields of 256 KiB and more - field by field: the copy of a field into the pinned staging buffer, then ITS transfer -
    // the DMA of field k runs while the host copies field k + 1 (round 5; one transfer of all five behind all five copies left the bus
    // idle for the copies' 0.15 ms and the host idle for the transfer's 0.1 ms).  Small batches stay one transfer: five API calls would
    // cost more than they hide.
    enum : unsigned { ID_COLUMN = 1, OVERLAP = 2 };
    void fields(Buf& buf, unsigned how, const uint32_t* ids, std::initializer_list<const uint8_t*> src) {
        if (rc != FABGPU_OK) return;
        kb = (how & ID_COLUMN) ? round_up(n * 4, 64) : 0;
        const size_t total = kb + src.size() * fb;
        if ((rc = room(buf, total))) return;
        uint8_t* h = (uint8_t*)buf.h;
        d = (uint8_t*)buf.d;
        if (ids) memcpy(h, ids, n * 4);
        const bool each = (how & OVERLAP) && fb >= ((size_t)256 << 10);
        hipError_t err = each && kb ? hipMemcpyAsync(d, h, kb, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;   // (the ids travel first)
        size_t at = kb;
        for (const uint8_t* f : src) {
            if (err != hipSuccess) break;
            memcpy(h + at, f, fb);
            if (each) err = hipMemcpyAsync(d + at, h + at, fb, hipMemcpyHostToDevice, ctx->stream);
            at += fb;
        }
        if (!each) err = hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, ctx->stream);
        rc = hip_to_rc(err);
    }
    // behind the staging, before the _dev call: room for the results (the buffers are made in the order they always were)
    bool ready() {
        if (rc == FABGPU_OK) rc = room(ctx->out, out_bytes);
        return rc == FABGPU_OK;
    }
    const void* ids() const { return d; }
    const void* field(size_t f) const { return d + kb + f * fb; }
    void* dout() const { return ctx->out.d; }
    void* dstatus(const uint8_t* status) const { return status ? (uint8_t*)ctx->out.d + st_off : nullptr; }
    // the first `bytes` of ctx->out to the host behind everything queued, and the wait for it
    void download(size_t bytes) {
        if (rc == FABGPU_OK) rc = hip_to_rc(hipMemcpyAsync(ctx->out.h, ctx->out.d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    int drain() {
        const hipError_t drained = hipStreamSynchronize(ctx->stream);
        if (rc == FABGPU_OK) rc = hip_to_rc(drained);
        return rc;
    }
    int fetch(size_t bytes) {
        download(bytes);
        return drain();
    }
    int fetch_verdicts(uint64_t* verdict_bits, uint8_t* status) {
        if (fetch(status ? st_off + n : words * 8)) return rc;
        memcpy(verdict_bits, ctx->out.h, words * 8);
        if (status) memcpy(status, (uint8_t*)ctx->out.h + st_off, n);
        return FABGPU_OK;
    }
    int fetch_digests(uint8_t* digests) {
        if (fetch(n * 32)) return rc;
        memcpy(digests, ctx->out.h, n * 32);
        return FABGPU_OK;
    }
};

int fabgpu_p256_verify_batch(fabgpu_ctx* ctx, size_t n, const uint8_t* qx, const uint8_t* qy, const uint8_t* e, const uint8_t* r,
                             const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    if (!ctx || (n && (!qx || !qy || !e || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 160) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    HostStage h(ctx, n);
    h.fields(ctx->fields, HostStage::OVERLAP, nullptr, {qx, qy, e, r, s});
    if (h.ready())
        h.rc = fabgpu_p256_verify_batch_dev(ctx, n, h.field(0), h.field(1), h.field(2), h.field(3), h.field(4), h.dout(), h.dstatus(status), ctx->stream);
    return h.fetch_verdicts(verdict_bits, status);
}

int fabgpu_p256_verify_batch_keyed(fabgpu_ctx* ctx, size_t n, const uint32_t* key_id, const uint8_t* e, const uint8_t* r, const uint8_t* s,
                                   uint64_t* verdict_bits, uint8_t* status) {
    if (!ctx || (n && (!key_id || !e || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 100) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    HostStage h(ctx, n);
    h.fields(ctx->keyed, HostStage::ID_COLUMN, key_id, {e, r, s});
    if (h.ready())
        h.rc = fabgpu_p256_verify_batch_keyed_dev(ctx, n, h.ids(), h.field(0), h.field(1), h.field(2), h.dout(), h.dstatus(status), ctx->stream);
    return h.fetch_verdicts(verdict_bits, status);
}

// The three message-taking shapes, shared by the hash families: `dev` is the family's device-resident twin (SHA-256 here, SHA3-256
// below).
using HashDev = int (*)(fabgpu_ctx*, size_t, const void*, size_t, const void*, void*, void*);
using HashVerifyDev = int (*)(fabgpu_ctx*, size_t, const void*, size_t, const void*, const void*, const void*, const void*, const void*, void*, void*, void*);
using HashVerifyKeyedDev = int (*)(fabgpu_ctx*, size_t, const void*, size_t, const void*, const void*, const void*, const void*, void*, void*, void*);

static int hash_batch_host(HashDev dev, fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, uint8_t* digests) {
    if (!ctx || (n && (!off || !digests))) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 32) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    if (!arena && off[n] != off[0]) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    HostStage h(ctx, n, true);
    h.messages(arena, off);
    if (h.ready()) h.rc = dev(ctx, n, ctx->arena.d, h.ab, ctx->offs.d, h.dout(), ctx->stream);
    return h.fetch_digests(digests);
}

static int hash_verify_host(HashVerifyDev dev, fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint8_t* qx, const uint8_t* qy,
                            const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    if (!ctx || (n && (!off || !qx || !qy || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 160) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    if (!arena && off[n] != off[0]) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    HostStage h(ctx, n);
    h.messages(arena, off);
    h.fields(ctx->fields, 0, nullptr, {qx, qy, r, s});
    if (h.ready())
        h.rc = dev(ctx, n, ctx->arena.d, h.ab, ctx->offs.d, h.field(0), h.field(1), h.field(2), h.field(3), h.dout(), h.dstatus(status), ctx->stream);
    return h.fetch_verdicts(verdict_bits, status);
}

static int hash_verify_keyed_host(HashVerifyKeyedDev dev, fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint32_t* key_id,
                                  const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status, size_t field_bytes = 32) {
    if (!ctx || (n && (!off || !key_id || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 160) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    if (!arena && off[n] != off[0]) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    HostStage h(ctx, n, false, field_bytes);
    h.messages(arena, off);
    h.fields(ctx->keyed, HostStage::ID_COLUMN, key_id, {r, s});
    if (h.ready()) h.rc = dev(ctx, n, ctx->arena.d, h.ab, ctx->offs.d, h.ids(), h.field(0), h.field(1), h.dout(), h.dstatus(status), ctx->stream);
    return h.fetch_verdicts(verdict_bits, status);
}

int fabgpu_sha256_batch(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, uint8_t* digests) {
    return hash_batch_host(fabgpu_sha256_batch_dev, ctx, n, arena, off, digests);
}

int fabgpu_sha256_p256_verify_batch(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint8_t* qx,
                                    const uint8_t* qy, const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    return hash_verify_host(fabgpu_sha256_p256_verify_batch_dev, ctx, n, arena, off, qx, qy, r, s, verdict_bits, status);
}

int fabgpu_sha256_p256_verify_batch_keyed(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint32_t* key_id,
                                          const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    return hash_verify_keyed_host(fabgpu_sha256_p256_verify_batch_keyed_dev, ctx, n, arena, off, key_id, r, s, verdict_bits, status);
}

int fabgpu_idemix_nym_verify_batch(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint32_t* issuer_id,
                                   const uint8_t* nym_x, const uint8_t* nym_y, const uint8_t* proof_c, const uint8_t* proof_s_sk,
                                   const uint8_t* proof_s_r_nym, const uint8_t* nonce, uint64_t* verdict_bits, uint8_t* status) {
    if (!ctx || (n && (!off || !nym_x || !nym_y || !proof_c || !proof_s_sk || !proof_s_r_nym || !nonce || !verdict_bits))) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 200) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    if (!arena && off[n] != off[0]) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    HostStage h(ctx, n);
    h.messages(arena, off);
    h.fields(ctx->nym, HostStage::ID_COLUMN, issuer_id, {nym_x, nym_y, proof_c, proof_s_sk, proof_s_r_nym, nonce});
    if (h.ready())
        h.rc = fabgpu_idemix_nym_verify_batch_dev(ctx, n, ctx->arena.d, h.ab, ctx->offs.d, issuer_id ? h.ids() : nullptr, h.field(0), h.field(1), h.field(2),
                                                  h.field(3), h.field(4), h.field(5), h.dout(), h.dstatus(status), ctx->stream);
    return h.fetch_verdicts(verdict_bits, status);
}

// ---- SHA3-256 (sha3_kernels.hip): an MSP of the SHA3 hash family (msp/identities.go:216-224) ---------------------------------
// Hash, then verify: two launches on one stream.  The SHA3 launch writes its digests into a context-owned n x 32 byte device buffer -
// one of the pooled workspaces, under their rule (acquire_qws: reserved until an event is recorded behind the launch that read it) -
// and the unchanged verify-only entry point consumes that buffer as `e`: the digest never leaves the chip, and the verify kernel is
// chosen by n and the context's flags exactly as for a caller who brings digests.
// The SHA3-256 launches of a (possibly prefixed) batch, chosen by the context's switch.  Without FABGPU_FLAG_SHA3_COOP: the mid-state
// launch (unless pa.mid_ready) and the one-lane kernel, as ever.  With it: up to SHA3_COOP_MAX messages on 32 lanes each, prefixed ones
// hashed whole - no mid-state launch, pa.mid_scratch is not touched -; larger plain launches through the mixed kernel; larger prefixed
// ones on the one-lane road with its mid-states.
static hipError_t sha3_launch_messages(fabgpu_ctx* ctx, uint32_t n, const void* arena, size_t arena_bytes, const void* off, const ShaPrefixArgs& pa,
                                       hipStream_t st) {
    const bool prefixed = pa.m != 0 && pa.pre_idx != nullptr;
    if (ctx->sha3_coop.load(std::memory_order_relaxed)) {
        if (n <= SHA3_COOP_MAX) {
            const hipError_t err = launch_sha3_256_messages_coop(n, arena, arena_bytes, off, pa, st);
            if (err == hipSuccess) ctx->sha3_coop_rows.fetch_add(n, std::memory_order_relaxed);
            return err;
        }
        if (!prefixed) return launch_sha3_256_mixed(n, arena, arena_bytes, off, pa.spans, pa.digests, ctx->d_sha3_coop_rows, st);
    }
    hipError_t err = hipSuccess;
    if (prefixed && !pa.mid_ready) err = launch_sha3_256_midstates(arena, arena_bytes, pa, st);
    if (err == hipSuccess) err = launch_sha3_256_messages(n, arena, arena_bytes, off, pa, st);
    return err;
}

int fabgpu_sha3_256_batch_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, void* digests, void* stream) {
    if (!ctx || (n && (!arena || !off || !digests))) return FABGPU_EINVAL;
    if (dev_too_big(n, arena_bytes)) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    return timed_launch(ctx, st, 0, [&](void*) {
        ShaPrefixArgs pa;
        pa.digests = digests;
        return sha3_launch_messages(ctx, (uint32_t)n, arena, arena_bytes, off, pa, st);
    });
}

// the digests of a (possibly prefixed) batch into `dig`, then the verify-only entry point over them; key_id == nullptr: fresh keys
static int sha3_then_verify_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, ShaPrefixArgs pa, const void* qx,
                                const void* qy, const void* key_id, const void* r, const void* s, void* verdict_bits, void* status, hipStream_t st) {
    size_t di = 0;
    void* dig = pa.digests;
    const bool pooled = dig == nullptr;
    if (pooled) {
        int rc = ctx->acquire_qws(n * 32, &di, &dig, st);
        if (rc != FABGPU_OK) return rc;
    }
    pa.digests = dig;
    int rc = hip_to_rc(launched(ctx, sha3_launch_messages(ctx, (uint32_t)n, arena, arena_bytes, off, pa, st)));
    if (rc == FABGPU_OK)
        rc = key_id ? fabgpu_p256_verify_batch_keyed_dev(ctx, n, key_id, dig, r, s, verdict_bits, status, st)
                    : fabgpu_p256_verify_batch_dev(ctx, n, qx, qy, dig, r, s, verdict_bits, status, st);
    if (pooled) ctx->release_qws(di, st);
    return rc;
}

int fabgpu_sha3_256_p256_verify_batch_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, const void* qx,
                                          const void* qy, const void* r, const void* s, void* verdict_bits, void* status, void* stream) {
    if (!ctx || (n && (!arena || !off || !qx || !qy || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (dev_too_big(n, arena_bytes)) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    return sha3_then_verify_dev(ctx, n, arena, arena_bytes, off, ShaPrefixArgs(), qx, qy, nullptr, r, s, verdict_bits, status, (hipStream_t)stream);
}

int fabgpu_sha3_256_p256_verify_batch_keyed_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, const void* key_id,
                                                const void* r, const void* s, void* verdict_bits, void* status, void* stream) {
    if (!ctx || (n && (!arena || !off || !key_id || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (dev_too_big(n, arena_bytes)) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    return sha3_then_verify_dev(ctx, n, arena, arena_bytes, off, ShaPrefixArgs(), nullptr, nullptr, key_id, r, s, verdict_bits, status, (hipStream_t)stream);
}

int fabgpu_sha3_256_batch(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, uint8_t* digests) {
    return hash_batch_host(fabgpu_sha3_256_batch_dev, ctx, n, arena, off, digests);
}

int fabgpu_sha3_256_p256_verify_batch(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint8_t* qx, const uint8_t* qy,
                                      const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    return hash_verify_host(fabgpu_sha3_256_p256_verify_batch_dev, ctx, n, arena, off, qx, qy, r, s, verdict_bits, status);
}

int fabgpu_sha3_256_p256_verify_batch_keyed(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint32_t* key_id,
                                            const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    return hash_verify_keyed_host(fabgpu_sha3_256_p256_verify_batch_keyed_dev, ctx, n, arena, off, key_id, r, s, verdict_bits, status);
}

// ---- ECDSA P-384 (p384_kernels.hip): fresh keys, direct calls only --------------------------------------------------------------
// All operands 48 bytes big-endian per tuple.  Not in the block pass, no registered keys, no fabgpu_multi form.
// P-384's generator table: fifteen affine multiples, built by the host compilation of p384.h and uploaded by the context's first P-384
// call (a context that never sees a P-384 key allocates nothing and its construction is what it was)
static int p384_gtab(fabgpu_ctx* ctx) {
    std::lock_guard<std::mutex> lk(ctx->gtab384_mu);
    if (ctx->d_gtab384) return FABGPU_OK;
    uint32_t g384[fab::p384::P384_GTAB_WORDS];
    fab::p384::build_gtab(g384);
    uint32_t* d = nullptr;
    if (hipMalloc((void**)&d, sizeof(g384)) != hipSuccess) return FABGPU_ENOMEM;
    if (hipMemcpy(d, g384, sizeof(g384), hipMemcpyHostToDevice) != hipSuccess) {      // (synchronous: the table is there when this returns)
        hipFree(d);
        return FABGPU_ELAUNCH;
    }
    ctx->d_gtab384 = d;
    return FABGPU_OK;
}

static int p384_verify_dev(fabgpu_ctx* ctx, size_t n, const void* qx, const void* qy, const void* e, bool e_is_digest32, const void* r, const void* s,
                           void* verdict_bits, void* status, hipStream_t st) {
    if (int rc = p384_gtab(ctx)) return rc;
    P384Launch v;
    v.n = (uint32_t)n;
    v.qx = qx; v.qy = qy; v.e = e; v.e_is_digest32 = e_is_digest32; v.r = r; v.s = s;
    v.gtab = ctx->d_gtab384;
    v.verdict_bits = verdict_bits; v.status = status;
    return timed_launch(ctx, st, p384_workspace_bytes((uint32_t)n), [&](void* wsp) {
        v.qws = wsp;
        return launch_p384_verify(v, st);
    });
}

int fabgpu_p384_verify_batch_dev(fabgpu_ctx* ctx, size_t n, const void* qx, const void* qy, const void* e, const void* r, const void* s,
                                 void* verdict_bits, void* status, void* stream) {
    if (!ctx || (n && (!qx || !qy || !e || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (dev_too_big(n)) return FABGPU_ETOOBIG;
    DeviceGuard g(ctx->device);
    if (n == 0) return p384_gtab(ctx);            // the explicit warm call (fabgpu.h): the table, no launch
    return p384_verify_dev(ctx, n, qx, qy, e, false, r, s, verdict_bits, status, (hipStream_t)stream);
}

// Hash, then verify: the family's hash launch writes n x 32 digest bytes into a pooled context-owned buffer (as sha3_then_verify_dev
// does), the P-384 kernel reads them as 256-bit integers - Go's hashToInt for a digest shorter than the order - on the same stream.
static int hash_then_p384_dev(HashDev hash, fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, const void* qx,
                              const void* qy, const void* r, const void* s, void* verdict_bits, void* status, void* stream) {
    if (!ctx || (n && (!arena || !off || !qx || !qy || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (dev_too_big(n, arena_bytes)) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    size_t di = 0;
    void* dig = nullptr;
    int rc = ctx->acquire_qws(n * 32, &di, &dig, st);
    if (rc != FABGPU_OK) return rc;
    rc = hash(ctx, n, arena, arena_bytes, off, dig, stream);
    if (rc == FABGPU_OK) rc = p384_verify_dev(ctx, n, qx, qy, dig, true, r, s, verdict_bits, status, st);
    ctx->release_qws(di, st);
    return rc;
}
int fabgpu_sha256_p384_verify_batch_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, const void* qx,
                                        const void* qy, const void* r, const void* s, void* verdict_bits, void* status, void* stream) {
    return hash_then_p384_dev(fabgpu_sha256_batch_dev, ctx, n, arena, arena_bytes, off, qx, qy, r, s, verdict_bits, status, stream);
}
int fabgpu_sha3_256_p384_verify_batch_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, const void* qx,
                                          const void* qy, const void* r, const void* s, void* verdict_bits, void* status, void* stream) {
    return hash_then_p384_dev(fabgpu_sha3_256_batch_dev, ctx, n, arena, arena_bytes, off, qx, qy, r, s, verdict_bits, status, stream);
}

int fabgpu_p384_verify_batch(fabgpu_ctx* ctx, size_t n, const uint8_t* qx, const uint8_t* qy, const uint8_t* e, const uint8_t* r,
                             const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    if (!ctx || (n && (!qx || !qy || !e || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 240) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    HostStage h(ctx, n, false, 48);
    h.fields(ctx->fields, HostStage::OVERLAP, nullptr, {qx, qy, e, r, s});
    if (h.ready())
        h.rc = fabgpu_p384_verify_batch_dev(ctx, n, h.field(0), h.field(1), h.field(2), h.field(3), h.field(4), h.dout(), h.dstatus(status), ctx->stream);
    return h.fetch_verdicts(verdict_bits, status);
}

static int hash_p384_verify_host(HashVerifyDev dev, fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint8_t* qx, const uint8_t* qy,
                                 const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    if (!ctx || (n && (!off || !qx || !qy || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 240) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    if (!arena && off[n] != off[0]) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    HostStage h(ctx, n, false, 48);
    h.messages(arena, off);
    h.fields(ctx->fields, 0, nullptr, {qx, qy, r, s});
    if (h.ready())
        h.rc = dev(ctx, n, ctx->arena.d, h.ab, ctx->offs.d, h.field(0), h.field(1), h.field(2), h.field(3), h.dout(), h.dstatus(status), ctx->stream);
    return h.fetch_verdicts(verdict_bits, status);
}
int fabgpu_sha256_p384_verify_batch(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint8_t* qx, const uint8_t* qy,
                                    const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    return hash_p384_verify_host(fabgpu_sha256_p384_verify_batch_dev, ctx, n, arena, off, qx, qy, r, s, verdict_bits, status);
}
int fabgpu_sha3_256_p384_verify_batch(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint8_t* qx, const uint8_t* qy,
                                      const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    return hash_p384_verify_host(fabgpu_sha3_256_p384_verify_batch_dev, ctx, n, arena, off, qx, qy, r, s, verdict_bits, status);
}

// ---- registered P-384 keys (fabgpu_ctx::k384 has the story) ------------------------------------------------------------------------
namespace {

struct P384KeyName : std::string {      // qx || qy, 96 bytes
    P384KeyName(const uint8_t* qx48, const uint8_t* qy48) : std::string((const char*)qx48, 48) { append((const char*)qy48, 48); }
};
bool k384_stream(fabgpu_ctx* ctx) {
    return ctx->stream_k384 || hipStreamCreateWithFlags(&ctx->stream_k384, hipStreamNonBlocking) == hipSuccess;
}
// (k384_mu held, the context's device current) one drain as far as it goes without waiting for a launcher or a launch (wait: all the
// way).  true: done - the table and the array are on the free lists, the slot is reclaimable.
bool k384_drain_step_locked(fabgpu_ctx* ctx, fabgpu_ctx::Drain384& d, bool wait) {
    if (!d.recorded) {
        if (!ctx->fence384.quiet(wait)) return false;
        (void)ctx->fence384.record(d.evs, KeyedStreamOwned{ctx});
        d.recorded = true;
    }
    if (!ctx->fence384.done(d.evs, wait)) return false;
    if (d.tab) ctx->k384_tab_free.push_back(d.tab);
    if (d.tab16) ctx->k384_tab16_free.push_back(d.tab16);
    if (d.old_snap.p) ctx->snap384_free.push_back(d.old_snap);
    if (d.slot >= 0) ctx->k384.slots.drained((uint32_t)d.slot);     // (a parked slot stays parked)
    return true;
}
void k384_drain_advance_locked(fabgpu_ctx* ctx) {
    HipKeyedFence::advance(ctx->k384_drains, [ctx](fabgpu_ctx::Drain384& d, bool wait) { return k384_drain_step_locked(ctx, d, wait); });
}
bool k384_drain_wait_slot_locked(fabgpu_ctx* ctx, uint32_t slot) {
    return HipKeyedFence::wait_for(ctx->k384_drains, [slot](const fabgpu_ctx::Drain384& d) { return d.slot == (int64_t)slot; },
                                   [ctx](fabgpu_ctx::Drain384& d, bool wait) { return k384_drain_step_locked(ctx, d, wait); }) &&
           !ctx->k384.slots.draining(slot);
}
// (k384_mu held, the context's device current) the book as it is now becomes the snapshot later launches are handed: a fresh array,
// written and waited for before it replaces the previous one, which goes into `d` to be drained.  A failure leaves NO snapshot (every
// keyed row answers 4 until a later change of the book succeeds) - never a stale one.
int k384_publish_locked(fabgpu_ctx* ctx, fabgpu_ctx::Drain384& d) {
    const std::vector<fab::P384SlotSnap> snap = ctx->k384.snapshot();
    const size_t slot_bytes = sizeof(fab::P384SlotSnap) + (ctx->p384_tab16 ? sizeof(void*) : 0);     // (with the option: a second address per slot)
    d.old_snap = fabgpu_ctx::Snap384Room{(void*)ctx->d_snap384, ctx->snap384_cap};
    ctx->d_snap384 = nullptr;
    ctx->d_snap384x16 = nullptr;
    ctx->snap384_n = 0;
    ctx->snap384_cap = 0;
    if (snap.empty()) return FABGPU_OK;
    fabgpu_ctx::Snap384Room room{nullptr, 0};
    for (size_t i = 0; i < ctx->snap384_free.size(); i++)
        if (ctx->snap384_free[i].cap >= snap.size()) {
            room = ctx->snap384_free[i];
            ctx->snap384_free.erase(ctx->snap384_free.begin() + (long)i);
            break;
        }
    if (!room.p) {
        room.cap = 64;
        while (room.cap < snap.size()) room.cap *= 2;
        if (ctx->fault == 2 || hipMalloc(&room.p, room.cap * slot_bytes) != hipSuccess) return FABGPU_ENOMEM;
        ctx->k384_allocs.push_back(room.p);
        ctx->k384_snap_bytes += room.cap * slot_bytes;
    }
    // one image of the whole array: the slots, and behind the room's cap slots the 16-bit addresses
    const size_t off16 = room.cap * sizeof(fab::P384SlotSnap);
    std::vector<uint8_t> img(ctx->p384_tab16 ? off16 + snap.size() * sizeof(void*) : snap.size() * sizeof(fab::P384SlotSnap));
    memcpy(img.data(), snap.data(), snap.size() * sizeof(fab::P384SlotSnap));
    if (ctx->p384_tab16) {
        const std::vector<const uint32_t*> s16 = ctx->k384.snapshot16();
        memcpy(img.data() + off16, s16.data(), s16.size() * sizeof(void*));
    }
    hipError_t e = k384_stream(ctx) ? hipMemcpyAsync(room.p, img.data(), img.size(), hipMemcpyHostToDevice, ctx->stream_k384) : hipErrorLaunchFailure;
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream_k384);      // (`img` lives on this frame; and no launch is handed a half-written array)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->snap384_free.push_back(room);
        return hip_to_rc(e);
    }
    ctx->d_snap384 = (const fab::P384SlotSnap*)room.p;
    if (ctx->p384_tab16) ctx->d_snap384x16 = (const uint32_t* const*)((const uint8_t*)room.p + off16);
    ctx->snap384_n = (uint32_t)snap.size();
    ctx->snap384_cap = room.cap;
    return FABGPU_OK;
}
// (k384_mu held) `d` joins the drains if there is anything in it to wait for
void k384_drain_push_locked(fabgpu_ctx* ctx, fabgpu_ctx::Drain384&& d) {
    if (d.slot >= 0 || d.tab || d.tab16 || d.old_snap.p) ctx->k384_drains.push_back(std::move(d));
}
uint32_t* k384_tab_alloc_locked(fabgpu_ctx* ctx) {
    if (!ctx->k384_tab_free.empty()) {
        uint32_t* t = ctx->k384_tab_free.back();
        ctx->k384_tab_free.pop_back();
        return t;
    }
    void* t = nullptr;
    if (ctx->fault == 2 || hipMalloc(&t, fab::p384::CombTab384::TABLE_BYTES) != hipSuccess) return nullptr;
    ctx->k384_allocs.push_back(t);
    ctx->k384_n_tables++;
    return (uint32_t*)t;
}
// ---- the optional 16-bit tables (fabgpu_ctx::p384_tab16 has the story) ----
bool k384x16_stream(fabgpu_ctx* ctx) {
    return ctx->stream_k384x16 || hipStreamCreateWithFlags(&ctx->stream_k384x16, hipStreamNonBlocking) == hipSuccess;
}
// (k384_mu held) 144 MiB from the drained tables or the device; nullptr: the key (or the generator) simply has no 16-bit table
uint32_t* k384_tab16_alloc_locked(fabgpu_ctx* ctx) {
    if (!ctx->k384_tab16_free.empty()) {
        uint32_t* t = ctx->k384_tab16_free.back();
        ctx->k384_tab16_free.pop_back();
        return t;
    }
    void* t = nullptr;
    if (ctx->fault == 2 || hipMalloc(&t, fab::p384::CombTab384x16::TABLE_BYTES) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    ctx->k384_allocs.push_back(t);
    ctx->k384_n_tables16++;
    return (uint32_t*)t;
}
// (k384_build_mu and k384_mu held, the context's device current) the 16-bit build of the live key `id`, whose 8-bit table tab8 is
// complete, queued behind nothing the caller waits for.  Any refusal leaves the key without a 16-bit table and is no error.
void k384_queue16_locked(fabgpu_ctx* ctx, uint32_t id, const uint32_t* tab8) {
    if (!ctx->p384_tab16 || !ctx->d_gcomb384x16 || ctx->fault) return;
    if (ctx->k384.n_tables16() + ctx->k384_pending16.size() >= ctx->k384_tab16_cap) return;
    if (!k384x16_stream(ctx)) {
        (void)hipGetLastError();
        return;
    }
    hipEvent_t ev = ctx->fence384.get();      // (the fence's: a retirement may move it into a drain)
    if (!ev) return;
    uint32_t* t16 = k384_tab16_alloc_locked(ctx);
    if (!t16) {
        ctx->fence384.put(ev);
        return;
    }
    hipError_t e = launch_p384_keytab16_build(tab8, t16, ctx->stream_k384x16);
    if (e == hipSuccess) e = hipEventRecord(ev, ctx->stream_k384x16);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(ctx->stream_k384x16);      // (whatever was queued has run before the table is handed out again)
        (void)hipGetLastError();
        ctx->fence384.put(ev);
        ctx->k384_tab16_free.push_back(t16);
        return;
    }
    ctx->k384_pending16.push_back(fabgpu_ctx::Pending384x16{id, t16, ev});
}
// (k384_mu held, the context's device current) builds that have finished (wait: all of them, waited for - the test hooks only) enter
// the book, and if any did, the book is published again.  A publication that fails here keeps the snapshot in place: it is not stale,
// it only lacks the new addresses, and the next change of the book tries again.
void k384_poll16_locked(fabgpu_ctx* ctx, bool wait = false) {
    if (ctx->k384_pending16.empty()) return;
    bool news = false;
    for (size_t i = 0; i < ctx->k384_pending16.size();) {
        const fabgpu_ctx::Pending384x16 q = ctx->k384_pending16[i];
        const hipError_t e = wait ? hipEventSynchronize(q.ev) : hipEventQuery(q.ev);
        if (e == hipErrorNotReady) {
            (void)hipGetLastError();
            i++;
            continue;
        }
        ctx->fence384.put(q.ev);
        ctx->k384_pending16.erase(ctx->k384_pending16.begin() + (long)i);
        if (e == hipSuccess && ctx->k384.set_table16(q.id, q.tab)) {
            news = true;
        } else {                                   // (a failed device: nothing of it runs any more)
            (void)hipGetLastError();
            ctx->k384_tab16_free.push_back(q.tab);
        }
    }
    if (!news) return;
    const fab::P384SlotSnap* keep = ctx->d_snap384;
    const uint32_t* const* keep16 = ctx->d_snap384x16;
    const uint32_t keep_n = ctx->snap384_n;
    const size_t keep_cap = ctx->snap384_cap;
    fabgpu_ctx::Drain384 d;
    if (k384_publish_locked(ctx, d) != FABGPU_OK) {
        ctx->d_snap384 = keep;
        ctx->d_snap384x16 = keep16;
        ctx->snap384_n = keep_n;
        ctx->snap384_cap = keep_cap;
        return;
    }
    k384_drain_push_locked(ctx, std::move(d));
}
// (k384_build_mu held, the context's device current) the generator's 16-bit table from its finished 8-bit one, and the counter of the
// rows the 24-window stream verified: once per context, waited for.  A failure leaves the context on 8-bit tables and is no error.
void k384_gcomb16_build(fabgpu_ctx* ctx, const uint32_t* g8) {
    uint32_t* t16 = nullptr;
    void* ctr = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->k384_mu);
        if (!ctx->p384_tab16 || ctx->d_gcomb384x16 || ctx->fault || !k384x16_stream(ctx)) {
            (void)hipGetLastError();
            return;
        }
        if (hipMalloc(&ctr, 16) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        ctx->k384_allocs.push_back(ctr);
        if (!(t16 = k384_tab16_alloc_locked(ctx))) return;
    }
    hipError_t e = hipMemsetAsync(ctr, 0, 16, ctx->stream_k384x16);
    if (e == hipSuccess) e = launch_p384_keytab16_build(g8, t16, ctx->stream_k384x16);
    const hipError_t drained = hipStreamSynchronize(ctx->stream_k384x16);
    std::lock_guard<std::mutex> lk(ctx->k384_mu);
    if (e != hipSuccess || drained != hipSuccess) {
        (void)hipGetLastError();
        ctx->k384_tab16_free.push_back(t16);
        return;
    }
    ctx->d_k384_rows16 = (unsigned long long*)ctr;
    ctx->d_gcomb384x16 = t16;
}
// (k384_build_mu held, the context's device current) the comb tables of m points (qxy: m x 96 bytes) into tabs[0 .. m), complete on return
int k384_build_locked(fabgpu_ctx* ctx, uint32_t m, const uint8_t* qxy, uint32_t* const* tabs) {
    if (ctx->fault) return ctx->fault == 2 ? FABGPU_ENOMEM : FABGPU_ELAUNCH;
    const size_t in_bytes = (size_t)96 * m + sizeof(void*) * m, scr_bytes = p384_keytab_scratch_bytes(m);
    if (ctx->k384_in_cap < in_bytes) {
        if (ctx->d_k384_in) hipFree(ctx->d_k384_in);
        ctx->d_k384_in = nullptr;
        ctx->k384_in_cap = 0;
        if (hipMalloc(&ctx->d_k384_in, in_bytes * 2) != hipSuccess) return FABGPU_ENOMEM;
        ctx->k384_in_cap = in_bytes * 2;
    }
    if (ctx->k384_scr_cap < scr_bytes) {
        if (ctx->d_k384_scr) hipFree(ctx->d_k384_scr);
        ctx->d_k384_scr = nullptr;
        ctx->k384_scr_cap = 0;
        if (hipMalloc(&ctx->d_k384_scr, scr_bytes * 2) != hipSuccess) return FABGPU_ENOMEM;
        ctx->k384_scr_cap = scr_bytes * 2;
    }
    if (!k384_stream(ctx)) return FABGPU_ELAUNCH;
    std::vector<uint8_t> in(in_bytes);
    memcpy(in.data(), qxy, (size_t)96 * m);
    memcpy(&in[(size_t)96 * m], tabs, sizeof(void*) * m);
    hipStream_t st = ctx->stream_k384;
    hipError_t e = hipMemcpyAsync(ctx->d_k384_in, in.data(), in_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_p384_keytab_build(m, ctx->d_k384_in, (void* const*)((uint8_t*)ctx->d_k384_in + (size_t)96 * m), ctx->d_k384_scr, st);
    const hipError_t drained = hipStreamSynchronize(st);         // (`in` lives on this frame; a table is complete before anybody learns its address)
    return hip_to_rc(e != hipSuccess ? e : drained);
}
// the generator's comb: the builder run on G, once per context, at the first registration or keyed call
int p384_gcomb(fabgpu_ctx* ctx) {
    {
        std::lock_guard<std::mutex> lk(ctx->k384_mu);
        if (ctx->d_gcomb384) return FABGPU_OK;
    }
    std::lock_guard<std::mutex> blk(ctx->k384_build_mu);
    uint32_t* t = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->k384_mu);
        if (ctx->d_gcomb384) return FABGPU_OK;
        if (!(t = k384_tab_alloc_locked(ctx))) return FABGPU_ENOMEM;
    }
    uint8_t g[96];
    fab::p384::generator_be(g, g + 48);
    const int rc = k384_build_locked(ctx, 1, g, &t);
    {
        std::lock_guard<std::mutex> lk(ctx->k384_mu);
        if (rc != FABGPU_OK) ctx->k384_tab_free.push_back(t);
        else ctx->d_gcomb384 = t;
    }
    if (rc == FABGPU_OK) k384_gcomb16_build(ctx, t);
    return rc;
}
// n points of the curve (qxy: n x 96 bytes; the caller's gate) registered on one context: one build for those the context does not have
// yet, ids in the order of qxy (keys the context has keep theirs).  Any failure: nothing was installed that is not complete.
int p384_key_register_batch(fabgpu_ctx* ctx, int n, const uint8_t* qxy, uint32_t* key_ids) {
    DeviceGuard g(ctx->device);
    if (int rc = p384_gcomb(ctx)) return rc;
    std::lock_guard<std::mutex> blk(ctx->k384_build_mu);
    std::vector<std::string> names((size_t)n);
    std::vector<int> todo;                                      // first occurrences of keys the context does not have
    std::vector<uint32_t*> tabs;
    auto give_back_locked = [&] {
        for (uint32_t* t : tabs)
            if (t) ctx->k384_tab_free.push_back(t);
    };
    {
        std::lock_guard<std::mutex> lk(ctx->k384_mu);
        for (int i = 0; i < n; i++) {
            names[(size_t)i].assign((const char*)qxy + 96 * (size_t)i, 96);
            bool dup = false;
            uint32_t id;
            for (int j : todo) dup = dup || names[(size_t)j] == names[(size_t)i];
            if (!dup && !ctx->k384.lookup(names[(size_t)i], &id)) todo.push_back(i);
        }
        if (todo.size() > ctx->k384.slots.room()) return FABGPU_ENOMEM;
        k384_drain_advance_locked(ctx);
        for (size_t t = 0; t < todo.size(); t++) {
            uint32_t* d = k384_tab_alloc_locked(ctx);
            if (!d) {
                give_back_locked();
                return FABGPU_ENOMEM;
            }
            tabs.push_back(d);
        }
    }
    const uint32_t m = (uint32_t)todo.size();
    if (m) {
        std::vector<uint8_t> keys((size_t)96 * m);
        for (uint32_t t = 0; t < m; t++) memcpy(&keys[(size_t)96 * t], qxy + 96 * (size_t)todo[t], 96);
        if (int rc = k384_build_locked(ctx, m, keys.data(), tabs.data())) {
            std::lock_guard<std::mutex> lk(ctx->k384_mu);
            give_back_locked();
            return rc;
        }
    }
    std::lock_guard<std::mutex> lk(ctx->k384_mu);
    int rc = FABGPU_OK;
    for (uint32_t t = 0; t < m && rc == FABGPU_OK; t++) {
        const int64_t slot = ctx->k384.slots.next_slot();
        if (slot < 0) rc = FABGPU_ENOMEM;
        else if (ctx->k384.slots.draining((uint32_t)slot) && !k384_drain_wait_slot_locked(ctx, (uint32_t)slot)) rc = FABGPU_ELAUNCH;
        if (rc != FABGPU_OK) break;
        const uint32_t id = ctx->k384.install(names[(size_t)todo[t]], tabs[t]);
        k384_queue16_locked(ctx, id, tabs[t]);
        tabs[t] = nullptr;
    }
    give_back_locked();
    if (m) {
        fabgpu_ctx::Drain384 d;
        const int prc = k384_publish_locked(ctx, d);
        k384_drain_push_locked(ctx, std::move(d));
        if (rc == FABGPU_OK) rc = prc;
    }
    k384_poll16_locked(ctx);
    for (int i = 0; i < n && rc == FABGPU_OK; i++)
        if (!ctx->k384.lookup(names[(size_t)i], &key_ids[i])) rc = FABGPU_ELAUNCH;
    return rc;
}

// What a keyed P-384 launch site takes of the book, under k384_mu, and its ticket of fence384, held until its keyed launch is queued
// (the destructor).  Nothing between the two may take k384_mu.
struct KeyedSnap384 {
    const fab::P384SlotSnap* snap = nullptr;
    uint32_t nkeys = 0;
    const uint32_t* gcomb = nullptr;
    const uint32_t* gcomb16 = nullptr;         // all three null without FABGPU_FLAG_P384_KEY_TABLES_16BIT (or without the generator's 16-bit table)
    const uint32_t* const* snap16 = nullptr;
    void* rows16 = nullptr;
    HipKeyedFence::Ticket ticket;
    KeyedSnap384(fabgpu_ctx* ctx, hipStream_t st) {
        std::lock_guard<std::mutex> lk(ctx->k384_mu);
        k384_poll16_locked(ctx);               // (finished 16-bit builds: hipEventQuery, and a fresh snapshot if there is news)
        snap = ctx->d_snap384;
        nkeys = ctx->snap384_n;
        gcomb = ctx->d_gcomb384;
        if (ctx->d_gcomb384x16 && (ctx->d_snap384x16 || !nkeys)) {
            gcomb16 = ctx->d_gcomb384x16;
            snap16 = ctx->d_snap384x16;
            rows16 = ctx->d_k384_rows16;
        }
        ticket = ctx->fence384.enter({st});
    }
};

int p384_verify_keyed_dev(fabgpu_ctx* ctx, size_t n, const void* key_id, const void* e, bool e_is_digest32, const void* r, const void* s,
                          void* verdict_bits, void* status, hipStream_t st) {
    if (int rc = p384_gcomb(ctx)) return rc;
    KeyedSnap384 snap(ctx, st);
    P384KeyedLaunch v;
    v.n = (uint32_t)n;
    v.key_id = key_id; v.e = e; v.e_is_digest32 = e_is_digest32; v.r = r; v.s = s;
    v.gcomb = snap.gcomb; v.snap = snap.snap; v.nkeys = snap.nkeys;
    v.gcomb16 = snap.gcomb16; v.snap16 = (const void* const*)snap.snap16; v.rows16 = snap.rows16;
    v.verdict_bits = verdict_bits; v.status = status;
    ctx->k384_launches.fetch_add(1, std::memory_order_relaxed);
    if (fab::ctx_p384_wide_serves(ctx, n)) {
        ctx->k384_wide_rows.fetch_add(n, std::memory_order_relaxed);
        return timed_launch(ctx, st, P384_WIDE_WS_BYTES, [&](void* wsp) {
            v.wide_scratch = wsp;
            return launch_p384_verify_keyed_wide(v, st);
        });
    }
    return timed_launch(ctx, st, 0, [&](void*) { return launch_p384_verify_keyed(v, st); });
}

int hash_then_p384_keyed_dev(HashDev hash, fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off, const void* key_id,
                             const void* r, const void* s, void* verdict_bits, void* status, void* stream) {
    if (!ctx || (n && (!arena || !off || !key_id || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (dev_too_big(n, arena_bytes)) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    size_t di = 0;
    void* dig = nullptr;
    int rc = ctx->acquire_qws(n * 32, &di, &dig, st);
    if (rc != FABGPU_OK) return rc;
    rc = hash(ctx, n, arena, arena_bytes, off, dig, stream);
    if (rc == FABGPU_OK) rc = p384_verify_keyed_dev(ctx, n, key_id, dig, true, r, s, verdict_bits, status, st);
    ctx->release_qws(di, st);
    return rc;
}

}  // namespace

int fabgpu_p384_key_register(fabgpu_ctx* ctx, const uint8_t* qx48, const uint8_t* qy48, uint32_t* key_id) {
    if (!ctx || !qx48 || !qy48 || !key_id) return FABGPU_EINVAL;
    if (!fabgpu_p384_pubkey_on_curve(qx48, qy48)) return FABGPU_EINVAL;   // the KeyImport gate: such keys stay with bccsp/sw
    const P384KeyName k(qx48, qy48);
    return p384_key_register_batch(ctx, 1, (const uint8_t*)k.data(), key_id);
}

int fabgpu_p384_key_register_many(fabgpu_ctx* const* ctxs, int n, const uint8_t* qx48, const uint8_t* qy48, uint32_t* key_ids) {
    if (!ctxs || n <= 0 || !qx48 || !qy48 || !key_ids) return FABGPU_EINVAL;
    for (int g = 0; g < n; g++)
        if (!ctxs[g]) return FABGPU_EINVAL;
    if (!fabgpu_p384_pubkey_on_curve(qx48, qy48)) return FABGPU_EINVAL;
    const P384KeyName k(qx48, qy48);
    for (int g = 0; g < n; g++)
        if (int rc = p384_key_register_batch(ctxs[g], 1, (const uint8_t*)k.data(), &key_ids[g])) return rc;   // (contexts before it keep the key: idempotent)
    return FABGPU_OK;
}

int fabgpu_p384_key_lookup(fabgpu_ctx* ctx, const uint8_t* qx48, const uint8_t* qy48, uint32_t* key_id) {
    if (!ctx || !qx48 || !qy48 || !key_id) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->k384_mu);
    return ctx->k384.lookup(P384KeyName(qx48, qy48), key_id) ? FABGPU_OK : 1;
}

int fabgpu_p384_key_count(fabgpu_ctx* ctx) {
    if (!ctx) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->k384_mu);
    return (int)ctx->k384.slots.n_live();
}

int fabgpu_p384_key_unregister(fabgpu_ctx* ctx, uint32_t key_id) {
    if (!ctx) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->k384_mu);
    fabgpu_ctx::Drain384 d;
    if (ctx->k384.retire(key_id, &d.tab, &d.tab16)) return 1;
    d.slot = fab::KeySlots::slot_of(key_id);
    DeviceGuard g(ctx->device);
    for (size_t i = 0; i < ctx->k384_pending16.size(); i++)
        if (ctx->k384_pending16[i].id == key_id) {             // its 16-bit build is still queued: the drain waits for it too
            d.tab16 = ctx->k384_pending16[i].tab;
            d.evs.push_back(ctx->k384_pending16[i].ev);
            ctx->k384_pending16.erase(ctx->k384_pending16.begin() + (long)i);
            break;
        }
    // launches queued before this moment hold the previous snapshot and answer for the key; none queued from now on can name it
    (void)k384_publish_locked(ctx, d);
    k384_drain_push_locked(ctx, std::move(d));
    k384_drain_advance_locked(ctx);
    return FABGPU_OK;
}

int fabgpu_p384_wide_rows(fabgpu_ctx* ctx, uint64_t* rows) {
    if (!ctx || !rows) return FABGPU_EINVAL;
    *rows = ctx->k384_wide_rows.load(std::memory_order_relaxed);
    return FABGPU_OK;
}

// rows hashed on 32 lanes so far: the small launches as queued, the long rows of the mixed kernel as the device has counted them
int fabgpu_sha3_coop_rows(fabgpu_ctx* ctx, uint64_t* rows) {
    if (!ctx || !rows) return FABGPU_EINVAL;
    *rows = ctx->sha3_coop_rows.load(std::memory_order_relaxed);
    if (!ctx->d_sha3_coop_rows) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    unsigned long long v = 0;
    if (hipMemcpy(&v, ctx->d_sha3_coop_rows, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return FABGPU_ELAUNCH;
    }
    *rows += v;
    return FABGPU_OK;
}

int fabgpu_p384_tables16_rows(fabgpu_ctx* ctx, uint64_t* rows) {
    if (!ctx || !rows) return FABGPU_EINVAL;
    *rows = 0;
    std::lock_guard<std::mutex> lk(ctx->k384_mu);
    if (!ctx->d_k384_rows16) return FABGPU_OK;
    DeviceGuard g(ctx->device);
    unsigned long long v = 0;
    if (hipMemcpy(&v, ctx->d_k384_rows16, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return FABGPU_ELAUNCH;
    }
    *rows = v;
    return FABGPU_OK;
}

int fabgpu_p384_key_table_stats(fabgpu_ctx* ctx, uint64_t* out, int cap) {
    if (!ctx || (cap > 0 && !out)) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->k384_mu);
    {
        DeviceGuard g(ctx->device);
        k384_drain_advance_locked(ctx);
        k384_poll16_locked(ctx);
    }
    const uint64_t bytes = ctx->k384_n_tables * (uint64_t)fab::p384::CombTab384::TABLE_BYTES + ctx->k384_snap_bytes;
    const uint64_t live16 = ctx->k384.n_tables16();
    const uint64_t v[FABGPU_P384_KEY_TABLE_STATS] = {ctx->k384.slots.n_live(), ctx->k384.slots.n_draining(), ctx->k384.slots.n_reused(), ctx->k384.slots.n_parked(),
                                                     ctx->k384_launches.load(std::memory_order_relaxed), bytes, ctx->k384.slots.high_water(),
                                                     live16, live16 * (uint64_t)fab::p384::CombTab384x16::TABLE_BYTES};
    for (int i = 0; i < cap && i < FABGPU_P384_KEY_TABLE_STATS; i++) out[i] = v[i];
    return FABGPU_P384_KEY_TABLE_STATS;
}

int fabgpu_p384_verify_batch_keyed_dev(fabgpu_ctx* ctx, size_t n, const void* key_id, const void* e, const void* r, const void* s,
                                       void* verdict_bits, void* status, void* stream) {
    if (!ctx || (n && (!key_id || !e || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (dev_too_big(n)) return FABGPU_ETOOBIG;
    DeviceGuard g(ctx->device);
    if (n == 0) return p384_gcomb(ctx);            // the explicit warm call (fabgpu.h): the generator's comb, no launch
    return p384_verify_keyed_dev(ctx, n, key_id, e, false, r, s, verdict_bits, status, (hipStream_t)stream);
}
int fabgpu_sha256_p384_verify_batch_keyed_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off,
                                              const void* key_id, const void* r, const void* s, void* verdict_bits, void* status, void* stream) {
    return hash_then_p384_keyed_dev(fabgpu_sha256_batch_dev, ctx, n, arena, arena_bytes, off, key_id, r, s, verdict_bits, status, stream);
}
int fabgpu_sha3_256_p384_verify_batch_keyed_dev(fabgpu_ctx* ctx, size_t n, const void* arena, size_t arena_bytes, const void* off,
                                                const void* key_id, const void* r, const void* s, void* verdict_bits, void* status, void* stream) {
    return hash_then_p384_keyed_dev(fabgpu_sha3_256_batch_dev, ctx, n, arena, arena_bytes, off, key_id, r, s, verdict_bits, status, stream);
}

int fabgpu_p384_verify_batch_keyed(fabgpu_ctx* ctx, size_t n, const uint32_t* key_id, const uint8_t* e, const uint8_t* r, const uint8_t* s,
                                   uint64_t* verdict_bits, uint8_t* status) {
    if (!ctx || (n && (!key_id || !e || !r || !s || !verdict_bits))) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 160) return FABGPU_ETOOBIG;
    if (n == 0) return FABGPU_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    HostStage h(ctx, n, false, 48);
    h.fields(ctx->keyed, HostStage::ID_COLUMN, key_id, {e, r, s});
    if (h.ready())
        h.rc = fabgpu_p384_verify_batch_keyed_dev(ctx, n, h.ids(), h.field(0), h.field(1), h.field(2), h.dout(), h.dstatus(status), ctx->stream);
    return h.fetch_verdicts(verdict_bits, status);
}
int fabgpu_sha256_p384_verify_batch_keyed(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint32_t* key_id,
                                          const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    return hash_verify_keyed_host(fabgpu_sha256_p384_verify_batch_keyed_dev, ctx, n, arena, off, key_id, r, s, verdict_bits, status, 48);
}
int fabgpu_sha3_256_p384_verify_batch_keyed(fabgpu_ctx* ctx, size_t n, const uint8_t* arena, const uint32_t* off, const uint32_t* key_id,
                                            const uint8_t* r, const uint8_t* s, uint64_t* verdict_bits, uint8_t* status) {
    return hash_verify_keyed_host(fabgpu_sha3_256_p384_verify_batch_keyed_dev, ctx, n, arena, off, key_id, r, s, verdict_bits, status, 48);
}

// ---- identity.Verify over a described batch: optional shared prefixes, fresh or registered keys ------------------------
int fabgpu_identity_verify_batch_dev(fabgpu_ctx* ctx, const fabgpu_identity_batch* b, void* mid_scratch, void* stream) {
    if (!ctx || !b) return FABGPU_EINVAL;
    const size_t n = b->n;
    if (n == 0) return FABGPU_OK;
    const bool keyed = b->key_id != nullptr;
    const bool prefixed = b->n_prefixes != 0 && b->pre_idx != nullptr;
    if (!b->arena || !b->off || !b->r || !b->s || !b->verdict_bits || (!keyed && (!b->qx || !b->qy))) return FABGPU_EINVAL;
    if (prefixed && (!b->pre_off || !mid_scratch)) return FABGPU_EINVAL;
    if (b->flags & ~(uint32_t)(FABGPU_IDB_SPANS | FABGPU_IDB_SHA3_256)) return FABGPU_EINVAL;
    if (n > 0xFFFFFFF0ull || b->arena_bytes > 0xFFFFFFFFull) return FABGPU_ETOOBIG;
    if (b->n_gather && (!b->gather_spans || !b->gather_digests || !b->gather_off || !b->gather_scratch || b->gather_scratch_bytes > 0xFFFFFFFFull))
        return FABGPU_EINVAL;
    ShaPrefixArgs pa;
    pa.spans = (b->flags & FABGPU_IDB_SPANS) != 0;
    pa.digests = b->digests;
    if (prefixed) {
        pa.m = b->n_prefixes;
        pa.pre_off = b->pre_off;
        pa.pre_idx = b->pre_idx;
        pa.mid_scratch = mid_scratch;
    }
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    hipError_t err;
    if (b->flags & FABGPU_IDB_SHA3_256) {
        // messages and prefixes under SHA3-256 (mid_scratch: n_prefixes x 200 bytes), the verification over the digests; the gathered
        // digests stay SHA-256 - TxID and proposal hash are SHA-256 whatever the MSP's family (protoutil/proputils.go:357-375)
        int rc = sha3_then_verify_dev(ctx, n, b->arena, b->arena_bytes, b->off, pa, b->qx, b->qy, b->key_id, b->r, b->s, b->verdict_bits, b->status, st);
        if (rc != FABGPU_OK) return rc;
        err = hipSuccess;
        if (b->n_gather)
            err = launch_gather_sha256(b->n_gather, b->arena, b->arena_bytes, b->gather_spans, b->gather_off, b->gather_scratch, b->gather_scratch_bytes,
                                       b->gather_digests, st);
        return hip_to_rc(err);
    }
    VerifyLaunch v;
    v.n = (uint32_t)n;
    v.arena = b->arena; v.arena_bytes = b->arena_bytes; v.off = b->off; v.pa = pa;
    v.r = b->r; v.s = b->s;
    v.gtab = ctx->d_gtab;
    v.verdict_bits = b->verdict_bits; v.status = b->status;
    v.allow_pair = ctx->allow_pair;
    if (keyed) {
        KeyedSnap snap(ctx, {st});
        const uint32_t nkeys = snap.nkeys;
        const int32_t** kt = snap.kt;
        if (nkeys == 0) return FABGPU_EINVAL;
        if (ctx->allow_wide && n <= (size_t)WIDE_LAUNCH_MAX) {
            int rc = keyed_wide_identity_dev(ctx, (uint32_t)n, b->arena, b->arena_bytes, b->off, b->key_id, nkeys, (const void*)kt, b->r, b->s, b->verdict_bits,
                                             b->status, pa, st);
            if (rc != FABGPU_OK) return rc;
            err = hipSuccess;
            if (b->n_gather)
                err = launch_gather_sha256(b->n_gather, b->arena, b->arena_bytes, b->gather_spans, b->gather_off, b->gather_scratch, b->gather_scratch_bytes,
                                           b->gather_digests, st);
            return hip_to_rc(err);
        }
        if (ctx->time_kernels) hipEventRecord(ctx->ev0, st);
        v.key_id = b->key_id; v.nkeys = nkeys; v.ktabs = (const void*)kt;
        err = launch_verify(v, st);
        if (ctx->time_kernels) hipEventRecord(ctx->ev1, st);
    } else {
        size_t wi = 0;
        void* wsp = nullptr;
        int rc = ctx->acquire_qws(verify_workspace_bytes((uint32_t)n, ctx->allow_pair), &wi, &wsp, st);
        if (rc != FABGPU_OK) return rc;
        if (ctx->time_kernels) hipEventRecord(ctx->ev0, st);
        v.qx = b->qx; v.qy = b->qy; v.qws = wsp;
        err = launch_verify(v, st);
        if (ctx->time_kernels) hipEventRecord(ctx->ev1, st);
        ctx->release_qws(wi, st);
    }
    ctx->timed = ctx->time_kernels;
    err = launched(ctx, err);
    if (err == hipSuccess && b->n_gather)   // behind the verification on the same stream; not part of fabgpu_last_kernel_ms
        err = launch_gather_sha256(b->n_gather, b->arena, b->arena_bytes, b->gather_spans, b->gather_off, b->gather_scratch, b->gather_scratch_bytes,
                                   b->gather_digests, st);
    return hip_to_rc(err);
}

}  // extern "C"

static int keep_acquire(fabgpu_ctx* ctx, size_t len);
namespace fab {
// `n` pool buffers of block_bytes each, pinned now (provider construction) instead of inside the first passes' uploads
void host_copy_preallocate(fabgpu_ctx* ctx, size_t block_bytes, uint32_t n) {
    if (!ctx || !block_bytes) return;
    DeviceGuard g(ctx->device);
    std::vector<int> got;
    for (uint32_t i = 0; i < n; i++) {
        const int idx = keep_acquire(ctx, block_bytes);
        if (idx < 0) break;
        got.push_back(idx);
    }
    // ... and sent through the DMA path once, whole: the first transfer out of a freshly registered range costs milliseconds (measured
    // with tools/gpu_r06_first_memo_probe.py: 2.2 ms "wait for upload" on a provider's first memo-seeding pass against 0.2-0.3 after)
    void* d = nullptr;
    if (!got.empty() && hipMalloc(&d, block_bytes) == hipSuccess) {
        for (int idx : got) (void)hipMemcpy(d, ctx->keep_pool[(size_t)idx]->pin.h, block_bytes, hipMemcpyHostToDevice);
        hipFree(d);
    }
    std::lock_guard<std::mutex> lk(ctx->keep_mu);
    for (int idx : got) ctx->keep_pool[(size_t)idx]->in_use = false;
    ctx->keep_refused = 0;
}
void host_copy_release(HostCopy* c) {
    if (!c || !c->ctx || c->idx < 0) {
        if (c) *c = HostCopy();
        return;
    }
    {
        std::lock_guard<std::mutex> lk(c->ctx->keep_mu);
        if ((size_t)c->idx < c->ctx->keep_pool.size()) c->ctx->keep_pool[(size_t)c->idx]->in_use = false;
    }
    *c = HostCopy();
}
void host_copy_limit(fabgpu_ctx* ctx, uint32_t blocks) {
    if (!ctx) return;
    std::lock_guard<std::mutex> lk(ctx->keep_mu);
    ctx->keep_max = blocks > 64 ? 64 : blocks;
}
void host_copy_stats(fabgpu_ctx* ctx, uint64_t* held, uint64_t* bytes_held, uint64_t* refused) {
    uint64_t h = 0, b = 0, r = 0;
    if (ctx) {
        std::lock_guard<std::mutex> lk(ctx->keep_mu);
        for (const auto& k : ctx->keep_pool)
            if (k->in_use) {
                h++;
                b += k->pin.cap;
            }
        r = ctx->keep_refused;
    }
    if (held) *held = h;
    if (bytes_held) *bytes_held = b;
    if (refused) *refused = r;
}
}  // namespace fab

// a buffer of the keep pool with room for `len` bytes, marked in use; -1: none to spare (or fault injection "oom")
static int keep_acquire(fabgpu_ctx* ctx, size_t len) {
    if (ctx->fault == 2) return -1;
    int idx = -1;
    {
        std::lock_guard<std::mutex> lk(ctx->keep_mu);
        if (ctx->keep_pool.capacity() < 64) ctx->keep_pool.reserve(64);   // (holders read their entry without the lock: the array never moves)
        // a free buffer that is already large enough, else any free one, else a new one while the pool may grow
        for (size_t i = 0; i < ctx->keep_pool.size() && idx < 0; i++)
            if (!ctx->keep_pool[i]->in_use && ctx->keep_pool[i]->pin.cap >= len) idx = (int)i;
        for (size_t i = 0; i < ctx->keep_pool.size() && idx < 0; i++)
            if (!ctx->keep_pool[i]->in_use) idx = (int)i;
        if (idx < 0 && ctx->keep_pool.size() < ctx->keep_max) {
            ctx->keep_pool.emplace_back(new fabgpu_ctx::KeepBuf);
            idx = (int)ctx->keep_pool.size() - 1;
        }
        if (idx < 0) {
            ctx->keep_refused++;
            return -1;
        }
        ctx->keep_pool[(size_t)idx]->in_use = true;
    }
    // (pinning outside the pool's lock: the buffer is ours)
    if (ctx->keep_pool[(size_t)idx]->pin.ensure(len) != FABGPU_OK) {
        std::lock_guard<std::mutex> lk(ctx->keep_mu);
        ctx->keep_pool[(size_t)idx]->in_use = false;
        ctx->keep_refused++;
        return -1;
    }
    return idx;
}

static int arena_stage_impl(fabgpu_ctx* ctx, const void* arena, size_t len, uint64_t* token, fab::HostCopy* keep);

extern "C" int fabgpu_arena_stage(fabgpu_ctx* ctx, const void* arena, size_t len, uint64_t* token) { return arena_stage_impl(ctx, arena, len, token, nullptr); }
namespace fab {
int arena_stage_keep(fabgpu_ctx* ctx, const void* arena, size_t len, uint64_t* token, HostCopy* keep) {
    if (keep) *keep = HostCopy();
    return arena_stage_impl(ctx, arena, len, token, keep);
}
}  // namespace fab

static int arena_stage_impl(fabgpu_ctx* ctx, const void* arena, size_t len, uint64_t* token, fab::HostCopy* keep) {
    if (!ctx || !arena || !token || len == 0) return FABGPU_EINVAL;
    if (len > 0xFFFFFF00ull) return FABGPU_ETOOBIG;
    // the least recently filled slot nobody is using; all in use: wait for the oldest
    fabgpu_ctx::Staged* sl = nullptr;
    std::unique_lock<std::mutex> slot_lk;
    {
        std::lock_guard<std::mutex> lk(ctx->smu);
        int order[fabgpu_ctx::N_STAGED];
        for (int i = 0; i < fabgpu_ctx::N_STAGED; i++) order[i] = i;
        std::sort(order, order + fabgpu_ctx::N_STAGED, [&](int x, int y) { return ctx->staged_slots[x].token.load() < ctx->staged_slots[y].token.load(); });
        for (int i = 0; i < fabgpu_ctx::N_STAGED && !sl; i++) {
            std::unique_lock<std::mutex> t(ctx->staged_slots[order[i]].m, std::try_to_lock);
            if (t.owns_lock()) {
                sl = &ctx->staged_slots[order[i]];
                slot_lk = std::move(t);
            }
        }
        if (!sl) sl = &ctx->staged_slots[order[0]];
    }
    if (!slot_lk.owns_lock()) slot_lk = std::unique_lock<std::mutex>(sl->m);
    DeviceGuard g(ctx->device);
    // the caller keeps a host copy: the bytes go through a pool buffer that is then his (whatever the arena's size)
    const int keep_idx = keep ? keep_acquire(ctx, len) : -1;
    struct KeepBack {                                      // an early exit hands the buffer back
        fabgpu_ctx* c;
        int idx;
        ~KeepBack() {
            if (idx < 0) return;
            std::lock_guard<std::mutex> lk(c->keep_mu);
            c->keep_pool[(size_t)idx]->in_use = false;
        }
    } keep_back{ctx, keep_idx};
    uint8_t* const keep_pin = keep_idx >= 0 ? (uint8_t*)ctx->keep_pool[(size_t)keep_idx]->pin.h : nullptr;
    const size_t need = round_up(len, 64) + 128;          // + room for a batch's tail (fabgpu_identity_batch.tail) in the slack below
    sl->token.store(0);                                    // the previous upload is gone from here on
    sl->len = 0;
    if (sl->cap < need + (64 << 10)) {                     // (a batch reading the old buffer would hold the slot's mutex)
        if (sl->d) hipFree(sl->d);
        sl->d = nullptr;
        sl->cap = 0;
        if (hipMalloc(&sl->d, need + need / 8 + (64 << 10)) != hipSuccess) return FABGPU_ENOMEM;
        sl->cap = need + need / 8 + (64 << 10);
    }
    // A block arrives in memory the runtime has never seen (a peer's blocks are fresh allocations): a pageable hipMemcpy of such
    // memory spends more time making the pages DMA-able than moving them - 50 MB took 2.0-2.5 ms against 0.9 ms for a buffer that was
    // sent before, which the runtime keeps pinned (tools/gpu_probe_fresh_buffers.py).  Arenas of 4 MiB and more therefore travel
    // through a pinned staging buffer the context owns: a few threads copy 2 MiB pieces into it and queue each piece's DMA as soon as
    // it is there (four copiers): 2.2 ms per 10 000-transaction pass whatever the
    // buffer's history, against 2.9-3.9 ms (fresh) / 1.85 ms (re-sent, which a peer never does) on the pageable path.  Splitting the pageable copy itself over threads
    // was measured too: slower than one call (the pinning serialises in the driver).
    static const bool stage_timing = getenv("FABGPU_PASS_TIMING") != nullptr;
    const auto stage_t0 = std::chrono::steady_clock::now();
    constexpr int stage_threads = 4;             // measured from 0 (the runtime's pageable path) to 16 in rounds 2-3; no difference from two up
    hipError_t err = hipSuccess;
    if (stage_threads == 0 || len < ((size_t)4 << 20)) {
        if (keep_pin) {                                                    // a small arena somebody keeps: one copy, then the DMA from pinned memory
            memcpy(keep_pin, arena, len);
            err = hipMemcpy(sl->d, keep_pin, len, hipMemcpyHostToDevice);
        } else {
            err = hipMemcpy(sl->d, arena, len, hipMemcpyHostToDevice);
        }
    } else {
        std::lock_guard<std::mutex> plk(ctx->stage_pin_mu);              // one upload at a time per device: uploads share the bus anyway
        if (ctx->fault == 2 || (!keep_pin && ctx->stage_pin.ensure(len) != FABGPU_OK)) return FABGPU_ENOMEM;
        // pieces: 256 KiB, 512 KiB, 1 MiB, then 2 MiB each - the first DMA starts after 25 us of copying instead of 200
        std::vector<size_t> cut;
        constexpr size_t max_piece = (size_t)2048 << 10;
        for (size_t at = 0, sz = (size_t)256 << 10; at < len; at += sz, sz = std::min(sz * 2, max_piece)) cut.push_back(at);
        cut.push_back(len);
        const size_t n_pieces = cut.size() - 1;
        std::atomic<size_t> next(0);
        std::unique_ptr<std::atomic<uint8_t>[]> done(new std::atomic<uint8_t>[n_pieces]);
        for (size_t k = 0; k < n_pieces; k++) done[k].store(0, std::memory_order_relaxed);
        int failed = 0;
        uint8_t* dst = (uint8_t*)sl->d;
        uint8_t* pin = keep_pin ? keep_pin : (uint8_t*)ctx->stage_pin.h;
        const uint8_t* src = (const uint8_t*)arena;
        // Pieces go round-robin over four upload queues so that one piece's set-up overlaps another's transfer:
        // measured (round 3, 48.6 MB) 1.33 ms with one queue, 1.23 with two, 1.13 with four - 43 GB/s; the
        // number of copier threads makes no difference from two up.
        constexpr int n_queues = 4;
        hipStream_t cs[4] = {ctx->stream_copy, ctx->stream_copy_more[0], ctx->stream_copy_more[1], ctx->stream_copy_more[2]};
        const int dev = ctx->device;
        // The copiers (the host side's worker pool: idle while a block travels) claim pieces in order; this thread queues a piece's DMA
        // as soon as it is in the staging buffer - it alone talks to the runtime (several threads queueing on one stream spend their
        // time on its lock) - and copies pieces itself while it has nothing to queue.
        auto copy_one = [&]() -> bool {
            const size_t k = next.fetch_add(1, std::memory_order_relaxed);
            if (k >= n_pieces) return false;
            memcpy(pin + cut[k], src + cut[k], cut[k + 1] - cut[k]);
            done[k].store(1, std::memory_order_release);
            return true;
        };
        const int nth = (int)std::min<size_t>((size_t)stage_threads, n_pieces);
        if (!ctx->stage_pool) ctx->stage_pool.reset(new (std::nothrow) WorkerPool(stage_threads));   // (stage_pin_mu is held)
        run_workers(nth + 1, [&](int w) {
            if (w != 0) {
                while (copy_one()) {}
                return;
            }
            hipSetDevice(dev);
            for (size_t k = 0; k < n_pieces; k++) {
                while (!done[k].load(std::memory_order_acquire))
                    if (!copy_one()) std::this_thread::yield();
                if (hipMemcpyAsync(dst + cut[k], pin + cut[k], cut[k + 1] - cut[k], hipMemcpyHostToDevice, cs[k % (size_t)n_queues]) != hipSuccess) failed = 1;
            }
        }, ctx->stage_pool.get());
        for (int q = 0; q < n_queues; q++) {
            const hipError_t e = hipStreamSynchronize(cs[q]);
            if (err == hipSuccess) err = e;
        }
        if (err == hipSuccess && failed) err = hipErrorUnknown;
    }
    if (err == hipSuccess) err = hipMemset((uint8_t*)sl->d + len, 0, need - len);
    if (err != hipSuccess) return hip_to_rc(err);
    if (stage_timing)
        fprintf(stderr, "fabgpu arena stage: %.1f MB in %.2f ms\n", len / 1e6, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - stage_t0).count());
    sl->len = len;
    uint64_t t;
    {
        std::lock_guard<std::mutex> lk(ctx->smu);
        t = ++ctx->stage_seq;
    }
    sl->token.store(t);
    *token = t;
    if (keep && keep_idx >= 0) {
        keep->ctx = ctx;
        keep->idx = keep_idx;
        keep->p = keep_pin;
        keep->len = len;
        keep_back.idx = -1;                                // (the caller's now: host_copy_release)
    }
    return FABGPU_OK;
}

// What a DESCRIBED batch stages on top of HostStage (fabgpu_identity_verify_batch and the P-384 entries): the staged upload it may name, the
// bytes of the caller's arena its plan references (described_plan.h), the rebased offsets in ctx->offs, pre_off | pre_idx | mid-state
// room in ctx->pre, and ctx->out as verdict words | status bytes | digest rows.  Every step from the first upload on is skipped once
// rc is set, and the entry leaves through drain(): HostStage's failure rule, with ctx->stream2 drained too where it carries work (side).
struct DescribedStage : HostStage {
    const uint32_t m;                    // prefixes
    const bool spans;
    const size_t noff, npre;             // u32 values of off and of pre_off
    const size_t ib, pob, dg_off;        // bytes of n u32 padded to 64; of pre_off likewise; where the digest rows start in ctx->out
    fabgpu_ctx::Staged* sl = nullptr;    // the staged upload, or nullptr: the arena is the caller's
    std::unique_lock<std::mutex> slk;    // its slot stays locked - the stager kept out of it - until this batch has run
    bool side = false;                   // ctx->stream2 carries work of this call

    DescribedStage(fabgpu_ctx* c, size_t rows, size_t field_bytes, uint32_t prefixes, bool pairs)
        : HostStage(c, rows, false, field_bytes), m(prefixes), spans(pairs), noff(pairs ? 2 * rows : rows + 1),
          npre(prefixes ? (pairs ? 2 * (size_t)prefixes : (size_t)prefixes + 1) : 0), ib(round_up(rows * 4, 64)),
          pob(round_up((npre + 1) * 4, 64)), dg_off(round_up(st_off + rows, 64)) {}
    // FABGPU_IDB_ARENA_STAGED, before ctx->mu is taken: find the upload and lock its slot
    int slot(uint64_t token) {
        rc = FABGPU_EINVAL;
        if (token == 0) return rc;
        for (auto& c : ctx->staged_slots)
            if (c.token.load() == token) sl = &c;
        if (!sl) return rc;                                                                     // replaced meanwhile
        slk = std::unique_lock<std::mutex>(sl->m);
        if (sl->token.load() == token && sl->len != 0) rc = FABGPU_OK;                          // ... or just now
        return rc;
    }
    // the closed plan against what holds the arena
    int bind(DescribedPlan& p, const uint8_t* arena) {
        if (sl) {
            if (p.hi > sl->len) return rc = FABGPU_EINVAL;
            p.absolute();
        } else if (p.span() && !arena) {
            return rc = FABGPU_EINVAL;
        }
        return FABGPU_OK;
    }
    // small arenas go through the pinned staging buffer; big ones (a marshalled block) are handed to the driver directly - one copy less
    // on the host, the slack the kernels may touch zeroed on the device
    bool direct(const DescribedPlan& p) const { return !sl && p.span() >= ((size_t)4 << 20); }
    int rooms(size_t arena_room, size_t mid_bytes, size_t tail_room, size_t out_room) {
        if ((!sl && (rc = room(ctx->arena, arena_room))) || (rc = room(ctx->offs, noff * 4)) || (m && (rc = room(ctx->pre, pob + ib + (size_t)m * mid_bytes + 64))) ||
            (tail_room && (rc = room(ctx->tailbuf, tail_room))))
            return rc;
        return rc = room(ctx->out, out_room);
    }
    // the referenced bytes of the caller's arena and zeros up to ab; tail_in_arena (or nullptr): the tail, laid at tail_base into the
    // pinned copy - a direct upload leaves it to upload_tail.  A staged upload is already there.
    void upload_arena(const DescribedPlan& p, const uint8_t* arena, size_t ab, const void* tail_in_arena) {
        if (rc != FABGPU_OK || sl) return;
        const size_t span = p.span();
        hipError_t err;
        if (direct(p)) {
            err = hipMemcpyAsync(ctx->arena.d, arena + p.lo, span, hipMemcpyHostToDevice, ctx->stream);
            if (err == hipSuccess) err = hipMemsetAsync((uint8_t*)ctx->arena.d + span, 0, ab - span, ctx->stream);
        } else {
            if (span) memcpy(ctx->arena.h, arena + p.lo, span);
            memset((uint8_t*)ctx->arena.h + span, 0, ab - span);
            if (tail_in_arena) memcpy((uint8_t*)ctx->arena.h + (p.tail_base - p.lo), tail_in_arena, p.tail_len);
            err = hipMemcpyAsync(ctx->arena.d, ctx->arena.h, ab, hipMemcpyHostToDevice, ctx->stream);
        }
        rc = hip_to_rc(err);
    }
    // the tail through its own pinned staging: its bytes and zeros up to `bytes`, to dst
    void upload_tail(const DescribedPlan& p, const void* tail, void* dst, size_t bytes) {
        if (rc != FABGPU_OK) return;
        memcpy(ctx->tailbuf.h, tail, p.tail_len);
        memset((uint8_t*)ctx->tailbuf.h + p.tail_len, 0, bytes - p.tail_len);
        rc = hip_to_rc(hipMemcpyAsync(dst, ctx->tailbuf.h, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    void upload_offsets(const DescribedPlan& p, const uint32_t* off, const uint32_t* pre_off, const uint32_t* pre_idx) {
        if (rc != FABGPU_OK) return;
        p.rebase((uint32_t*)ctx->offs.h, off, noff, spans);
        hipError_t err = hipMemcpyAsync(ctx->offs.d, ctx->offs.h, noff * 4, hipMemcpyHostToDevice, ctx->stream);
        if (m) {
            p.rebase((uint32_t*)ctx->pre.h, pre_off, npre, spans);
            memcpy((uint8_t*)ctx->pre.h + pob, pre_idx, n * 4);
            if (err == hipSuccess) err = hipMemcpyAsync(ctx->pre.d, ctx->pre.h, pob + ib, hipMemcpyHostToDevice, ctx->stream);
        }
        rc = hip_to_rc(err);
    }
    void* mid() const { return m ? (uint8_t*)ctx->pre.d + pob + ib : nullptr; }
    // the device-side batch: what was staged here (fields() has run); arena, tail, flags and digests are the entry's
    template <class Batch> void describe(Batch& d, bool keyed, bool want_status) const {
        d.off = (const uint32_t*)ctx->offs.d;
        d.n_prefixes = m;
        d.pre_off = m ? (const uint32_t*)ctx->pre.d : nullptr;
        d.pre_idx = m ? (const uint32_t*)((uint8_t*)ctx->pre.d + pob) : nullptr;
        d.key_id = keyed ? (const uint32_t*)ids() : nullptr;
        d.qx = keyed ? nullptr : field(0);
        d.qy = keyed ? nullptr : field(1);
        d.r = field(keyed ? 0 : 2);
        d.s = field(keyed ? 1 : 3);
        d.verdict_bits = ctx->out.d;
        d.status = want_status ? (uint8_t*)ctx->out.d + st_off : nullptr;
    }
    void download_results(const void* status, const void* digests) { download(digests ? dg_off + n * 32 : (status ? st_off + n : words * 8)); }
    int drain() {
        HostStage::drain();
        const hipError_t drained = side ? hipStreamSynchronize(ctx->stream2) : hipSuccess;
        if (rc == FABGPU_OK) rc = hip_to_rc(drained);
        return rc;
    }
    void copy_out(void* verdict_bits, void* status, void* digests) const {
        memcpy(verdict_bits, ctx->out.h, words * 8);
        if (status) memcpy(status, (uint8_t*)ctx->out.h + st_off, n);
        if (digests) memcpy(digests, (uint8_t*)ctx->out.h + dg_off, n * 32);
    }
};

extern "C" {

int fabgpu_identity_verify_batch(fabgpu_ctx* ctx, const fabgpu_identity_batch* b) {
    if (!ctx || !b) return FABGPU_EINVAL;
    const size_t n = b->n;
    if (n == 0) return FABGPU_OK;
    const bool keyed = b->key_id != nullptr;
    const uint32_t m = (b->n_prefixes != 0 && b->pre_idx != nullptr) ? b->n_prefixes : 0;
    if (!b->off || !b->r || !b->s || !b->verdict_bits || (!keyed && (!b->qx || !b->qy)) || (m && !b->pre_off)) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 160) return FABGPU_ETOOBIG;
    const uint8_t* arena = (const uint8_t*)b->arena;
    const bool spans = (b->flags & FABGPU_IDB_SPANS) != 0;
    const bool staged = (b->flags & FABGPU_IDB_ARENA_STAGED) != 0;
    if (b->flags & ~(uint32_t)(FABGPU_IDB_SPANS | FABGPU_IDB_ARENA_STAGED | FABGPU_IDB_SHA3_256)) return FABGPU_EINVAL;
    const size_t mid_bytes = (b->flags & FABGPU_IDB_SHA3_256) ? 200 : 32;   // a SHA3-256 mid-state is the whole Keccak state
    const size_t nn = b->n_nym;            // pseudonym signatures over the same arena, on the second stream
    if (nn && (!spans || !b->nym_off || !b->nym_issuer || !b->nym_fields || !b->nym_verdict_bits)) return FABGPU_EINVAL;
    if (nn > 0x7FFFFFF0ull / 200) return FABGPU_ETOOBIG;
    const uint32_t ng = b->n_gather;
    if (ng && (!b->gather_spans || !b->gather_digests)) return FABGPU_EINVAL;
    DescribedStage h(ctx, n, 32, m, spans);
    if (staged && h.slot(b->stage_token)) return h.rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    // the tail is written into the device arena at tail_base
    DescribedPlan p(DescribedPlan::IN_ARENA, spans, b->tail, b->tail_base, b->tail_len);
    p.see_rows(b->off, n, true);
    p.see_rows(b->nym_off, nn, true);
    p.see_rows(b->pre_off, m, false);                      // prefixes never lie in the tail
    p.see_gather(b->gather_spans, (size_t)ng * 3);
    if (p.close() || h.bind(p, arena)) return p.rc ? p.rc : h.rc;
    const size_t tbase = p.tail_base, tlen = p.tail_len;
    if (staged && p.tail_used && (tbase < round_up(h.sl->len, 64) || tbase + tlen + 128 > h.sl->cap)) return FABGPU_EINVAL;
    // extent of the device arena: the caller's bytes, then (if used) zero padding up to tail_base and the tail
    const size_t held = staged ? h.sl->len : p.span(), extent = p.tail_used ? tbase - p.lo + tlen : held, ab = round_up(extent, 4) + 64;
    const bool apart = p.tail_used && (staged || h.direct(p));   // the tail travels through its own pinned staging
    const size_t gsb = round_up((size_t)ng * 24, 64), gob = round_up(((size_t)ng + 1) * 4, 64), gscr = round_up((size_t)p.gather_total, 4) + 64;
    const size_t nkb = round_up(nn * 4, 64), nfb = nn * 32, nwords = (nn + 63) / 64, nst_off = round_up(nwords * 8, 64);
    if (h.rooms(ab + 64, mid_bytes, apart ? tlen : 0, h.dg_off + (b->digests ? h.fb : 0)) ||
        (ng && ((h.rc = h.room(ctx->gath, gsb + gob + (size_t)ng * 32)) || (h.rc = h.room(ctx->gscr, gscr)))) ||
        (nn && ((h.rc = h.room(ctx->nym, nkb + 6 * nfb + nn * 8)) || (h.rc = h.room(ctx->nymout, nst_off + nn)))))
        return h.rc;
    h.side = nn != 0;
    uint8_t* darena = (uint8_t*)(staged ? h.sl->d : ctx->arena.d);
    h.upload_arena(p, arena, ab, p.tail_used ? b->tail : nullptr);
    if (apart) {                                           // a staged upload gets 128 zero bytes behind the tail
        h.upload_tail(p, b->tail, darena + (tbase - p.lo), tlen);
        if (staged && h.rc == FABGPU_OK) h.rc = hip_to_rc(hipMemsetAsync(darena + tbase + tlen, 0, 128, ctx->stream));
    }
    h.upload_offsets(p, b->off, b->pre_off, b->pre_idx);
    if (keyed) h.fields(ctx->fields, HostStage::ID_COLUMN, b->key_id, {(const uint8_t*)b->r, (const uint8_t*)b->s});
    else h.fields(ctx->fields, 0, nullptr, {(const uint8_t*)b->qx, (const uint8_t*)b->qy, (const uint8_t*)b->r, (const uint8_t*)b->s});
    fabgpu_identity_batch d = *b;
    h.describe(d, keyed, b->status != nullptr);
    d.flags = b->flags & (FABGPU_IDB_SPANS | FABGPU_IDB_SHA3_256);
    d.arena = darena;
    d.arena_bytes = staged ? round_up(p.tail_used ? tbase + tlen : held, 4) + 64 : ab;
    d.tail = nullptr;
    d.tail_base = d.tail_len = 0;
    d.digests = b->digests ? (uint8_t*)ctx->out.d + h.dg_off : nullptr;
    uint8_t* gd = (uint8_t*)ctx->gath.d;
    if (ng && h.rc == FABGPU_OK) {
        uint32_t* go = (uint32_t*)((uint8_t*)ctx->gath.h + gsb);
        p.rebase((uint32_t*)ctx->gath.h, b->gather_spans, (size_t)ng * 6, true);
        uint32_t run = 0;
        for (uint32_t j = 0; j < ng; j++) {
            go[j] = run;
            for (int k = 0; k < 3; k++) run += b->gather_spans[6 * (size_t)j + 2 * k + 1] - b->gather_spans[6 * (size_t)j + 2 * k];
        }
        go[ng] = run;
        h.rc = hip_to_rc(hipMemcpyAsync(gd, ctx->gath.h, gsb + gob, hipMemcpyHostToDevice, ctx->stream));
        d.gather_spans = (const uint32_t*)gd;
        d.gather_off = (const uint32_t*)(gd + gsb);
        d.gather_digests = gd + gsb + gob;
        d.gather_scratch = ctx->gscr.d;
        d.gather_scratch_bytes = gscr;
    }
    // the pseudonym signatures: staged and launched on the second stream BEFORE the ECDSA kernels are queued, so that the two run
    // side by side (a block's idemix creators are a latency-bound launch of their own: bn_quad29.h)
    uint8_t* nd = (uint8_t*)ctx->nym.d;
    uint8_t* nout = (uint8_t*)ctx->nymout.d;
    if (nn && h.rc == FABGPU_OK) {
        uint8_t* nh = (uint8_t*)ctx->nym.h;
        memcpy(nh, b->nym_issuer, nn * 4);
        memcpy(nh + nkb, b->nym_fields, 6 * nfb);
        p.rebase((uint32_t*)(nh + nkb + 6 * nfb), b->nym_off, 2 * nn, true);
        hipError_t err = hipEventRecord(ctx->ev_up, ctx->stream);            // arena (and tail) uploads are queued on `stream`
        if (err == hipSuccess) err = hipStreamWaitEvent(ctx->stream2, ctx->ev_up, 0);
        if (err == hipSuccess) err = hipMemcpyAsync(nd, nh, nkb + 6 * nfb + nn * 8, hipMemcpyHostToDevice, ctx->stream2);
        if ((h.rc = hip_to_rc(err)) == FABGPU_OK)
            h.rc = nym_verify_dev(ctx, nn, d.arena, d.arena_bytes, nd + nkb + 6 * nfb, true, nd, nd + nkb, nd + nkb + nfb, nd + nkb + 2 * nfb, nd + nkb + 3 * nfb,
                                  nd + nkb + 4 * nfb, nd + nkb + 5 * nfb, nout, b->nym_status ? nout + nst_off : nullptr, ctx->stream2, false);
        if (h.rc == FABGPU_OK)
            h.rc = hip_to_rc(hipMemcpyAsync(ctx->nymout.h, nout, b->nym_status ? nst_off + nn : nwords * 8, hipMemcpyDeviceToHost, ctx->stream2));
    }
    if (h.rc == FABGPU_OK) h.rc = fabgpu_identity_verify_batch_dev(ctx, &d, h.mid(), ctx->stream);
    h.download_results(b->status, b->digests);
    if (ng && h.rc == FABGPU_OK)
        h.rc = hip_to_rc(hipMemcpyAsync((uint8_t*)ctx->gath.h + gsb + gob, gd + gsb + gob, (size_t)ng * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (h.drain()) return h.rc;                            // nothing of this call is running any more, nothing was copied out
    h.copy_out(b->verdict_bits, b->status, b->digests);
    if (ng) memcpy(b->gather_digests, (uint8_t*)ctx->gath.h + gsb + gob, (size_t)ng * 32);
    if (nn) {
        memcpy(b->nym_verdict_bits, ctx->nymout.h, nwords * 8);
        if (b->nym_status) memcpy(b->nym_status, (uint8_t*)ctx->nymout.h + nst_off, nn);
    }
    return FABGPU_OK;
}

// ---- identity.Verify over a described batch of P-384 identities: the digest rows (p384_described_kernels.hip; for the _sha3 entries
// p384_described_sha3_kernels.hip), then the fresh or the keyed P-384 kernel over them on the same stream.  One body per form, the hash
// family a parameter: the flags a caller may pass are the same for both families (FABGPU_IDB_SHA3_256 is not among them) ------------
static int identity_verify_batch_p384_dev(fabgpu_ctx* ctx, const fabgpu_identity_batch_p384* b, void* mid_scratch, void* stream, bool sha3) {
    if (!ctx || !b) return FABGPU_EINVAL;
    const size_t n = b->n;
    const bool keyed = b->key_id != nullptr;
    DeviceGuard g(ctx->device);
    if (n == 0) return keyed ? p384_gcomb(ctx) : p384_gtab(ctx);      // the explicit warm call (fabgpu.h): a table, no launch
    const bool prefixed = b->n_prefixes != 0 && b->pre_idx != nullptr;
    if (!b->arena || !b->off || !b->r || !b->s || !b->verdict_bits || (!keyed && (!b->qx || !b->qy))) return FABGPU_EINVAL;
    if (prefixed && (!b->pre_off || !mid_scratch)) return FABGPU_EINVAL;
    if (b->flags & ~(uint32_t)FABGPU_IDB_SPANS) return FABGPU_EINVAL;   // (FABGPU_IDB_SHA3_256 among them: the family is the entry's)
    if (sha3 && prefixed && ((uintptr_t)mid_scratch & 7u)) return FABGPU_EINVAL;   // (mid_scratch: 200 bytes a prefix)
    if (dev_too_big(n, b->arena_bytes)) return FABGPU_ETOOBIG;
    const bool has_tail = b->tail != nullptr && b->tail_len != 0;
    if (has_tail && (!(b->flags & FABGPU_IDB_SPANS) || (b->tail_base & 63u) || (uint64_t)b->tail_base + b->tail_len > 0xFFFFFFF0ull)) return FABGPU_EINVAL;
    if (b->arena_bytes < 4 || (b->arena_bytes & 3u) || ((uintptr_t)b->arena & 3u) || (has_tail && ((uintptr_t)b->tail & 3u))) return FABGPU_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    size_t di = 0;
    void* dig = b->digests;
    if (!dig) {
        const int rc = ctx->acquire_qws(n * 32, &di, &dig, st);
        if (rc != FABGPU_OK) return rc;
    }
    P384DescribedLaunch v;
    v.n = (uint32_t)n;
    v.arena = b->arena; v.arena_bytes = b->arena_bytes; v.off = b->off;
    v.pa.spans = (b->flags & FABGPU_IDB_SPANS) != 0;
    if (prefixed) {
        v.pa.m = b->n_prefixes;
        v.pa.pre_off = b->pre_off;
        v.pa.pre_idx = b->pre_idx;
        v.pa.mid_scratch = mid_scratch;
    }
    if (has_tail) {
        v.tail = b->tail; v.tail_base = b->tail_base; v.tail_len = b->tail_len;
    }
    v.digests = dig;
    int rc = timed_launch(ctx, st, 0, [&](void*) { return sha3 ? launch_p384_described_sha3_digests(v, st) : launch_p384_described_digests(v, st); });
    if (rc == FABGPU_OK)
        rc = keyed ? p384_verify_keyed_dev(ctx, n, b->key_id, dig, true, b->r, b->s, b->verdict_bits, b->status, st)
                   : p384_verify_dev(ctx, n, b->qx, b->qy, dig, true, b->r, b->s, b->verdict_bits, b->status, st);
    if (!b->digests) ctx->release_qws(di, st);
    return rc;
}

static int identity_verify_batch_p384_host(fabgpu_ctx* ctx, const fabgpu_identity_batch_p384* b, bool sha3) {
    if (!ctx || !b) return FABGPU_EINVAL;
    const size_t n = b->n;
    const bool keyed = b->key_id != nullptr;
    if (n == 0) return identity_verify_batch_p384_dev(ctx, b, nullptr, nullptr, sha3);
    const uint32_t m = (b->n_prefixes != 0 && b->pre_idx != nullptr) ? b->n_prefixes : 0;
    if (!b->off || !b->r || !b->s || !b->verdict_bits || (!keyed && (!b->qx || !b->qy)) || (m && !b->pre_off)) return FABGPU_EINVAL;
    if (n > 0x7FFFFFF0ull / 240) return FABGPU_ETOOBIG;
    const uint8_t* arena = (const uint8_t*)b->arena;
    const bool spans = (b->flags & FABGPU_IDB_SPANS) != 0;
    const bool staged = (b->flags & FABGPU_IDB_ARENA_STAGED) != 0;
    if (b->flags & ~(uint32_t)(FABGPU_IDB_SPANS | FABGPU_IDB_ARENA_STAGED)) return FABGPU_EINVAL;   // (FABGPU_IDB_SHA3_256: the family is the entry's)
    const size_t mid_bytes = sha3 ? SHA3_MID_BYTES_HOST : 32;   // a SHA3-256 mid-state is the whole Keccak state
    DescribedStage h(ctx, n, 48, m, spans);
    if (staged && h.slot(b->stage_token)) return h.rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    DescribedPlan p(DescribedPlan::OWN_BUFFER, spans, b->tail, b->tail_base, b->tail_len);
    p.see_rows(b->off, n, true);
    p.see_rows(b->pre_off, m, false);                      // prefixes never lie in the tail
    if (p.close() || h.bind(p, arena)) return p.rc ? p.rc : h.rc;
    // the device arena: the staged upload as it lies there (fabgpu_arena_stage zeroed its slack up to the next 64 and beyond), or the
    // referenced bytes of the caller's arena; the tail in a buffer of its own either way, so a staged upload is read and never written
    const size_t ab = staged ? round_up(h.sl->len, 64) : round_up(p.span(), 4) + 64, tb = round_up((size_t)p.tail_len, 4);
    if (h.rooms(ab, mid_bytes, p.tail_used ? tb + 64 : 0, h.dg_off + n * 32)) return h.rc;
    h.upload_arena(p, arena, ab, nullptr);
    if (p.tail_used) h.upload_tail(p, b->tail, ctx->tailbuf.d, tb + 64);
    h.upload_offsets(p, b->off, b->pre_off, b->pre_idx);
    if (keyed) h.fields(ctx->keyed, HostStage::ID_COLUMN, b->key_id, {(const uint8_t*)b->r, (const uint8_t*)b->s});
    else h.fields(ctx->fields, 0, nullptr, {(const uint8_t*)b->qx, (const uint8_t*)b->qy, (const uint8_t*)b->r, (const uint8_t*)b->s});
    fabgpu_identity_batch_p384 d = *b;
    h.describe(d, keyed, b->status != nullptr);
    d.flags = b->flags & FABGPU_IDB_SPANS;
    d.arena = staged ? h.sl->d : ctx->arena.d;
    d.arena_bytes = ab;
    d.tail = p.tail_used ? ctx->tailbuf.d : nullptr;
    d.tail_base = p.tail_used ? p.tail_base : 0;
    d.tail_len = p.tail_used ? p.tail_len : 0;
    d.digests = (uint8_t*)ctx->out.d + h.dg_off;           // (the rows the verify kernel reads: made here whether the caller wants them or not)
    if (h.rc == FABGPU_OK) h.rc = identity_verify_batch_p384_dev(ctx, &d, h.mid(), ctx->stream, sha3);
    h.download_results(b->status, b->digests);
    if (h.drain()) return h.rc;
    h.copy_out(b->verdict_bits, b->status, b->digests);
    return FABGPU_OK;
}

int fabgpu_identity_verify_batch_p384_dev(fabgpu_ctx* ctx, const fabgpu_identity_batch_p384* b, void* mid_scratch, void* stream) {
    return identity_verify_batch_p384_dev(ctx, b, mid_scratch, stream, false);
}
int fabgpu_identity_verify_batch_p384(fabgpu_ctx* ctx, const fabgpu_identity_batch_p384* b) { return identity_verify_batch_p384_host(ctx, b, false); }
// the same two for the batch of an MSP of the SHA3 hash family: SHA3-256 digest rows, 200 bytes of mid-state a prefix
int fabgpu_identity_verify_batch_p384_sha3_dev(fabgpu_ctx* ctx, const fabgpu_identity_batch_p384* b, void* mid_scratch, void* stream) {
    return identity_verify_batch_p384_dev(ctx, b, mid_scratch, stream, true);
}
int fabgpu_identity_verify_batch_p384_sha3(fabgpu_ctx* ctx, const fabgpu_identity_batch_p384* b) { return identity_verify_batch_p384_host(ctx, b, true); }

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// the block pass on the device (block_walk_dev.h)
// ------------------------------------------------------------------------------------------------
namespace fab {

int walk_idtab_set(fabgpu_ctx* ctx, uint32_t n, const DevIdEntry* entries, const uint8_t* bytes, size_t nbytes, uint64_t seed) {
    if (!ctx || (n && (!entries || !bytes))) return FABGPU_EINVAL;
    if (n > (1u << 20) || nbytes > 0x7FFFFFF0ull) return FABGPU_ETOOBIG;
    uint32_t cap = 16;
    while (cap < 2 * n) cap <<= 1;
    std::vector<uint32_t> slots(cap, 0);
    for (uint32_t i = 0; i < n; i++) {
        if ((uint64_t)entries[i].off + entries[i].len > nbytes) return FABGPU_EINVAL;
        uint32_t at = (uint32_t)entries[i].hash & (cap - 1), d = 0;
        while (slots[at] && d < bccsp::walk::WALK_ID_PROBE_MAX) {
            at = (at + 1) & (cap - 1);
            d++;
        }
        if (d < bccsp::walk::WALK_ID_PROBE_MAX) slots[at] = i + 1;     // (else: left out - the lookup would not walk that far either)
    }
    const size_t eo = round_up((size_t)cap * 4, 256), bo = round_up(eo + (size_t)n * sizeof(DevIdEntry), 256), total = bo + round_up(nbytes, 64) + 64;
    // The table lives in ONE grow-only allocation that is overwritten in place (it used to be a fresh hipMalloc per version with a
    // hipFree of the old one: a provider whose cache changes with every block - new clients - paid both before every pass).
    std::lock_guard<std::mutex> lk(ctx->mu);             // no pass is in flight while mu is held (a pass synchronises before it returns)
    DeviceGuard g(ctx->device);
    if (ctx->fault == 2) return FABGPU_ENOMEM;
    int rc = ctx->idtab_buf.ensure(total);
    if (rc != FABGPU_OK) return rc;
    void* d = ctx->idtab_buf.d;
    hipError_t err = hipMemcpy(d, slots.data(), (size_t)cap * 4, hipMemcpyHostToDevice);
    if (err == hipSuccess && n) err = hipMemcpy((uint8_t*)d + eo, entries, (size_t)n * sizeof(DevIdEntry), hipMemcpyHostToDevice);
    if (err == hipSuccess && nbytes) err = hipMemcpy((uint8_t*)d + bo, bytes, nbytes, hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        ctx->d_idtab = nullptr;                          // (half-written: the device treats everybody as unknown until the next table)
        ctx->idtab_n = 0;
        ctx->idtab_mask = 0;
        return hip_to_rc(err);
    }
    // The verify launches of a pass are queued on a prediction of "every tuple of this class has a key table" (pred_keyed_*: what held for
    // the previous block).  A table whose every P-256 identity HAS a key table is better evidence than the previous block: the second
    // pass of a fresh provider - identities learned and registered during the first - used to run on the fresh-key kernels once more
    // (2.9 ms instead of 2.0; profiles/r05_fresh_provider_probe.txt).  A wrong "keyed" guess only costs the relaunch of that class.
    {
        bool any = false, all = true;
        for (uint32_t i = 0; i < n; i++)
            if (entries[i].p256) {
                any = true;
                all = all && entries[i].key_id >= 0;
            }
        if (any && all) ctx->pred_keyed_creators = ctx->pred_keyed_others = true;
    }
    ctx->d_idtab = d;
    ctx->idtab_n = n;
    ctx->idtab_mask = cap - 1;
    ctx->idtab_seed = seed;
    ctx->idtab_entries_off = eo;
    ctx->idtab_bytes_off = bo;
    return FABGPU_OK;
}

// TEST HOOK: the wavefront signature gate of the device walk over n signatures held in host memory
int walk_gate_probe(fabgpu_ctx* ctx, uint32_t n, const uint8_t* arena, size_t arena_len, const uint32_t* spans, uint8_t* code, uint8_t* r, uint8_t* s_out) {
    if (!ctx || (n && (!arena || !spans || !code || !r || !s_out))) return FABGPU_EINVAL;
    if (n == 0) return FABGPU_OK;
    for (uint32_t i = 0; i < n; i++)
        if (spans[2 * i + 1] < spans[2 * i] || spans[2 * i + 1] > arena_len) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    void *da = nullptr, *ds = nullptr, *dout = nullptr;
    int rc = FABGPU_ENOMEM;
    if (hipMalloc(&da, arena_len + 256) == hipSuccess && hipMalloc(&ds, (size_t)n * 8) == hipSuccess && hipMalloc(&dout, (size_t)n * 65) == hipSuccess) {
        hipError_t e = hipMemcpy(da, arena, arena_len, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(ds, spans, (size_t)n * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = launch_walk_gate_probe(n, da, ds, (uint8_t*)dout + (size_t)n * 64, dout, (uint8_t*)dout + (size_t)n * 32, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpy(r, dout, (size_t)n * 32, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(s_out, (uint8_t*)dout + (size_t)n * 32, (size_t)n * 32, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(code, (uint8_t*)dout + (size_t)n * 64, n, hipMemcpyDeviceToHost);
        rc = hip_to_rc(e);
    }
    if (da) hipFree(da);
    if (ds) hipFree(ds);
    if (dout) hipFree(dout);
    return rc;
}

// TEST HOOK: the device's identity decoder (certificate -> P-256 key) over n identities held in host memory
int walk_idfix_probe(fabgpu_ctx* ctx, uint32_t n, const uint8_t* arena, size_t arena_len, const uint32_t* spans, uint8_t* code, uint8_t* key) {
    if (!ctx || (n && (!arena || !spans || !code || !key))) return FABGPU_EINVAL;
    if (n == 0) return FABGPU_OK;
    for (uint32_t i = 0; i < n; i++)
        if (spans[2 * i + 1] < spans[2 * i] || spans[2 * i + 1] > arena_len) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    void *da = nullptr, *ds = nullptr, *dout = nullptr;
    int rc = FABGPU_ENOMEM;
    if (hipMalloc(&da, arena_len + 256) == hipSuccess && hipMalloc(&ds, (size_t)n * 8) == hipSuccess && hipMalloc(&dout, (size_t)n * 65) == hipSuccess) {
        hipError_t e = hipMemcpy(da, arena, arena_len, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(ds, spans, (size_t)n * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = launch_walk_idfix_probe(n, da, ds, (uint8_t*)dout + (size_t)n * 64, dout, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpy(key, dout, (size_t)n * 64, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(code, (uint8_t*)dout + (size_t)n * 64, n, hipMemcpyDeviceToHost);
        rc = hip_to_rc(e);
    }
    if (da) hipFree(da);
    if (ds) hipFree(ds);
    if (dout) hipFree(dout);
    return rc;
}

namespace {
// The host's side of a WalkHostOut flag: poll the mapped word until the kernel has stored `seq` (everything it wrote before is then
// visible).  Every ~50 us the stream is asked whether it has drained: a drained stream without the flag is a launch that failed.
int wait_host_flag(const uint32_t* flag, uint32_t seq, hipStream_t st) {
    for (uint32_t spin = 1;; spin++) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return FABGPU_OK;
        if ((spin & 0x3FFu) == 0) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq ? FABGPU_OK : FABGPU_ELAUNCH;
            if (q != hipErrorNotReady) return hip_to_rc(q);
        }
        __builtin_ia32_pause();
    }
}
}  // namespace

// The pointers of a pass into its buffers, at the places walk_layout.h names: the per-envelope arrays (de = fabgpu_ctx::walk_env) ...
static void bind_env_arrays(WalkArrays& a, uint8_t* de, const WalkEnvLayout& E, uint32_t ne, bool host_counted) {
    a.env_spans = (const uint32_t*)(de + E.env.off);
    a.n_env = ne;
    a.counts = (uint4*)(de + E.cnt.off);
    a.stash = host_counted ? nullptr : (bccsp::walk::EnvStash*)(de + E.stash.off);
    a.bases = (uint4*)(de + E.base.off);
    a.cbase = (uint32_t*)(de + E.cbase.off);
    a.totals = (WalkTotals*)(de + E.tot.off);
    a.tx_type = de + E.type.off;
    a.tx_understood = de + E.und.off;
    a.tx_mask = (uint32_t*)(de + E.mask.off);
    a.tx_flags = de + E.flags.off;
    a.summary = (WalkSummary*)(de + E.sum.off);
    a.learn = (WalkLearn*)(de + E.learn.off);
}
// ... the per-tuple arrays (dt = fabgpu_ctx::walk_tup); the optional ones stay null unless the pass has them ...
static void bind_tuple_arrays(WalkArrays& a, uint8_t* dt, const WalkTupleLayout& T, bool nym_rows, bool memo, bool hmemo, bool row_digests, bool tuple_qxy) {
    a.tuples = (bccsp::BlockTuple*)(dt + T.tup.off);
    a.pre_off2 = (uint32_t*)(dt + T.pre.off);
    a.checks = (bccsp::BlockHashCheck*)(dt + T.chk.off);
    a.gather_spans = (uint32_t*)(dt + T.gsp.off);
    a.gather_off = (uint32_t*)(dt + T.gof.off);
    a.gather_digests = dt + T.gdg.off;
    a.id_idx = (uint32_t*)(dt + T.idx.off);
    a.off2 = (uint32_t*)(dt + T.off.off);
    a.pre_idx = (uint32_t*)(dt + T.pix.off);
    a.key_id = (uint32_t*)(dt + T.kid.off);
    a.qx = dt + T.qx.off; a.qy = dt + T.qy.off; a.r = dt + T.r.off; a.s = dt + T.s.off;
    a.gate_st = dt + T.gst.off;
    a.tflags = dt + T.tfl.off;
    if (nym_rows) {
        a.nym_fields = dt + T.nymf.off;
        a.nym_issuer = (uint32_t*)(dt + T.nymi.off);
        a.nym_issuer_out = (int32_t*)(dt + T.nymio.off);
        a.nym_spans = (uint32_t*)(dt + T.nymsp.off);
    }
    a.row_of = (uint32_t*)(dt + T.row.off);
    a.creator_spans = (uint32_t*)(dt + T.cspan.off);
    a.verdict_bits = (const uint64_t*)(dt + T.bits.off);
    a.verdict_bits_c = (const uint64_t*)(dt + T.bitc.off);
    a.row_digests = row_digests ? dt + T.dig.off : nullptr;
    a.tuple_digests = dt + T.tdig.off;
    a.tuple_qxy = tuple_qxy ? dt + T.tqxy.off : nullptr;
    a.summary_parts = (uint32_t*)(dt + T.sparts.off);
    if (memo) {
        a.memo_ent = (uint32_t*)(dt + T.ment.off);
        a.memo_slots = (uint32_t*)(dt + T.mslots.off);
        a.memo_key_off = (uint32_t*)(dt + T.mkoff.off);
        a.memo_keys = dt + T.mkeys.off;
        a.memo_status = dt + T.mst.off;
        a.memo_totals = (WalkMemoTotals*)(dt + T.mtot.off);
        a.memo_digests = dt + T.mdig.off;
        a.memo_tiles = dt + T.mtiles.off;
        if (hmemo) {
            a.memo_hspans = (uint32_t*)(dt + T.mhsp.off);
            a.memo_hslots = (uint32_t*)(dt + T.mhsl.off);
        }
    }
    a.dev_status = dt + T.dst.off;
    a.tuple_status = dt + T.tst.off;
    a.tuple_hashed = dt + T.hsh.off;
}
// ... and where the last kernel writes what the host waits for (m8 = the device's view of fabgpu_ctx::walk_map)
static void bind_host_out(WalkHostOut& ho, uint8_t* m8, const WalkMapLayout& M, uint32_t* done, bool memo) {
    ho.flag = (uint32_t*)(m8 + WALK_MAP_FINFLAG);
    ho.done = done;
    ho.summary = (WalkSummary*)(m8 + WALK_MAP_SUM);
    ho.memo_totals = memo ? (WalkMemoTotals*)(m8 + WALK_MAP_MTOT) : nullptr;
    ho.learn = (WalkLearn*)(m8 + M.learn.off);
    ho.tx_flags = m8 + M.flags.off; ho.tx_type = m8 + M.type.off; ho.tx_understood = m8 + M.und.off;
    ho.tuple_status = m8 + M.tst.off; ho.tuple_hashed = m8 + M.hsh.off;
    ho.id_idx = (uint32_t*)(m8 + M.idx.off);
}

int walk_block_pass(fabgpu_ctx* ctx, WalkRequest& rq) {
    if (!ctx || !rq.sizes || !rq.env_spans || rq.stage_token == 0) return FABGPU_EINVAL;
    if (rq.n_block_sigs && !rq.block_sigs) return FABGPU_EINVAL;
    const bool has_tail = rq.tail != nullptr && rq.tail_len != 0;
    if (has_tail && ((rq.tail_base & 63u) || (uint64_t)rq.tail_base + rq.tail_len > 0xFFFFFFF0ull)) return FABGPU_EINVAL;
    auto decline = [&](const char* why) {
        rq.declined_why = why;
        return WALK_DECLINED;
    };
    if (rq.n_env == 0) return decline("no envelopes");
    if (rq.n_env > 0x7FFFFFF0u / 64) return FABGPU_ETOOBIG;
    // the staged block: its slot stays locked - the stager kept out of it - until this pass has run
    fabgpu_ctx::Staged* sl = nullptr;
    for (auto& c : ctx->staged_slots)
        if (c.token.load() == rq.stage_token) sl = &c;
    if (!sl) return decline("the staged block was replaced");
    std::unique_lock<std::mutex> slk(sl->m);
    if (sl->token.load() != rq.stage_token || sl->len == 0 || sl->len != rq.block_len) return decline("the staged block was replaced");
    if (has_tail && ((size_t)rq.tail_base < round_up(sl->len, 64) || (size_t)rq.tail_base + rq.tail_len + 128 > sl->cap)) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->fault) return ctx->fault == 2 ? FABGPU_ENOMEM : FABGPU_ELAUNCH;
    DeviceGuard g(ctx->device);
    hipStream_t st = ctx->stream;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const auto t_start = now();
    // (developer aid: FABGPU_WALK_TRACE=1 prints where the HOST side of a pass spends its time, checkpoint by checkpoint)
    static const bool walk_trace = getenv("FABGPU_WALK_TRACE") != nullptr;
    auto mark = [&](const char* what) {
        if (walk_trace) fprintf(stderr, "fabgpu walk %p %-28s %8.3f ms\n", (void*)&rq, what, ms_since(t_start));
    };
    const uint32_t ne = rq.n_env;
    // ---- per-envelope arrays (walk_layout.h) ----
    // (what the host sends up sits together - envelope spans, payload spans, idemix MSPs and, when the host counted, the count kernel's
    //  and the scan's arrays - mirrored at the same offsets in the pinned staging buffer: ONE copy)
    const bool host_counted = rq.host_counts && rq.host_tx_type && rq.host_tx_understood;
    const uint32_t n_msps = rq.idemix_msps && !rq.walk_only ? std::min(rq.n_idemix_msps, WALK_IDEMIX_MSPS_MAX) : 0u;
    // The creators' messages are whole envelope payloads - the longest hashes of a block, a serial chain per message, and for a
    // block of a few hundred transactions THE critical path (300 tx: the chain is 240 us of a 600 us device phase).  With the host's
    // outline of where they are they start before anything is walked, beside the walk's two runs and the gates.
    const bool early_hash = rq.payload_spans && !rq.walk_only && ctx->allow_pair && (uint64_t)ne * 2 <= 65536u;
    WalkEnvShape es;
    es.ne = ne; es.n_msps = n_msps; es.early_hash = early_hash; es.host_counted = host_counted; es.has_issuer_hashes = rq.idemix_issuer_hashes != nullptr;
    const WalkEnvLayout E = walk_env_layout(es);
    int rc;
    if ((rc = ctx->walk_env.ensure(E.total))) return rc;
    // pinned staging: the region above as it goes up (the result arrays are sized further down)
    const size_t up_bytes = host_counted ? E.up_all : E.up_small;
    if ((rc = ctx->walk_pin.ensure(walk_pin_first(E)))) return rc;
    // host-mapped results: the fixed cells (WALK_MAP_*), the arrays follow
    if ((rc = ctx->walk_map.ensure(walk_map_early_bytes(ne)))) return rc;
    if (++ctx->walk_seq == 0) ++ctx->walk_seq;
    const uint32_t seq_tot = ctx->walk_seq;
    uint8_t* de = (uint8_t*)ctx->walk_env.d;
    WalkArrays a;
    a.block = (const uint8_t*)sl->d;
    a.block_len = (uint32_t)sl->len;
    a.arena_len = has_tail ? rq.tail_base + rq.tail_len : (uint32_t)sl->len;
    bind_env_arrays(a, de, E, ne, host_counted);
    uint8_t* up = (uint8_t*)ctx->walk_pin.h;
    memcpy(up + E.env.off, rq.env_spans, E.env.bytes);
    if (early_hash) memcpy(up + E.pay.off, rq.payload_spans, E.pay.bytes);
    if (n_msps) memcpy(up + E.msps.off, rq.idemix_msps, E.msps.bytes);
    if (n_msps && rq.idemix_issuer_hashes) memcpy(up + E.ihash.off, rq.idemix_issuer_hashes, E.ihash.bytes);
    WalkTotals host_tot = {};
    if (host_counted) {
        // the scan, here: exclusive prefix sums per envelope (walk_scan_kernel's outputs), and the totals the host would otherwise wait for
        memcpy(up + E.cnt.off, rq.host_counts, E.cnt.bytes);
        memcpy(up + E.type.off, rq.host_tx_type, E.type.bytes);
        memcpy(up + E.und.off, rq.host_tx_understood, E.und.bytes);
        uint32_t* bases = (uint32_t*)(up + E.base.off);
        uint32_t* cb = (uint32_t*)(up + E.cbase.off);
        uint64_t bt = 0, bp = 0, bc = 0, bg = 0;
        uint32_t bk = 0;
        for (uint32_t e = 0; e < ne; e++) {
            const uint32_t* c = rq.host_counts + 4 * (size_t)e;
            bases[4 * (size_t)e] = (uint32_t)bt; bases[4 * (size_t)e + 1] = (uint32_t)bp; bases[4 * (size_t)e + 2] = (uint32_t)bc; bases[4 * (size_t)e + 3] = (uint32_t)bg;
            cb[e] = bk;
            bt += c[0]; bp += c[1]; bc += c[2]; bg += c[3];
            bk += c[0] ? 1u : 0u;
        }
        if (bt > 0x7FFFFFF0ull || bp > 0x7FFFFFF0ull || bc > 0x7FFFFFF0ull) return FABGPU_ETOOBIG;
        host_tot.tuples = (uint32_t)bt; host_tot.prefixes = (uint32_t)bp; host_tot.checks = (uint32_t)bc; host_tot.creators = bk;
        host_tot.gather_bytes = bg;
    }
    hipError_t err = hipMemcpyAsync(de + E.env.off, up + E.env.off, up_bytes, hipMemcpyHostToDevice, st);
    bool s2_busy = false;
    struct Drain2 {                                                         // (an early exit must not leave the hashes running)
        hipStream_t s;
        bool* busy;
        bool armed = true;
        ~Drain2() { if (armed && *busy) hipStreamSynchronize(s); }
    } drain2{ctx->stream2, &s2_busy};
    if (err == hipSuccess && early_hash) {
        a.payload_spans = (const uint32_t*)(de + E.pay.off);
        a.digest_env = de + E.denv.off;
        err = hipEventRecord(ctx->ev_w[3], st);                            // "the span lists are on the device"
        if (err == hipSuccess) err = hipStreamWaitEvent(ctx->stream2, ctx->ev_w[3], 0);
        if (err == hipSuccess) {
            s2_busy = true;
            // (thousands of them: on CUs of their own, like every long-running launch of a big block)
            // (up to SHA_COOP_MAX of them: eight lanes on a message, the workgroups spread by what a block of ne transactions with four
            //  signatures each will run beside them - `pre` and the endorsements' hashes, nt / 8 workgroups each, the hash checks' ne / 4)
            err = launch_sha256_spans(ne, sl->d, round_up(sl->len, 4) + 64, a.payload_spans, a.digest_env, ctx->stream2, ne > 2048 ? 84u << 10 : 0u,
                                      spread_waves_per_cu(ne / 8 + ne + ne / 4 + 3));
        }
    }
    if (err == hipSuccess && has_tail) {
        if ((rc = ctx->tailbuf.ensure(rq.tail_len))) return rc;
        memcpy(ctx->tailbuf.h, rq.tail, rq.tail_len);
        err = hipMemcpyAsync((uint8_t*)sl->d + rq.tail_base, ctx->tailbuf.h, rq.tail_len, hipMemcpyHostToDevice, st);
        if (err == hipSuccess) err = hipMemsetAsync((uint8_t*)sl->d + rq.tail_base + rq.tail_len, 0, 128, st);
    }
    if (err == hipSuccess) err = hipMemsetAsync(de + E.mask.off, 0, E.mask.bytes, st);
    if (err == hipSuccess) err = hipMemsetAsync(de + E.sum.off, 0, E.sum.bytes, st);
    if (err == hipSuccess) err = hipMemsetAsync(de + E.learn.off, 0, E.learn.bytes, st);
    if (err == hipSuccess) err = hipMemsetAsync(de + E.done.off, 0, E.done.bytes, st);
    if (!host_counted) {
        uint8_t* mh = (uint8_t*)ctx->walk_map.h;
        void* md = nullptr;
        if (err == hipSuccess) err = hipHostGetDevicePointer(&md, mh, 0);
        if (err == hipSuccess) err = launch_walk_count(a, (WalkTotals*)((uint8_t*)md + WALK_MAP_TOT), (uint32_t*)((uint8_t*)md + WALK_MAP_TOTFLAG), seq_tot, st);
        if (err != hipSuccess) return hip_to_rc(err);
        // the one thing the host must know before it can go on - how many tuples, prefixes, checks - arrives in mapped memory
        if ((rc = wait_host_flag((const uint32_t*)(mh + WALK_MAP_TOTFLAG), seq_tot, st))) return rc;
    }
    if (err != hipSuccess) return hip_to_rc(err);
    const WalkTotals tot = host_counted ? host_tot : *(const WalkTotals*)((uint8_t*)ctx->walk_map.h + WALK_MAP_TOT);
    if (tot.gather_bytes > 0x7FFFFFF0ull) return decline("gathered hash inputs exceed 2 GiB");
    const uint64_t nt64 = (uint64_t)tot.tuples + rq.n_block_sigs;
    if (nt64 > 0x7FFFFFF0ull / 160) return FABGPU_ETOOBIG;
    const uint32_t nt = (uint32_t)nt64, np = tot.prefixes, nc = tot.checks;
    if (nt == 0) return decline("no signature in the block");
    WalkCounts cnts;
    cnts.n_tx = ne; cnts.n_tuples = nt; cnts.n_prefixes = np; cnts.n_checks = nc; cnts.n_creators = tot.creators;
    WalkOut out;
    mark("totals known");
    if (!rq.sizes(rq.user, cnts, out)) return FABGPU_ETOOBIG;
    mark("sizes callback");
    // ---- per-tuple arrays (walk_layout.h) ----
    // the verdict memo, if the caller gave room for it (WalkOut::memo_*): built behind the status kernel, copied straight into that room
    const bool memo = out.memo_slots && out.memo_key_off && out.memo_keys && out.memo_status && out.memo_digests && out.memo_slot_cap >= 16 &&
                      (out.memo_slot_cap & (out.memo_slot_cap - 1)) == 0 && out.memo_slot_cap >= 2 * (uint64_t)nt && out.memo_keys_cap != 0 &&
                      out.memo_keys_cap < 0xFFFFFFF0ull;
    // ... and the digest memo's index beside it (message spans by entry + a second slot table), if the caller gave room for that too
    const bool hmemo = memo && out.memo_hspans && out.memo_hslots;
    WalkTupleShape ts;
    ts.nt = nt; ts.np = np; ts.nc = nc; ts.creators = tot.creators; ts.n_msps = n_msps;
    ts.tuple_qxy = out.tuple_qxy != nullptr; ts.memo = memo; ts.hmemo = hmemo; ts.memo_slot_cap = out.memo_slot_cap; ts.memo_keys_cap = out.memo_keys_cap;
    const WalkTupleLayout T = walk_tuple_layout(ts);
    if ((rc = ctx->walk_tup.ensure(T.total))) return rc;
    uint8_t* dt = (uint8_t*)ctx->walk_tup.d;
    a.n_tuples = nt;
    const bool has_nym_rows = n_msps != 0 && tot.creators != 0;
    bind_tuple_arrays(a, dt, T, has_nym_rows, memo, hmemo, out.tuple_digest || memo /* the memo's keys hold the digests */, out.tuple_qxy != nullptr);
    if (has_nym_rows) {
        a.idemix_msps = (const DevIdemixMsp*)(de + E.msps.off);
        a.n_idemix_msps = n_msps;
    }
    a.n_dev_tuples = tot.tuples;
    a.n_creators = tot.creators;
    // Split the submission (WalkArrays::row_of) when one launch would have to run one lane per signature (more than VERIFY_PAIR_MAX
    // tuples) although creators on two lanes + everybody else on one still fit the chip's 65 536 lanes: the creators hash the longest
    // messages (whole payloads), so they get the shorter arithmetic.
    a.split = (ctx->allow_pair && nt > (uint32_t)VERIFY_PAIR_MAX && tot.creators != 0 && tot.creators <= (uint32_t)VERIFY_PAIR_MAX &&
               (uint64_t)2 * tot.creators + (nt - tot.creators) <= 65536u) ? 1u : 0u;
    // Smaller blocks split too - both launches with two lanes per signature, sharing the chip: what counts there is that the creators'
    // 40-block hashes start behind the emit kernel instead of inside the one fused launch (300 tx: 0.92 -> 0.82 ms, 1 000 tx:
    // 1.09 -> 0.99 ms; round-2 probe gpu_dw_small.sh, since removed)
    bool both_pair = false;
    if (!a.split && ctx->allow_pair && tot.creators != 0 && nt > tot.creators && (uint64_t)2 * nt <= 65536u) {
        a.split = 1;
        both_pair = true;
    }
    const bool exclusive = a.split && !both_pair;
    if (memo) {
        a.memo_mask = out.memo_slot_cap - 1;
        a.memo_keys_cap = (uint32_t)T.dev_keys_cap;
        if (n_msps && rq.idemix_issuer_hashes) a.issuer_hashes = de + E.ihash.off;
    }
    if (ctx->d_idtab) {
        a.id_slots = (const uint32_t*)ctx->d_idtab;
        a.id_mask = ctx->idtab_mask;
        a.id_seed = ctx->idtab_seed;
        a.id_entries = (const DevIdEntry*)((uint8_t*)ctx->d_idtab + ctx->idtab_entries_off);
        a.id_bytes = (uint8_t*)ctx->d_idtab + ctx->idtab_bytes_off;
    }
    // pinned room for everything that comes back
    const WalkPinLayout P = walk_pin_layout(E, ne, ts, rq.n_block_sigs, out.nym_issuer != nullptr);
    {
        // (growing the pinned buffer moves it: nothing above is still needed from the old one)
        if ((rc = ctx->walk_pin.ensure(P.total))) return rc;
    }
    uint8_t* ph = (uint8_t*)ctx->walk_pin.h;
    // ... and mapped room for what the last kernel writes itself (flags, statuses, identity indices, learn records, summary)
    const WalkMapLayout M = walk_map_layout(ne, nt);
    if ((rc = ctx->walk_map.ensure(M.total))) return rc;                   // (may move it: the totals above have been read)
    uint8_t* mh = (uint8_t*)ctx->walk_map.h;
    WalkHostOut ho;
    {
        void* md = nullptr;
        if (hipHostGetDevicePointer(&md, mh, 0) != hipSuccess) return FABGPU_ELAUNCH;
        bind_host_out(ho, (uint8_t*)md, M, (uint32_t*)(de + E.done.off), memo);
    }
    mark("buffers ensured");
    err = launch_walk_emit(a, tot, st);
    if (err == hipSuccess && rq.n_block_sigs) {
        memcpy(ph + P.sigs.off, rq.block_sigs, (size_t)rq.n_block_sigs * sizeof(bccsp::BlockTuple));
        err = hipMemcpyAsync(a.tuples + tot.tuples, ph + P.sigs.off, (size_t)rq.n_block_sigs * sizeof(bccsp::BlockTuple), hipMemcpyHostToDevice, st);
    }
    if (err != hipSuccess) return hip_to_rc(err);
    auto fetch = [&](void* host_dst, size_t pin_off, const void* dev_src, size_t bytes) {
        if (!host_dst || bytes == 0 || err != hipSuccess) return;
        err = hipMemcpyAsync(ph + pin_off, dev_src, bytes, hipMemcpyDeviceToHost, st);
    };
    auto deliver = [&](void* host_dst, size_t pin_off, size_t bytes) {
        if (host_dst && bytes) memcpy(host_dst, ph + pin_off, bytes);
    };
    if (rq.walk_only) {
        fetch(out.tx_type, P.type.off, a.tx_type, P.type.bytes);
        fetch(out.tx_understood, P.und.off, a.tx_understood, P.und.bytes);
        fetch(out.tuples, P.tup.off, a.tuples, P.tup.bytes);
        fetch(out.prefixes, P.pre.off, a.pre_off2, (size_t)np * 8);
        fetch(out.checks, P.chk.off, a.checks, (size_t)nc * sizeof(bccsp::BlockHashCheck));
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err != hipSuccess) return hip_to_rc(err);
        deliver(out.tx_type, P.type.off, P.type.bytes);
        deliver(out.tx_understood, P.und.off, P.und.bytes);
        deliver(out.tuples, P.tup.off, P.tup.bytes);
        deliver(out.checks, P.chk.off, (size_t)nc * sizeof(bccsp::BlockHashCheck));
        if (out.prefixes)                                          // (start, end) pairs on the device, (offset, length) for the caller
            for (uint32_t p = 0; p < np; p++) {
                const uint32_t s0 = ((const uint32_t*)(ph + P.pre.off))[2 * p], s1 = ((const uint32_t*)(ph + P.pre.off))[2 * p + 1];
                out.prefixes[p].off = s0;
                out.prefixes[p].len = s1 - s0;
            }
        rq.ms_walk = ms_since(t_start);
        return FABGPU_OK;
    }
    // From here on three streams work side by side; whatever happens, none of them may still be running when this call returns
    // (the next pass reuses every buffer).
    hipStream_t s2 = ctx->stream2, s3 = ctx->stream3, s4 = ctx->stream4;
    struct Drain {
        hipStream_t a, b, c, d;
        bool armed = true;
        ~Drain() {
            if (!armed) return;
            hipStreamSynchronize(a);
            hipStreamSynchronize(b);
            hipStreamSynchronize(c);
            hipStreamSynchronize(d);
        }
    } drain{s2, s3, s4, st};
    const size_t arena_bytes = round_up(has_tail ? (size_t)rq.tail_base + rq.tail_len : sl->len, 4) + 64;
    ShaPrefixArgs pa;
    pa.spans = true;
    if (np) {
        pa.m = np;
        pa.pre_off = a.pre_off2;
        pa.pre_idx = a.pre_idx;
        pa.mid_scratch = dt + T.mid.off;
    }
    const size_t gscr = round_up((size_t)tot.gather_bytes, 4) + 64;
    if (nc && (rc = ctx->gscr.ensure(gscr))) return rc;
    // the emitted prefixes / hash checks are all stream2 and stream3 need: mid-states and the TxID / proposal-hash digests run while
    // the main stream looks identities up and gates signatures
    hipStream_t sc = s2;                                                   // the creators' stream
    bool memo_early_pending = false;
    KeyedSnap snap(ctx, {st, s2, s3, s4});                                // (until the pass returns: a mispredicted class is launched again at its very end)
    const uint32_t nkeys = snap.nkeys;
    const int32_t** kt = snap.kt;
    bool keyed_c = ctx->pred_keyed_creators && nkeys != 0, keyed_o = ctx->pred_keyed_others && nkeys != 0;
    if (!a.split) keyed_c = keyed_o = keyed_c && keyed_o;                  // one launch serves both classes
    // A block of a few hundred transactions (what a default network cuts: sampleconfig/configtx.yaml:284 MaxMessageCount 500) cannot
    // fill the chip, and its device phase is a chain of LATENCIES: the creators' payload hashes (76 serial SHA-256 blocks), then a
    // keyed verification (78 000 instructions per wavefront on two lanes).  The wide kernels (p256_wide29.h) put eight lanes on a
    // signature and cut the verification in two: `pre` - s^-1, u2, u2 Q: everything but the digest - runs right behind the gates,
    // BESIDE the hashes; `post` (e w, u1 G, the final addition and comparison: 18 000 instructions) is all that is left behind them.
    const bool wide = ctx->allow_wide && both_pair && keyed_c && keyed_o && nt <= (uint32_t)WIDE_LAUNCH_MAX && !has_nym_rows;
    // The one-wavefront workgroups of a small block's launches - `pre` (nt / 8), the endorsements' hashes (nt / 8), the hash checks'
    // (nc / 8), the creators' early hashes still running - are placed together (kernels.h spread_waves_per_cu).
    const uint32_t spread = spread_waves_per_cu(nt / 8 + nt / 8 + nc / 8 + 3);
    err = hipEventRecord(ctx->ev_w[0], st);
    // (The gates are queued right here, ahead of the side streams' work: on a small block the host's calls, not the kernels, set the pace,
    //  and the gate kernel is the main stream's critical path.)
    if (a.split && early_hash) a.early_creator_hash = 1;
    if (err == hipSuccess && has_nym_rows) {
        // rows of creators that are not idemix stay all-zero; issuer_out -1 = inactive
        err = hipMemsetAsync(dt + T.nym_zeroed.off, 0, T.nym_zeroed.bytes, st);
        if (err == hipSuccess) err = hipMemsetAsync(dt + T.nymio.off, 0xFF, T.nymio.bytes, st);
    }
    // With idemix creators expected the creators' tuples are gated in a launch of their own, first: the nym launch (a long kernel: the
    // pass's critical path on such a block) waits for that one only.
    const bool creators_first = has_nym_rows && ctx->pred_has_nym;
    if (creators_first) {
        a.gate_mode = 1;
        if (err == hipSuccess) err = launch_walk_gate(a, st);
        if (err == hipSuccess) err = hipEventRecord(ctx->ev_w[5], st);   // "the creators' gates are through"
        a.gate_mode = 2;
        if (err == hipSuccess) err = launch_walk_gate(a, st);
        a.gate_mode = 0;
    } else {
        if (err == hipSuccess) err = launch_walk_gate(a, st);
        if (err == hipSuccess && has_nym_rows) err = hipEventRecord(ctx->ev_w[5], st);   // "the gates are through" (a nym launch waits for it)
    }
    if (err == hipSuccess && memo) {
        // stream4, behind its digests: the EARLY half of the verdict memo - candidates, keys up to the digest, offsets - and its copy into
        // the caller's table, all of it beside the verify launches (block_walk_kernels.hip "the block's verdict memo")
        err = hipEventRecord(ctx->ev_w[7], st);                            // "every gate is through"
        memo_early_pending = true;
    }
    // A block of a few hundred transactions: the endorsements' messages are hashed WHOLE, eight lanes on each (sha256_coop.h) - no
    // mid-state launch in front of them; the mid-states follow on the same stream, off the critical path, for the relaunch below that
    // continues from them should "keyed" have been a wrong guess.
    const bool coop_messages = wide && nt - tot.creators <= SHA_COOP_MAX;
    auto queue_midstates = [&]() {
        // stream3: the mid-states of the shared prefixes (the endorsements' launch continues from them), on CUs of their own: 40
        // workgroups that would otherwise share SIMDs with the 40 000 short-lived wavefronts of the gate kernel and take 4x as long,
        // with the endorsements' launch waiting for them (measured, round-2 probe gpu_dw_sched.sh, since removed: device phase 1.04 -> 0.90 ms)
        ShaPrefixArgs pm = pa;
        pm.lds_reserve = coop_messages ? 0u : 84u << 10;
        if (!coop_messages) err = hipStreamWaitEvent(s3, ctx->ev_w[0], 0);
        if (err == hipSuccess) err = launch_sha256_midstates(sl->d, arena_bytes, pm, s3);
        if (err == hipSuccess) err = hipEventRecord(ctx->ev_w[1], s3);
    };
    auto queue_messages = [&]() {
        // stream3 (behind the mid-states unless the messages are hashed whole): the endorsements' (and block signatures') digests, rows
        // [n_creators, nt) - hash only, beside `pre`
        ShaPrefixArgs ph = pa;
        ph.mid_ready = true;
        ph.digests = dt + T.dig.off + 32 * (size_t)tot.creators;
        if (np) ph.pre_idx = a.pre_idx + tot.creators;
        err = hipStreamWaitEvent(s3, ctx->ev_w[3], 0);                     // (recorded behind the gates: the emit kernel's event is implied)
        if (err == hipSuccess)
            err = coop_messages ? launch_sha256_messages_coop(nt - tot.creators, sl->d, arena_bytes, a.off2 + 2 * (size_t)tot.creators, ph, s3, spread)
                                : launch_sha256_messages(nt - tot.creators, sl->d, arena_bytes, a.off2 + 2 * (size_t)tot.creators, ph, s3);
        if (err == hipSuccess) err = hipEventRecord(ctx->ev_w[10], s3);
    };
    if (err == hipSuccess && wide) {
        err = hipEventRecord(ctx->ev_w[3], st);                            // the submission arrays are complete (the endorsements' hashes read them)
        // (the order of these calls is the order the kernels start in - the host's calls, 3 us each, set the pace of a small block - and
        //  since the hashes run on eight lanes `pre` is the longer leg of what `post` waits for: 75 us against 62)
        if (err == hipSuccess) err = launch_p256_wide_pre(nt, a.key_id, nkeys, (const void*)kt, a.r, a.s, ctx->d_gtab, dt + T.wide.off, st, spread);
        if (err == hipSuccess && coop_messages) queue_messages();
    }
    if (err == hipSuccess && a.split) {
        // stream2: the creators' digests into rows [0, n_creators), so that their launch only has the arithmetic left.  Either they
        // were hashed per envelope from the host's outline (early_hash, queued before the walk: a scatter by the scan's creator ranks
        // is all that is left), or they are hashed now, beside the identity lookup and the gates.
        err = hipStreamWaitEvent(sc, ctx->ev_w[0], 0);
        if (err == hipSuccess && early_hash) {
            err = launch_walk_creator_digests(a, dt + T.dig.off, sc);
        } else if (err == hipSuccess) {
            err = launch_sha256_spans(tot.creators, sl->d, arena_bytes, a.creator_spans, dt + T.dig.off, sc, exclusive ? 84u << 10 : 0u);
        }
        if (err == hipSuccess && wide) err = hipEventRecord(ctx->ev_w[4], sc);   // "the creators' digests are in their rows" (the one `post` launch waits for it)
    }
    if (err == hipSuccess && np && !coop_messages) queue_midstates();
    if (err == hipSuccess && wide && !coop_messages) queue_messages();
    if (err == hipSuccess && np && coop_messages) queue_midstates();
    if (err == hipSuccess && nc) {       // stream4: the TxID / proposal-hash digests (only the flags at the very end wait for them)
        err = hipStreamWaitEvent(s4, ctx->ev_w[0], 0);
        if (err == hipSuccess) err = launch_gather_sha256(nc, sl->d, arena_bytes, a.gather_spans, a.gather_off, ctx->gscr.d, gscr, dt + T.gdg.off, s4, 0, spread);
        if (err == hipSuccess) err = hipEventRecord(ctx->ev_w[2], s4);
    }
    mark("side streams queued");
    if (err == hipSuccess && memo_early_pending) {
        if (hmemo) err = hipMemsetAsync(dt + T.mhsl.off, 0, T.mhsl.bytes, s4);   // (ahead of the wait for the gates)
        if (err == hipSuccess) err = hipStreamWaitEvent(s4, ctx->ev_w[7], 0);
        // len, the tiled scan (entry indices, key offsets), then the key bytes on stream4 and - beside them, on stream3 - the digest
        // memo's index: both only need the scan (round 6: one after the other they were 85 us between the gates and the keys' copy)
        if (err == hipSuccess) err = launch_walk_memo_early(a, s4, hmemo ? ctx->ev_w[9] : nullptr);
        if (err == hipSuccess && hmemo) err = hipStreamWaitEvent(s3, ctx->ev_w[9], 0);          // "the scan is through"
        if (err == hipSuccess && hmemo) err = launch_walk_memo_index(a, s3);
        if (err == hipSuccess && hmemo) err = hipEventRecord(ctx->ev_w[11], s3);
        mark("memo early launched");
        if (err == hipSuccess) err = hipMemcpyAsync(out.memo_key_off, dt + T.mkoff.off, T.mkoff.bytes, hipMemcpyDeviceToHost, s4);
        mark("memo key_off copy queued");
        if (err == hipSuccess) err = hipMemcpyAsync(out.memo_keys, dt + T.mkeys.off, out.memo_keys_cap, hipMemcpyDeviceToHost, s4);
        mark("memo keys copy queued");
        if (err == hipSuccess && hmemo) err = hipStreamWaitEvent(s4, ctx->ev_w[11], 0);
        if (err == hipSuccess && hmemo) err = hipMemcpyAsync(out.memo_hspans, dt + T.mhsp.off, T.mhsp.bytes, hipMemcpyDeviceToHost, s4);
        if (err == hipSuccess && hmemo) err = hipMemcpyAsync(out.memo_hslots, dt + T.mhsl.off, T.mhsl.bytes, hipMemcpyDeviceToHost, s4);
        if (err == hipSuccess) err = hipEventRecord(ctx->ev_w[8], s4);
    }
    // The block's idemix creators: ONE nym launch over their rows, packed (walk_nym_pack_kernel: 2 000 idemix creators among 10 000 are
    // 125 wavefronts of the four-lane kernel, not 625 - the ECDSA launches beside it keep their SIMDs), on stream3 behind the mid-states.
    // Queued on a prediction like the key tables - the previous block had idemix creators, about so many - and caught up with below if
    // the gates say there are some and nobody launched, or more than the launch had rows for.
    bool nym_ran = false;
    uint32_t nym_cap = 0;
    auto run_nym = [&](uint32_t cap) -> int {
        cap = std::min<uint32_t>(tot.creators, (cap + 63u) & ~63u);
        // The launch's rows take their inputs through the pack kernel's list (row -> creator rank); rows nobody claims stay idle (~0).
        // The status bytes start out as "not decided" so that a row the nym kernel never ran over can not read as valid.  (All of that
        // ahead of the wait for the gates.)
        hipError_t e = hipMemsetAsync(dt + T.nymga.off, 0xFF, (size_t)cap * 4, s3);
        if (e == hipSuccess) e = hipMemsetAsync(dt + T.nymb.off, 0, walk_nym_bits_bytes(cap), s3);
        if (e == hipSuccess) e = hipMemsetAsync(dt + T.nymst.off, 6 /* FABGPU_NYM_NEEDS_SW */, walk_nym_status_bytes(cap), s3);
        if (e == hipSuccess) e = hipStreamWaitEvent(s3, ctx->ev_w[5], 0);
        a.nym_slot = (uint32_t*)(dt + T.nymsl.off);
        if (e == hipSuccess) e = launch_walk_nym_pack(a, (uint32_t*)(dt + T.nymga.off), cap, s3);
        if (e != hipSuccess) return hip_to_rc(e);
        const size_t col = T.nym_col;
        uint8_t* f = dt + T.nymf.off;
        int r2 = nym_verify_dev(ctx, cap, sl->d, arena_bytes, dt + T.nymsp.off, true, dt + T.nymi.off, f, f + col, f + 2 * col, f + 3 * col, f + 4 * col, f + 5 * col,
                                dt + T.nymb.off, dt + T.nymst.off, s3, false, dt + T.nymga.off,
                                exclusive ? 84u << 10 : 0u);   // on CUs of its own, like the two ECDSA launches (kernels.h)
        if (r2 != FABGPU_OK) return r2;
        e = hipEventRecord(ctx->ev_w[6], s3);                              // (the main stream waits for it in front of the status kernel, not here:
        if (e != hipSuccess) return hip_to_rc(e);                          // the ECDSA launches queued next must run BESIDE the nym kernel)
        a.nym_cap = cap;
        a.nym_status = dt + T.nymst.off;
        nym_ran = true;
        nym_cap = cap;
        return FABGPU_OK;
    };
    if (has_nym_rows && ctx->pred_has_nym && (rc = run_nym(ctx->pred_nym_rows + ctx->pred_nym_rows / 4 + 64))) return rc;
    // What the gates found decides which kernels SHOULD run per launch class - registered comb tables when every submitted tuple of the
    // class has one, keys carried in the rows otherwise - and whether this pass may answer at all.  Neither is waited for: the launches
    // are queued on a prediction (fabgpu_ctx::pred_keyed_*: what held for the previous block; "fresh keys" is always correct) and the
    // summary is read once, at the very end; a class that was predicted "keyed" and was not is launched again.
    rq.ms_walk = ms_since(t_start);
    const auto t_verify = now();
    pa.mid_ready = true;
    pa.digests = (out.tuple_digest || memo) ? dt + T.dig.off : nullptr;
    // rows [row0, row0 + n) as one fused (hash + verify) launch on stream `ls`
    auto verify_rows = [&](uint32_t row0, uint32_t n, bool prefixed, bool pair, bool keyed, void* bits, hipStream_t ls) -> int {
        ShaPrefixArgs p = pa;
        if (exclusive) p.lds_reserve = 84u << 10;                          // the two launches of a split submission on disjoint CUs (kernels.h)
        if (!prefixed) {
            p.m = 0;
            p.pre_off = p.pre_idx = nullptr;
            p.mid_scratch = nullptr;
        } else {
            p.pre_idx = a.pre_idx + row0;
        }
        if (p.digests) p.digests = dt + T.dig.off + 32 * (size_t)row0;
        VerifyLaunch v;
        v.n = n;
        v.arena = sl->d; v.arena_bytes = arena_bytes; v.off = a.off2 + 2 * (size_t)row0; v.pa = p;
        v.r = a.r + 32 * (size_t)row0; v.s = a.s + 32 * (size_t)row0;
        v.gtab = ctx->d_gtab;
        v.verdict_bits = bits; v.status = dt + T.dst.off + row0;
        v.allow_pair = pair;
        hipError_t e;
        if (keyed) {
            v.key_id = a.key_id + row0; v.nkeys = nkeys; v.ktabs = (const void*)kt;
            e = launch_verify(v, ls);
        } else {
            size_t wi = 0;
            void* wsp = nullptr;
            int r2 = ctx->acquire_qws(verify_workspace_bytes(n, pair), &wi, &wsp, ls);
            if (r2 != FABGPU_OK) return r2;
            v.qx = a.qx + 32 * (size_t)row0; v.qy = a.qy + 32 * (size_t)row0; v.qws = wsp;
            e = launch_verify(v, ls);
            ctx->release_qws(wi, ls);
        }
        return hip_to_rc(e);
    };
    // the creators of a split submission: rows [0, n_creators), digests ready (or about to be: same stream), arithmetic only
    auto verify_creators = [&](bool keyed) -> int {
        VerifyLaunch v;
        v.n = tot.creators;
        v.e = dt + T.dig.off; v.r = a.r; v.s = a.s;
        v.gtab = ctx->d_gtab;
        v.verdict_bits = dt + T.bitc.off; v.status = dt + T.dst.off;
        v.allow_pair = true; v.lds_reserve = exclusive ? 84u << 10 : 0u;
        hipError_t e;
        if (keyed) {
            v.key_id = a.key_id; v.nkeys = nkeys; v.ktabs = (const void*)kt;
            e = launch_verify(v, s2);
        } else {
            size_t wi = 0;
            void* wsp = nullptr;
            int r2 = ctx->acquire_qws(verify_workspace_bytes(tot.creators, true), &wi, &wsp, s2);
            if (r2 != FABGPU_OK) return r2;
            v.qx = a.qx; v.qy = a.qy; v.qws = wsp;
            v.table_lds = ctx->pair_table_lds; v.pair_solo = ctx->pair_solo; v.pair_dbl1 = ctx->pair_dbl1; v.pair_booth4 = ctx->pair_booth4; v.pair_table_add = ctx->pair_table_add;
            e = launch_verify(v, s2);
            ctx->release_qws(wi, s2);
        }
        return hip_to_rc(e);
    };
    // the end of a pass on the main stream: statuses and digest comparisons, the big optional arrays as copies (tuple records, digests,
    // keys: only a caller that seeds the memo or wants spans asks for them), then the kernel that writes the small results into mapped
    // memory and raises the flag - behind the copies, so the flag covers them too
    auto finish = [&]() -> int {
        if (++ctx->walk_seq == 0) ++ctx->walk_seq;
        ho.seq = ctx->walk_seq;
        if (err == hipSuccess && nym_ran) err = hipStreamWaitEvent(st, ctx->ev_w[6], 0);     // the nym kernel's answers
        if (err == hipSuccess && memo) err = hipMemsetAsync(dt + T.mslots.off, 0, T.mslots.bytes, st);
        if (err == hipSuccess && memo) err = hipMemsetAsync(&((WalkMemoTotals*)(dt + T.mtot.off))->live, 0, 4, st);
        mark("finish: memsets queued");
        if (!memo && !out.tuples && !out.tuple_digest && !out.tuple_qxy && !(has_nym_rows && out.nym_issuer) && walk_small_finish_fits(a, nc)) {
            // a small block, flags only: statuses, digest comparisons and the finish in one launch
            if (err == hipSuccess) err = launch_walk_status_finish_small(a, nc, ho, st);
            mark("finish: last kernel queued");
            if (err != hipSuccess) return hip_to_rc(err);
            int r2 = wait_host_flag((const uint32_t*)(mh + WALK_MAP_FINFLAG), ho.seq, st);
            if (r2 != FABGPU_OK) return r2;
            rq.summary = *(const WalkSummary*)(mh + WALK_MAP_SUM);
            return FABGPU_OK;
        }
        if (err == hipSuccess) err = launch_walk_status_checks(a, nc, st);
        if (memo) {
            // the LATE half of the memo: digests, status bytes and slots of the candidates that were hashed and decided
            if (err == hipSuccess) err = launch_walk_memo_late(a, st);
            if (err == hipSuccess) err = hipMemcpyAsync(out.memo_slots, dt + T.mslots.off, T.mslots.bytes, hipMemcpyDeviceToHost, st);
            if (err == hipSuccess) err = hipMemcpyAsync(out.memo_digests, dt + T.mdig.off, T.mdig.bytes, hipMemcpyDeviceToHost, st);
            if (err == hipSuccess) err = hipMemcpyAsync(out.memo_status, dt + T.mst.off, T.mst.bytes, hipMemcpyDeviceToHost, st);
            mark("finish: late memo copies queued");
        }
        fetch(out.tuples, P.tup.off, a.tuples, P.tup.bytes);
        fetch(out.tuple_digest, P.dig.off, dt + T.tdig.off, P.dig.bytes);
        fetch(out.tuple_qxy, P.qxy.off, dt + T.tqxy.off, P.qxy.bytes);
        if (has_nym_rows) fetch(out.nym_issuer, P.nymi.off, dt + T.nymio.off, P.nymi.bytes);
        if (err == hipSuccess && memo) err = hipStreamWaitEvent(st, ctx->ev_w[8], 0);        // the memo's early half (long done: it ran beside the verify launches)
        if (err == hipSuccess) err = launch_walk_finish(a, ho, st);
        mark("finish: last kernel queued");
        if (err != hipSuccess) return hip_to_rc(err);
        int r2 = wait_host_flag((const uint32_t*)(mh + WALK_MAP_FINFLAG), ho.seq, st);
        if (r2 != FABGPU_OK) return r2;
        rq.summary = *(const WalkSummary*)(mh + WALK_MAP_SUM);
        if (memo) {
            const WalkMemoTotals mt = *(const WalkMemoTotals*)(mh + WALK_MAP_MTOT);
            rq.memo_n = mt.overflow ? 0 : mt.n;
            rq.memo_live = mt.overflow ? 0 : mt.live;
            rq.memo_bytes = mt.overflow ? 0 : mt.bytes;
            if (rq.memo_n && mt.bytes > out.memo_keys_cap) {
                // more key bytes than the room that was copied ahead (signatures far longer than an ECDSA signature's 72 bytes): the caller
                // makes room, the keys are copied again - whole - and the pass answers a little later; no room: no memo for this block
                uint8_t* big = rq.memo_grow ? rq.memo_grow(rq.user, (size_t)mt.bytes) : nullptr;
                if (!big || hipMemcpy(big, dt + T.mkeys.off, (size_t)mt.bytes, hipMemcpyDeviceToHost) != hipSuccess) rq.memo_n = rq.memo_live = 0;
            }
        }
        return FABGPU_OK;
    };
    if (np && !wide) err = hipStreamWaitEvent(st, ctx->ev_w[1], 0);      // the mid-states (long done: they ran beside the gates)
    if (err != hipSuccess) return hip_to_rc(err);
    if (wide) {
        // the second phase of every row's verification as ONE launch, on this stream behind `pre`, once both kinds of digests are in
        // their rows (the endorsements' hashes: stream3; the creators' scatter: stream2 - both long done when `pre` ends): one launch
        // and one cross-stream wait fewer in front of the finish than a launch per class had
        err = hipStreamWaitEvent(st, ctx->ev_w[10], 0);
        if (err == hipSuccess) err = hipStreamWaitEvent(st, ctx->ev_w[4], 0);
        a.verdict_bits_all = (const uint64_t*)(dt + T.bita.off);
        a.all_creators = a.all_others = 1;
        if (err == hipSuccess) err = launch_p256_wide_post(nt, dt + T.dig.off, a.r, ctx->d_gtab, dt + T.wide.off, dt + T.bita.off, dt + T.dst.off, st, spread);
    } else if (a.split) {
        // creators on stream2 (two lanes per signature), everybody else on the main stream: side by side
        err = hipEventRecord(ctx->ev_w[3], st);                            // the submission arrays are complete
        if (err == hipSuccess) err = hipStreamWaitEvent(s2, ctx->ev_w[3], 0);
        if (err != hipSuccess) return hip_to_rc(err);
        if ((rc = verify_creators(keyed_c))) return rc;
        err = hipEventRecord(ctx->ev_w[4], s2);
        if (err != hipSuccess) return hip_to_rc(err);
        if ((rc = verify_rows(tot.creators, nt - tot.creators, np != 0, both_pair, keyed_o, dt + T.bits.off, st))) return rc;
        err = hipStreamWaitEvent(st, ctx->ev_w[4], 0);
    } else {
        if ((rc = verify_rows(0, nt, np != 0, ctx->allow_pair, keyed_o, dt + T.bits.off, st))) return rc;
    }
    if (err == hipSuccess && nc) err = hipStreamWaitEvent(st, ctx->ev_w[2], 0);
    if (err != hipSuccess) return hip_to_rc(err);
    mark("verify launches queued");
    if ((rc = finish())) return rc;
    mark("finish flag seen");
    if (rq.summary.n_outline_differs) return decline("the device's walk of an envelope differs from the host's outline of it (creator message span, or the counts)");
    // (summary.n_undecided - certificates whose key lies beyond the decoder's window - are TUPLE_ST_NEEDS_SW tuples of their own
    //  transactions, not a reason to give the block up)
    if (rq.summary.n_submitted == 0) return decline("no tuple for the device to decide");
    {
        // Was "keyed" a wrong guess for a class?  Then its rows ran against filler tables: launch it again with the keys carried along
        // (a new client's first block, an endorser's first 64 signatures: once per change of regime), and redo the flags.
        const bool unk_c = rq.summary.n_unkeyed_creator != 0, unk_o = rq.summary.n_unkeyed_other != 0;
        const bool redo_c = a.split ? (keyed_c && unk_c) : false, redo_o = a.split ? (keyed_o && unk_o) : (keyed_o && (unk_c || unk_o));
        // idemix creators turned up and nobody had launched for them, or for fewer
        const bool redo_nym = has_nym_rows && rq.summary.n_nym != 0 && (!nym_ran || rq.summary.n_nym > nym_cap);
        ctx->pred_keyed_creators = !unk_c;
        ctx->pred_keyed_others = !unk_o;
        ctx->pred_has_nym = has_nym_rows && rq.summary.n_nym != 0;
        ctx->pred_nym_rows = rq.summary.n_nym;
        if (redo_c || redo_o || redo_nym) {
            rq.relaunched = (redo_c ? 1u : 0u) + (redo_o ? 1u : 0u) + (redo_nym ? 1u : 0u);
            if (redo_nym && (rc = run_nym(rq.summary.n_nym))) return rc;
            if (redo_c) {
                keyed_c = false;
                a.all_creators = 0;                                        // (their verdicts come from their own launch's bitmap now)
                if ((rc = verify_creators(false))) return rc;
                err = hipEventRecord(ctx->ev_w[4], s2);
                if (err == hipSuccess) err = hipStreamWaitEvent(st, ctx->ev_w[4], 0);
                if (err != hipSuccess) return hip_to_rc(err);
            }
            if (redo_o) {
                keyed_o = false;
                a.all_others = 0;
                if (!a.split) keyed_c = false;
                if (wide && np && (err = hipStreamWaitEvent(st, ctx->ev_w[1], 0)) != hipSuccess) return hip_to_rc(err);   // (wide: nobody waited for the mid-states yet)
                if ((rc = a.split ? verify_rows(tot.creators, nt - tot.creators, np != 0, both_pair, false, dt + T.bits.off, st)
                                  : verify_rows(0, nt, np != 0, ctx->allow_pair, false, dt + T.bits.off, st)))
                    return rc;
            }
            err = hipMemsetAsync(de + E.mask.off, 0, E.mask.bytes, st);
            if (err == hipSuccess) err = hipMemsetAsync(a.summary, 0, offsetof(WalkSummary, n_learn), st);   // (the status kernel adds them up again)
            if (err == hipSuccess) err = hipMemsetAsync(de + E.done.off, 0, E.done.bytes, st);
            if (err != hipSuccess) return hip_to_rc(err);
            if ((rc = finish())) return rc;
        }
    }
    rq.keyed_creators = keyed_c;
    rq.keyed_others = keyed_o;
    rq.ms_verify = ms_since(t_verify);
    auto from_map = [&](void* host_dst, size_t map_off, size_t bytes) {
        if (host_dst && bytes) memcpy(host_dst, mh + map_off, bytes);
    };
    from_map(out.tx_flags, M.flags.off, M.flags.bytes);
    from_map(out.tx_type, M.type.off, M.type.bytes);
    from_map(out.tx_understood, M.und.off, M.und.bytes);
    from_map(out.tuple_status, M.tst.off, M.tst.bytes);
    from_map(out.tuple_hashed, M.hsh.off, M.hsh.bytes);
    from_map(out.id_idx, M.idx.off, M.idx.bytes);
    from_map(rq.learn_out, M.learn.off, M.learn.bytes);
    deliver(out.tuples, P.tup.off, P.tup.bytes);
    deliver(out.tuple_digest, P.dig.off, P.dig.bytes);
    deliver(out.tuple_qxy, P.qxy.off, P.qxy.bytes);
    if (has_nym_rows) deliver(out.nym_issuer, P.nymi.off, P.nymi.bytes);
    else if (out.nym_issuer && tot.creators) memset(out.nym_issuer, 0xFF, P.nymi.bytes);
    drain.armed = false;                                                    // (the flag was raised behind everything: all four streams are idle)
    drain2.armed = false;
    return FABGPU_OK;
}

// What `slots` overlapping passes over blocks of up to block_bytes / n_tx transactions / n_tuples signatures need on this device, made
// NOW (provider construction: ProviderOptions::concurrent_passes) instead of when passes first overlap - the staging slots for uploaded
// blocks, the pinned staging buffer, the pass's device / pinned / host-mapped arrays at their worst case (walk_layout.h), the gather scratch.  A peer
// that joins a channel gets no untimed rounds: measured in round 3, the first overlapping passes of a provider took 5-16 ms (a second
// and third 63 MB staging slot, the arrays of the first memo-seeding pass).  Best effort: a failed allocation is simply made later.
int walk_preallocate(fabgpu_ctx* ctx, size_t block_bytes, uint32_t n_tx, uint32_t n_tuples, int slots) {
    if (!ctx) return FABGPU_EINVAL;
    if (block_bytes > 0xFFFFFF00ull) return FABGPU_ETOOBIG;
    DeviceGuard g(ctx->device);
    int rc = FABGPU_OK;
    const size_t need = round_up(block_bytes, 64) + 128;
    // ALL staging slots, whatever `slots` says: fabgpu_arena_stage takes the least recently filled free slot, i.e. it walks round all
    // N_STAGED of them even when passes never overlap - with two of three made here, the third pass of a fresh provider paid for the
    // third slot's 57 MB hipMalloc inside its upload (1.5 ms instead of 1.05: profiles/r05_fresh_provider_probe.txt).
    (void)slots;
    // every kernel function the passes will launch, resolved now (kernels.h warm_kernel_functions_*)
    (void)warm_kernel_functions_kernels();
    (void)warm_kernel_functions_wide();
    (void)warm_kernel_functions_idemix();
    (void)warm_kernel_functions_walk();
    (void)warm_kernel_functions_keytab();
    for (int i = 0; i < fabgpu_ctx::N_STAGED; i++) {
        fabgpu_ctx::Staged& sl = ctx->staged_slots[i];
        std::lock_guard<std::mutex> lk(sl.m);
        if (sl.cap >= need + (64 << 10)) continue;
        if (sl.d) hipFree(sl.d);
        sl.d = nullptr;
        sl.cap = 0;
        sl.token.store(0);
        sl.len = 0;
        if (hipMalloc(&sl.d, need + need / 8 + (64 << 10)) != hipSuccess) {
            sl.d = nullptr;
            rc = FABGPU_ENOMEM;
            continue;
        }
        sl.cap = need + need / 8 + (64 << 10);
    }
    {
        std::lock_guard<std::mutex> plk(ctx->stage_pin_mu);
        if (block_bytes >= ((size_t)4 << 20) && ctx->stage_pin.ensure(block_bytes) != FABGPU_OK) rc = FABGPU_ENOMEM;
        if (!ctx->stage_pool) ctx->stage_pool.reset(new (std::nothrow) WorkerPool(4));
    }
    {
        // the device's copy of the identity cache (walk_idtab_set): a fresh provider's first non-empty table arrives before its SECOND
        // pass - its room and its three small synchronous uploads are rehearsed with a one-entry table, then the table is empty again
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            if (ctx->idtab_buf.ensure((size_t)1 << 20) != FABGPU_OK) rc = FABGPU_ENOMEM;
        }
        DevIdEntry e;
        memset(&e, 0, sizeof(e));
        e.len = 4;
        const uint8_t four[4] = {0, 0, 0, 0};
        if (walk_idtab_set(ctx, 1, &e, four, sizeof(four), 0) == FABGPU_OK) (void)walk_idtab_set(ctx, 0, nullptr, nullptr, 0, 0);
    }
    {
        // what the first registrations of a channel's signers need (keytab_kernels.hip): a slab of key tables, the builder's room for
        // sixteen keys, its stream - a provider's FIRST block makes its signers eligible, and hipMalloc inside that pass cost more than the build
        std::lock_guard<std::mutex> bl(ctx->ktab_build_mu);
        std::lock_guard<std::mutex> kl(ctx->kmu);
        if (ctx->ktab_slabs.empty()) {
            int32_t* first = ktab_alloc_locked(ctx);
            if (first) ctx->ktab_free.push_back(first);
            else rc = FABGPU_ENOMEM;
        }
        const size_t in_bytes = (size_t)(64 + sizeof(void*)) * 16 * 2, scr_bytes = keytab_scratch_bytes(16) * 2;
        if (ctx->ktab_in_cap < in_bytes && hipMalloc(&ctx->d_ktab_in, in_bytes) == hipSuccess) ctx->ktab_in_cap = in_bytes;
        if (ctx->ktab_scr_cap < scr_bytes && hipMalloc(&ctx->d_ktab_scr, scr_bytes) == hipSuccess) ctx->ktab_scr_cap = scr_bytes;
        if (!ctx->stream_keytab) (void)hipStreamCreateWithFlags(&ctx->stream_keytab, hipStreamNonBlocking);
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    // the pass's four buffers at the largest layout a pass of this size can have (walk_layout.h walk_worst_case; never below the
    // estimates made here before the layout was written down: walk_preallocate_floor)
    const WalkSizes need_walk = walk_preallocate_sizes(n_tx, n_tuples);
    if (ctx->walk_env.ensure(need_walk.env) != FABGPU_OK) rc = FABGPU_ENOMEM;
    if (ctx->walk_tup.ensure(need_walk.tup) != FABGPU_OK) rc = FABGPU_ENOMEM;
    if (ctx->walk_pin.ensure(need_walk.pin) != FABGPU_OK) rc = FABGPU_ENOMEM;
    if (ctx->walk_map.ensure(need_walk.map) != FABGPU_OK) rc = FABGPU_ENOMEM;
    if (ctx->gscr.ensure(walk_gather_scratch_estimate(n_tx)) != FABGPU_OK) rc = FABGPU_ENOMEM;
    if (ctx->tailbuf.ensure((size_t)64 << 10) != FABGPU_OK) rc = FABGPU_ENOMEM;
    // The copy ENGINES, too.  The runtime creates a DMA queue the first time a copy of a direction needs one more of them - ~10 ms each,
    // on the calling thread, inside hipMemcpyAsync: measured (rocprofv3 --memory-copy-trace, profiles/r04_trace_first_memo_passes.txt) as
    // 11 ms of nothing on the device in front of the first memo-seeding passes' key copies (device -> pinned host, 8.5 MB, beside the
    // uploads of the other pass), four passes in a row - what round 3 booked as "pinned memo tables allocated on first overlap".  Copies
    // of both directions on all four pass streams at once, twice, make the runtime create them now.
    {
        const size_t piece = (size_t)4 << 20;
        void *d = nullptr, *h = nullptr;
        if (hipMalloc(&d, 4 * piece) == hipSuccess && hipHostMalloc(&h, 4 * piece, hipHostMallocPortable) == hipSuccess) {
            hipStream_t ss[4] = {ctx->stream, ctx->stream2, ctx->stream3, ctx->stream4};
            for (int rep = 0; rep < 2; rep++) {
                for (int k = 0; k < 4; k++) (void)hipMemcpyAsync((uint8_t*)h + k * piece, (uint8_t*)d + k * piece, piece, hipMemcpyDeviceToHost, ss[k]);
                for (int k = 0; k < 4; k++) (void)hipMemcpyAsync((uint8_t*)d + k * piece, (uint8_t*)h + k * piece, piece, hipMemcpyHostToDevice, ss[3 - k]);
                for (int k = 0; k < 4; k++) (void)hipStreamSynchronize(ss[k]);
            }
        }
        if (d) hipFree(d);
        if (h) hipHostFree(h);
    }
    return rc;
}

// Device -> pinned-host copies into the given buffers on the pass's streams, as a memo-seeding pass issues them; returns the longest
// time one hipMemcpyAsync call kept the calling thread (ms; < 0: a copy failed).  GPUCSP::Preallocate runs this beside an upload until
// the calls return at once: see walk_preallocate on the runtime's lazily created DMA queues.
double walk_warm_copies(fabgpu_ctx* ctx, void* const* pinned, const size_t* bytes, int n) {
    if (!ctx || !pinned || !bytes || n <= 0) return -1;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    if (!ctx->walk_tup.d || !ctx->walk_pin.h || ctx->walk_tup.cap < ((size_t)8 << 20)) return -1;
    hipStream_t ss[4] = {ctx->stream4, ctx->stream, ctx->stream2, ctx->stream3};
    uint8_t* dt = (uint8_t*)ctx->walk_tup.d;
    double worst = 0;
    auto timed = [&](hipError_t e, const std::chrono::steady_clock::time_point& t0) {
        worst = std::max(worst, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        return e == hipSuccess;
    };
    for (int i = 0; i < n; i++) {
        const size_t b = std::min(bytes[i], (size_t)8 << 20);
        // every kind of command a pass queues, on every stream it queues them on: fills (large, small), copies both ways (large, small),
        // an event recorded on one stream and awaited on the next
        for (int k = 0; k < 4; k++) {
            auto t0 = std::chrono::steady_clock::now();
            if (!timed(hipMemsetAsync(dt + ((size_t)k << 20), 0, (size_t)512 << 10, ss[k]), t0)) return -1;
            t0 = std::chrono::steady_clock::now();
            if (!timed(hipMemsetAsync(dt + ((size_t)k << 20), 0, 4, ss[k]), t0)) return -1;
            t0 = std::chrono::steady_clock::now();
            if (!timed(hipMemcpyAsync(dt + ((size_t)(4 + k) << 20), ctx->walk_pin.h, std::min<size_t>(ctx->walk_pin.cap, 80000), hipMemcpyHostToDevice, ss[k]), t0)) return -1;
            t0 = std::chrono::steady_clock::now();
            if (!timed(hipEventRecord(ctx->ev_w[k], ss[k]), t0)) return -1;
            t0 = std::chrono::steady_clock::now();
            if (!timed(hipStreamWaitEvent(ss[(k + 1) & 3], ctx->ev_w[k], 0), t0)) return -1;
        }
        auto t0 = std::chrono::steady_clock::now();
        if (!timed(hipMemcpyAsync(pinned[i], dt, b, hipMemcpyDeviceToHost, ss[i & 1]), t0)) return -1;
        t0 = std::chrono::steady_clock::now();
        // (the small ones that follow the keys in a pass: offsets, statuses)
        if (!timed(hipMemcpyAsync(pinned[i], dt, std::min<size_t>(b, 160000), hipMemcpyDeviceToHost, ss[(i + 1) & 1]), t0)) return -1;
    }
    for (int k = 0; k < 4; k++) (void)hipStreamSynchronize(ss[k]);
    return worst;
}

// A registered key's comb table built OUTSIDE the registration (6 ms of host arithmetic per key: the provider builds the tables of the
// identities a block made eligible side by side on its worker pool, then installs them one after the other so that every device hands
// out the same ids).
size_t key_table_words() { return KeyTab8::TABLE_WORDS; }
bool key_table_build(const uint8_t* qx32, const uint8_t* qy32, int32_t* out) {
    if (!qx32 || !qy32 || !out || !fabgpu_p256_pubkey_on_curve(qx32, qy32)) return false;
    u256 qx, qy;
    from_be32(qx, qx32);
    from_be32(qy, qy32);
    build_key_comb_table8(out, qx, qy);
    return true;
}
// TEST HOOK support: the first word at which the context's generator comb differs from the host builder's table (-1: identical; -2: error)
int64_t gtab_compare_with_host(fabgpu_ctx* ctx) {
    if (!ctx || !ctx->d_gtab) return -2;
    std::vector<int32_t> host(GTab16::TABLE_WORDS), dev(GTab16::TABLE_WORDS);
    build_g_comb_table16(host.data());
    DeviceGuard g(ctx->device);
    if (hipMemcpy(dev.data(), ctx->d_gtab, sizeof(int32_t) * GTab16::TABLE_WORDS, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    for (size_t i = 0; i < host.size(); i++)
        if (host[i] != dev[i]) return (int64_t)i;
    return -1;
}
// TEST HOOK support (FABGPU_FLAG_KEY_TABLES_16BIT): waits for the queued builds, then checks key `key_id`'s 16-bit comb against its 8-bit
// comb - T16[w][d] = T8[2 w][d] and T16[w][256 d] = T8[2 w + 1][d] for d = 1 .. 255, entry for entry (two tables built by different
// launches that must agree where they overlap).  Returns the number of 16-bit tables of the context; -1: the key has none; -2: error;
// -(1000 + w): window w disagrees.
int64_t key_tables16_check(fabgpu_ctx* ctx, uint32_t key_id) {
    if (!ctx) return -2;
    DeviceGuard g(ctx->device);
    void* t16 = nullptr;
    int32_t* t8 = nullptr;
    int64_t count = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->kmu);
        if (ctx->stream_keytab16 && hipStreamSynchronize(ctx->stream_keytab16) != hipSuccess) return -2;
        if (!ctx->kslots.live(key_id)) return -2;
        if (!ctx->k16_pending.empty()) k16_publish_locked(ctx);
        key_id = fab::KeySlots::slot_of(key_id);
        count = (int64_t)ctx->ktab16_count;
        t8 = ctx->ktabs[key_id];
        t16 = key_id < ctx->ktab16.size() ? ctx->ktab16[key_id] : nullptr;
    }
    if (!t16) return -1;
    const int32_t* slot[KTAB_STRIDE] = {nullptr, nullptr};
    if (hipMemcpy(slot, (const void*)(ctx->d_ktabs + KTAB_STRIDE * (size_t)key_id), sizeof(slot), hipMemcpyDeviceToHost) != hipSuccess) return -2;
    if (slot[0] != t8 || slot[1] != (const int32_t*)t16) return -2;       // the device's pointer array says the same
    std::vector<int32_t> h8(KeyTab8::TABLE_WORDS), e16(COMB_ENTRY_WORDS);
    if (hipMemcpy(h8.data(), t8, sizeof(int32_t) * KeyTab8::TABLE_WORDS, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    for (int w = 0; w < GTab16::WINDOWS; w++)
        for (uint32_t d = 1; d < 256; d++)
            for (int hi = 0; hi < 2; hi++) {
                const size_t at16 = GTab16::index(w, hi ? d << 8 : d), at8 = KeyTab8::index(2 * w + hi, d);
                if (hipMemcpy(e16.data(), (const int32_t*)t16 + at16, sizeof(int32_t) * COMB_ENTRY_WORDS, hipMemcpyDeviceToHost) != hipSuccess) return -2;
                if (memcmp(e16.data(), &h8[at8], sizeof(int32_t) * COMB_ENTRY_WORDS) != 0) return -(1000 + w);
            }
    return count;
}
int key_register_batch(fabgpu_ctx* ctx, int n, const uint8_t* qxy, uint32_t* key_ids) { return key_register_batch_dev(ctx, n, qxy, key_ids); }
// TEST HOOK support: the device's table of key `key_id` copied to the host (KeyTab8::TABLE_WORDS words)
int key_table_copy(fabgpu_ctx* ctx, uint32_t key_id, int32_t* out) {
    if (!ctx || !out) return FABGPU_EINVAL;
    int32_t* d = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->kmu);
        if (!ctx->kslots.live(key_id)) return FABGPU_EINVAL;
        d = ctx->ktabs[fab::KeySlots::slot_of(key_id)];
    }
    DeviceGuard g(ctx->device);
    return hip_to_rc(hipMemcpy(out, d, sizeof(int32_t) * KeyTab8::TABLE_WORDS, hipMemcpyDeviceToHost));
}
int key_register_many_prebuilt(fabgpu_ctx* const* ctxs, int n, const uint8_t* qx32, const uint8_t* qy32, const int32_t* table, uint32_t* key_ids) {
    return key_register_many_impl(ctxs, n, qx32, qy32, table, key_ids);
}

static std::mutex g_huge_mu;
static std::set<void*> g_huge_tables;      // memo tables that came from pinned_huge_alloc (the others from hipHostMalloc)
void* walk_pinned_alloc(fabgpu_ctx* ctx, size_t bytes) {
    if (!ctx || bytes == 0) return nullptr;
    DeviceGuard g(ctx->device);
    static const bool timing = getenv("FABGPU_PASS_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    // (portable: a memo table is recycled by whichever device of the provider's pool runs the next pass; on huge pages where the kernel
    //  grants them: the table is probed at random by every validator thread)
    void* p = pinned_huge_alloc(bytes);
    if (p) {
        std::lock_guard<std::mutex> lk(g_huge_mu);
        g_huge_tables.insert(p);
    } else if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {
        return nullptr;
    }
    if (timing) fprintf(stderr, "fabgpu: %.1f MB of pinned memory for a memo table in %.2f ms\n", bytes / 1e6, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return p;
}
void walk_pinned_free(fabgpu_ctx* ctx, void* p) {
    if (!ctx || !p) return;
    static const bool timing = getenv("FABGPU_PASS_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    DeviceGuard g(ctx->device);
    bool huge = false;
    {
        std::lock_guard<std::mutex> lk(g_huge_mu);
        huge = g_huge_tables.erase(p) != 0;
    }
    if (huge) pinned_huge_free(p);
    else (void)hipHostFree(p);
    if (timing) fprintf(stderr, "fabgpu: a memo table's pinned memory freed in %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// TEST HOOK support: the comb table of P-384 key `key_id` (or, generator != 0, the generator's) as it lies on the device
int p384_key_table_copy(fabgpu_ctx* ctx, uint32_t key_id, int generator, uint32_t* out) {
    if (!ctx || !out) return FABGPU_EINVAL;
    const uint32_t* d = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->k384_mu);
        d = generator ? ctx->d_gcomb384 : ctx->k384.table(key_id);
    }
    if (!d) return FABGPU_EINVAL;
    DeviceGuard g(ctx->device);
    return hip_to_rc(hipMemcpy(out, d, p384::CombTab384::TABLE_BYTES, hipMemcpyDeviceToHost));
}
// ... the 16-bit tables (FABGPU_FLAG_P384_KEY_TABLES_16BIT).  tables16_wait: every queued build waited for and published; how many
// 16-bit tables are live.  tables16_cap: the cap on live 16-bit tables, for the registrations that follow.  key_table16_check: after
// the same wait, *bad = the entries of the key's (generator != 0: the generator's) 16-bit table that are not T8[2 w][lo] + T8[2 w + 1][hi]
// as p384_keytab16_check_kernel recomputes them from the 8-bit table on the device, and out3 (three windows' words, or null) = windows
// 0, 11 and 23 as they lie on the device.  1: the key has no 16-bit table.
int p384_tables16_wait(fabgpu_ctx* ctx) {
    if (!ctx) return FABGPU_EINVAL;
    DeviceGuard g(ctx->device);
    std::lock_guard<std::mutex> lk(ctx->k384_mu);
    k384_poll16_locked(ctx, true);
    return (int)ctx->k384.n_tables16();
}
int p384_tables16_cap(fabgpu_ctx* ctx, uint32_t cap) {
    if (!ctx || cap > FABGPU_P384_MAX_TABLES16) return FABGPU_EINVAL;
    std::lock_guard<std::mutex> lk(ctx->k384_mu);
    ctx->k384_tab16_cap = cap;
    return FABGPU_OK;
}
int p384_key_table16_check(fabgpu_ctx* ctx, uint32_t key_id, int generator, uint64_t* bad, uint32_t* out3) {
    if (!ctx || !bad) return FABGPU_EINVAL;
    DeviceGuard g(ctx->device);
    const uint32_t *t8 = nullptr, *t16 = nullptr;
    unsigned long long* ctr = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->k384_mu);
        k384_poll16_locked(ctx, true);
        t8 = generator ? ctx->d_gcomb384 : ctx->k384.table(key_id);
        t16 = generator ? ctx->d_gcomb384x16 : ctx->k384.table16(key_id);
        ctr = ctx->d_k384_rows16;
    }
    if (!t8 || !t16 || !ctr) return 1;
    ctr++;                                         // (the second word of the counter's allocation is the hooks')
    hipStream_t st = ctx->stream_k384x16;
    hipError_t e = hipMemsetAsync(ctr, 0, sizeof(*ctr), st);
    if (e == hipSuccess) e = launch_p384_keytab16_check(t8, t16, ctr, st);
    unsigned long long v = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&v, ctr, sizeof(v), hipMemcpyDeviceToHost, st);
    const hipError_t drained = hipStreamSynchronize(st);
    if (e != hipSuccess || drained != hipSuccess) return hip_to_rc(e != hipSuccess ? e : drained);
    *bad = v;
    const uint32_t wins[3] = {0, 11, 23};
    for (int i = 0; out3 && i < 3; i++)
        if (int rc = hip_to_rc(hipMemcpy(out3 + (size_t)i * p384::CombTab384x16::WINDOW_WORDS, t16 + p384::CombTab384x16::index(wins[i], 0),
                                         p384::CombTab384x16::WINDOW_WORDS * 4, hipMemcpyDeviceToHost)))
            return rc;
    return FABGPU_OK;
}
// ... and a batch of keys (qxy: n x 96 bytes, every one a point of the curve) registered with one build
int p384_key_register_batch_hook(fabgpu_ctx* ctx, int n, const uint8_t* qxy, uint32_t* key_ids) {
    if (!ctx || n <= 0 || !qxy || !key_ids) return FABGPU_EINVAL;
    for (int i = 0; i < n; i++)
        if (!fabgpu_p384_pubkey_on_curve(qxy + 96 * (size_t)i, qxy + 96 * (size_t)i + 48)) return FABGPU_EINVAL;
    return p384_key_register_batch(ctx, n, qxy, key_ids);
}

}  // namespace fab
