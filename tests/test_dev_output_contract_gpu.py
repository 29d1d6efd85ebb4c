"""The OUTPUT CONTRACT of the device-resident entry points (include/fabgpu.h): after a _dev call that returned 0 and whose stream has
been synchronised, every one of the ceil(n / 64) verdict words is fully written with zeros at and above bit n, status[0, n) and
digests[0, n) hold the oracle's answers, and no other byte of the caller's memory has changed.

The host-pointer entries cannot show a breach - they copy n status bytes and ceil(n / 64) words out of a staging buffer, and
fabgpu.unpack_bits drops what lies at or above bit n - so here the kernels write straight into ONE torch.uint8 allocation
(dev_contract_image.Layout: every output region on a multiple of 256, at least 256 guard bytes in front, between and behind), every
case runs over the allocation filled with 0x00 and again filled with 0xFF, and the whole allocation is compared byte for byte with an
image built on the CPU from coracle / hashlib / idemix_oracle.  One context per kernel form (the kernel each reaches is named beside
it; read off launch_verify in csrc/kernels.hip, launch_idemix_nym_verify in csrc/idemix_kernels.hip, the keyed entries in
csrc/fabgpu_api.hip and the launchers in csrc/wide_kernels.hip / sha3_kernels.hip), each at the row counts where the rule for who owns
which part of the last verdict word changes."""
import ctypes
import hashlib

import numpy as np
import pytest

import coracle
import fabgpu
import test_batch_entry_points as bep
import test_described_entries_gpu as described
from dev_contract_image import ALIGN, FILLS, Layout, check, verdict_words
from idemix_common import be32, fixtures, make_batch as make_nym_batch

pytestmark = pytest.mark.gpu

# row counts around a wavefront's, a workgroup's and a verdict word's rows, per lane geometry
ONE_LANE = [1, 63, 64, 65, 255, 256, 257]                                  # 64 rows a wavefront, 256 a workgroup
TWO_LANES = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]         # 32 | 128; at 32 and 96 nobody's rows lie in the upper half of the last word
EIGHT_LANES = [1, 7, 8, 9, 55, 56, 57, 63, 64, 65, 71, 72]                 # 8 rows a wavefront = one byte of a verdict word
FOUR_LANES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]           # idemix: 16 | 64, and the challenge kernel's 8 | 32
NB = 257                                                                   # rows of a P-256 base: a case of n rows is its first n

F = fabgpu
# flags -> what a context made with them launches (V: fabgpu_p256_verify_batch_dev, also behind the SHA3-256 launch of the sha3 entries;
# H: fabgpu_sha256_p256_verify_batch_dev; K / HK: the keyed ones, the sha3 keyed entry behind its hash launch takes K's; N: idemix)
FORMS = {
    # V p256_verify_pair_kernel (n <= PAIR_TABLE_LDS_FROM: table in the global workspace), H sha256_p256_verify_pair_kernel,
    # K p256_wide_pre_kernel + p256_wide_post_kernel, HK the same around sha256_messages_coop_kernel,
    # N idemix_nym_verify_quad_kernel<.., false> beside idemix_nym_comb_quad_kernel (side stream), then idemix_nym_challenge_coop_kernel
    "default": 0,
    "pair-lds": F.FLAG_PAIR_TABLE_LDS,                                     # V p256_verify_pair_lds_kernel (helper waves, 512 threads)
    "pair-lds-solo": F.FLAG_PAIR_TABLE_LDS | F.FLAG_PAIR_SOLO,             # V p256_verify_pair_lds_solo_kernel
    # V p256_verify_kernel, H sha256_p256_verify_kernel, K p256_verify_keyed_kernel, HK sha256_p256_verify_keyed_kernel, N idemix_nym_verify_kernel
    "one-lane": F.FLAG_ONE_LANE_ONLY,
    "no-wide": F.FLAG_NO_WIDE,                                             # K p256_verify_keyed_pair_kernel, HK sha256_p256_verify_keyed_pair_kernel
    "nym-no-side-stream": F.FLAG_NYM_NO_SIDE_STREAM,                       # N quad_kernel<.., false> (fixed-base terms inside), challenge_coop_kernel
    "nym-fused": F.FLAG_NYM_FUSED_HASH,                                    # N idemix_nym_verify_quad_kernel<.., true>
    "nym-two-lanes": F.FLAG_NO_QUAD,                                       # N idemix_nym_verify_split_kernel
}


@pytest.fixture(scope="module")
def context_of():
    """form -> its context, made at first use: the two keys of bep.key_pool() registered as ids 0 and 1, the issuer MSP1OU1 as 0"""
    made = {}

    def of(form):
        if form not in made:
            c = fabgpu.Context(device=0, flags=FORMS[form])
            qx, qy = bep.key_pool()
            assert [c.key_register(qx[j].tobytes(), qy[j].tobytes()) for j in range(2)] == [0, 1]
            ipk = fixtures()["MSP1OU1"]["ipk"]
            assert c.idemix_issuer_register((be32(ipk.h_sk[0]), be32(ipk.h_sk[1])), (be32(ipk.h_rand[0]), be32(ipk.h_rand[1])), ipk.hash) == 0
            made[form] = c
        return made[form]

    yield of
    for c in made.values():
        c.close()


# ---- the harness ------------------------------------------------------------------------------------------------------------------------
def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def run_both_fills(layout, call):
    """call(p: region -> device address) launches on torch's current stream -> {fill: the whole allocation, read back}"""
    import torch
    images = {}
    for fill in FILLS:
        buf = torch.full((layout.total,), fill, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % ALIGN == 0
        call({k: buf.data_ptr() + layout.offset[k] for k in layout.names})
        torch.cuda.synchronize()
        images[fill] = buf.cpu().numpy()
    return images


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def assert_both_answers_in_the_last_word(want, n):
    last = np.asarray(want[(n - 1) // 64 * 64:n]) == 0
    assert last.size < 2 or (last.any() and not last.all()), n


def verdict_case(n, want, with_status, launch):
    """launch(verdict_bits, status or 0) -> the differences from the image the oracle's `want` asks for"""
    assert_both_answers_in_the_last_word(want, n)
    layout = Layout([("verdict_bits", (n + 63) // 64 * 8), ("status", n)])
    written = dict(verdict_bits=verdict_words(np.asarray(want[:n]) == 0))
    if with_status:
        written["status"] = np.asarray(want[:n], dtype=np.uint8)           # (without: the region stays as filled)
    images = run_both_fills(layout, lambda p: launch(p["verdict_bits"], p["status"] if with_status else 0))
    return ["n = %d: %s" % (n, x) for x in check(layout, images, written)]


def digest_case(n, want, launch):
    layout = Layout([("digests", 32 * n)])
    images = run_both_fills(layout, lambda p: launch(p["digests"]))
    return ["n = %d: %s" % (n, x) for x in check(layout, images, dict(digests=want[:n]))]


# ---- P-256: inputs and the oracle's answers, made once ----------------------------------------------------------------------------------
_p256 = {}


def _two_signers(n, seed, e):
    """every row signed by key i % 2 of bep.key_pool()"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    k[:, 0] &= 0x7F
    k[:, 31] |= 1
    ki = (np.arange(n) % 2).astype(np.uint32)
    qx, qy, r, s = (np.zeros((n, 32), np.uint8) for _ in range(4))
    P = coracle._p
    coracle.lib().oracle_p256_make_batch(ctypes.c_size_t(n), P(np.ascontiguousarray(bep.KEY_D[ki])), P(k), P(e.copy()), P(qx), P(qy), P(r), P(s))
    return dict(qx=qx, qy=qy, r=r, s=s, key_id=ki)


def _break(cols, broken):
    """r or s of the broken rows, four ways in turn (r + 1, the high-S mirror, the next row's s, r = 0): the message and its digest
    stay, so one set of columns serves the digest-given and the hashing entries"""
    s0 = cols["s"].copy()
    be = lambda v: np.frombuffer(int(v).to_bytes(32, "big"), dtype=np.uint8)
    for j, i in enumerate(np.nonzero(broken)[0]):
        if j % 4 == 0:
            cols["r"][i] = be((int.from_bytes(cols["r"][i].tobytes(), "big") + 1) % (1 << 256))
        elif j % 4 == 1:
            cols["s"][i] = be(coracle.N_INT - int.from_bytes(cols["s"][i].tobytes(), "big"))
        elif j % 4 == 2:
            cols["s"][i] = s0[(i + 1) % len(s0)]
        else:
            cols["r"][i] = 0


def p256_base(family):
    """family 'sha256' | 'sha3_256' -> NB messages, their digests, fresh-key and two-signer columns with about every third row broken -
    but row 64 k never and row 64 k + 1 always, so that both answers occur in every last word of two rows or more - and what coracle
    says of them; the device copies ride along (made at first use)"""
    if family in _p256:
        return _p256[family]
    rng = np.random.default_rng(256 + len(family))
    msgs = [bytes(rng.integers(0, 256, size=int(ln), dtype=np.uint8)) for ln in rng.integers(1, 150, size=NB)]
    arena, off = bep._arena(msgs)
    e = bep._hashes(family, msgs)
    broken = rng.random(NB) < 0.33
    broken[0::64], broken[1::64] = False, True
    broken[[5, 130]] = False                                                # (the two rows whose keys leave the curve below: nothing else wrong with them)
    fresh = {k: v for k, v in coracle.make_batch(NB, seed=300 + len(family), digests=e).items() if k != "kind"}
    fresh["qy"][[5, 130], 31] ^= 1                                          # two keys that are not on the curve
    keyed = _two_signers(NB, 400 + len(family), e)
    _break(fresh, broken)
    _break(keyed, broken)
    pool_qx, pool_qy = bep.key_pool()
    b = dict(arena=arena, off=off, e=e, fresh=fresh, keyed=keyed,
             want_fresh=coracle.verify_batch(fresh["qx"], fresh["qy"], e, fresh["r"], fresh["s"]),
             want_keyed=coracle.verify_batch(pool_qx[keyed["key_id"]], pool_qy[keyed["key_id"]], e, keyed["r"], keyed["s"]))
    for w in (b["want_fresh"], b["want_keyed"]):
        assert (w[0::64] == 0).all() and (w[1::64] != 0).all() and {0, 1, 2, 3} <= set(w.tolist())
    assert b["want_fresh"][5] == 4 and b["want_fresh"][130] == 4
    b["dev"] = dict(arena=up(arena), off=up(off), e=up(e), fresh={k: up(v) for k, v in fresh.items()}, keyed={k: up(v) for k, v in keyed.items()})
    _p256[family] = b
    return b


P256_ENTRIES = {   # entry -> (hash family of its base, keyed)
    "p256_verify_batch_dev": ("sha256", False), "sha256_p256_verify_batch_dev": ("sha256", False), "sha3_256_p256_verify_batch_dev": ("sha3_256", False),
    "p256_verify_batch_keyed_dev": ("sha256", True), "sha256_p256_verify_batch_keyed_dev": ("sha256", True),
    "sha3_256_p256_verify_batch_keyed_dev": ("sha3_256", True),
}


def p256_launch(ctx, entry, n, verdict_bits, status):
    family, keyed = P256_ENTRIES[entry]
    d = p256_base(family)["dev"]
    c = {k: v.data_ptr() for k, v in d["keyed" if keyed else "fresh"].items()}
    key = (c["key_id"],) if keyed else (c["qx"], c["qy"])
    if entry.startswith("p256_"):
        getattr(ctx, entry)(n, *key, d["e"].data_ptr(), c["r"], c["s"], verdict_bits, status, stream())
    else:
        getattr(ctx, entry)(n, d["arena"].data_ptr(), d["arena"].numel(), d["off"].data_ptr(), *key, c["r"], c["s"], verdict_bits, status, stream())


FRESH, KEYED = [e for e, (_, k) in P256_ENTRIES.items() if not k], [e for e, (_, k) in P256_ENTRIES.items() if k]
P256_CASES = ([("default", e, TWO_LANES) for e in FRESH] + [("one-lane", e, ONE_LANE) for e in FRESH + KEYED] +
              # (the table's home concerns the verify-only fresh-key kernel alone; the sha3 entry reaches it behind its hash launch)
              [(form, e, TWO_LANES) for form in ("pair-lds", "pair-lds-solo") for e in ("p256_verify_batch_dev", "sha3_256_p256_verify_batch_dev")] +
              [("default", e, EIGHT_LANES) for e in KEYED] + [("no-wide", e, TWO_LANES) for e in KEYED])


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("form,entry,sizes", P256_CASES, ids=["%s-%s" % c[:2] for c in P256_CASES])
def test_p256_entries_write_their_words_whole_and_nothing_else(context_of, form, entry, sizes, with_status):
    ctx = context_of(form)
    family, keyed = P256_ENTRIES[entry]
    want = p256_base(family)["want_keyed" if keyed else "want_fresh"]
    lines = []
    for n in sizes:
        lines += verdict_case(n, want, with_status, lambda v, s: p256_launch(ctx, entry, n, v, s))
    assert not lines, "%s on the %s context:\n%s" % (entry, form, "\n".join(lines))


def test_one_lane_grid_stride_at_one_row_more_than_the_slots_hold(context_of):
    """65 537 = VERIFY_MAX_WGS * VERIFY_BLOCK + 1 rows on the one-lane kernel: workgroup 0 walks a second tile for the one row of the
    1 025th word.  The rows are a fabgpu.synth_batch of 4 099 taken round and round (4 099 does not divide 65 536: the rows of a slot's
    two tiles differ); their statuses are the oracle's over those 4 099 - which the generator's kinds must agree with - and over the
    last 257 rows as they are sent."""
    ctx = context_of("one-lane")
    n, nb = 256 * 256 + 1, 4099
    base = fabgpu.synth_batch(nb, seed=65537, invalid_permille=300)
    st = coracle.verify_batch(base["qx"], base["qy"], base["e"], base["r"], base["s"])
    assert np.array_equal(st, np.array([0, 1, 1, 2, 1], dtype=np.uint8)[base["kind"]])
    idx = np.arange(n) % nb
    cols = {k: np.ascontiguousarray(base[k][idx]) for k in ("qx", "qy", "e", "r", "s")}
    want = st[idx]
    want[-257:] = coracle.verify_batch(*(cols[k][-257:] for k in ("qx", "qy", "e", "r", "s")))
    d = {k: up(v) for k, v in cols.items()}
    lines = verdict_case(n, want, True, lambda v, s: ctx.p256_verify_batch_dev(n, *(d[k].data_ptr() for k in ("qx", "qy", "e", "r", "s")), v, s, stream()))
    assert not lines, "\n".join(lines)


# ---- idemix pseudonym signatures --------------------------------------------------------------------------------------------------------
_nym = {}


def nym_case(n):
    if n not in _nym:
        msgs, cols, want = bep._nym_rows(n)
        arena, off = bep._arena(msgs)
        _nym[n] = dict(want=want, dev=[up(arena), up(off), up(np.zeros(n, dtype=np.uint32))] + [up(c) for c in cols])
    return _nym[n]


def nym_launch(ctx, n, verdict_bits, status):
    arena, off, iid, *cols = nym_case(n)["dev"]
    ctx.idemix_nym_verify_batch_dev(n, arena.data_ptr(), arena.numel(), off.data_ptr(), iid.data_ptr(), *(c.data_ptr() for c in cols), verdict_bits, status,
                                    stream())


NYM_CASES = [("default", FOUR_LANES, False), ("default", FOUR_LANES, True), ("nym-no-side-stream", FOUR_LANES, False), ("nym-fused", FOUR_LANES, False),
             ("nym-two-lanes", TWO_LANES, False), ("one-lane", ONE_LANE, False)]


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("form,sizes,side_after", NYM_CASES, ids=[c[0] + ("-side-after" if c[2] else "") for c in NYM_CASES])
def test_idemix_entry_writes_its_words_whole_and_nothing_else(context_of, form, sizes, side_after, with_status):
    """side_after: the test hook that orders the side launch behind the commitments, so that these compute the fixed-base terms themselves"""
    ctx = context_of(form)
    lines = []
    try:
        if side_after:
            ctx.test_nym_side_after(True)
        for n in sizes:
            lines += verdict_case(n, nym_case(n)["want"], with_status, lambda v, s: nym_launch(ctx, n, v, s))
    finally:
        if side_after:
            ctx.test_nym_side_after(False)
    assert not lines, "idemix_nym_verify_batch_dev on the %s context:\n%s" % (form, "\n".join(lines))


# ---- hash-only ----------------------------------------------------------------------------------------------------------------------------
# fabgpu_sha256_batch_dev -> launch_sha256_batch: up to SHA_COOP_MAX = 2 048 messages sha256_messages_coop_kernel, eight lanes a message -
# <1> (one wavefront a workgroup) while the launch has fewer than COOP_WG_WAVES = 4 wavefronts of eight, i.e. up to 24 messages, <4>
# from 25 on; from 2 049 on sha256_mixed_kernel in workgroups of 64: one lane a message, but the first eight messages of a group of 64
# that are longer than max(2 048, 1.25 x the mean) on eight lanes in the scan workgroups.  fabgpu_sha3_256_batch_dev -> sha3_256_batch_kernel,
# one lane a message in workgroups of 256, whatever n.
SHA256_SIZES = [1, 7, 8, 9, 24, 25, 63, 64, 65, 2048, 2049]
SHA3_SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257]
N_MIXED = 2057                                             # 32 groups of 64 and a last one of 9
LONG_ROWS = list(range(3, 12)) + [2050, 2056]              # nine in the first group (eight go to the scan wavefront, the ninth stays), two in the partial last one
_hash = {}


def hash_base(long_rows=()):
    """2 049 (long_rows: N_MIXED) messages: those of the sha256 base round and round, each with its row number behind it, the long ones
    2 100 bytes and more -> arena, offsets, hashlib's digests under both families, the device copies"""
    key = tuple(long_rows)
    if key not in _hash:
        n = N_MIXED if long_rows else max(SHA256_SIZES)
        rng = np.random.default_rng(2049 + len(key))
        short = [bytes(rng.integers(0, 256, size=int(ln), dtype=np.uint8)) for ln in rng.integers(0, 150, size=NB)]
        msgs = [short[i % NB] + i.to_bytes(2, "big") for i in range(n)]
        for j, i in enumerate(long_rows):
            msgs[i] = bytes(rng.integers(0, 256, size=2100 + 37 * j, dtype=np.uint8))
        arena, off = bep._arena(msgs)
        _hash[key] = dict(n=n, msgs=msgs, arena_bytes=arena.size, dev=(up(arena), up(off)),
                          sha256=bep._hashes("sha256", msgs), sha3_256=bep._hashes("sha3_256", msgs))
    return _hash[key]


@pytest.mark.parametrize("family,sizes", [("sha256", SHA256_SIZES), ("sha3_256", SHA3_SIZES)])
def test_hash_entries_write_n_digest_rows_and_nothing_else(context_of, family, sizes):
    ctx = context_of("default")
    h = hash_base()
    arena, off = h["dev"]
    f = getattr(ctx, family + "_batch_dev")
    lines = []
    for n in sizes:
        lines += digest_case(n, h[family], lambda dig: f(n, arena.data_ptr(), arena.numel(), off.data_ptr(), dig, stream()))
    assert not lines, "%s_batch_dev:\n%s" % (family, "\n".join(lines))


def test_sha256_mixed_kernel_with_long_messages_in_a_partial_last_group(context_of):
    ctx = context_of("default")
    h = hash_base(LONG_ROWS)
    n = h["n"]
    mean = h["arena_bytes"] // n
    long_over = max(2048, mean + mean // 4)                # launch_sha256_mixed's threshold over the arena_bytes handed in below
    lens = np.array([len(m) for m in h["msgs"]])
    assert n > 2048 and n % 64 == 9 and np.nonzero(lens > long_over)[0].tolist() == LONG_ROWS and lens[lens <= long_over].max() < 160
    arena, off = h["dev"]
    assert arena.numel() == h["arena_bytes"]
    lines = digest_case(n, h["sha256"], lambda dig: ctx.sha256_batch_dev(n, arena.data_ptr(), arena.numel(), off.data_ptr(), dig, stream()))
    assert not lines, "\n".join(lines)


# ---- the described batch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("keyed", [False, True], ids=["fresh", "keyed"])
@pytest.mark.parametrize("form", ["default", "no-wide", "one-lane"])
def test_described_batch_guards_every_buffer_it_names(context_of, form, keyed, n, with_status):
    """fabgpu_identity_verify_batch_dev over the 65-row case of test_described_entries_gpu.py (two prefixes, spans, a message in the
    tail's place, an empty one; n = 1: its row 1 alone) with `digests`, one gathered message and two pseudonym riders.  Every buffer the
    description names lies in the guarded allocation: the verdict words, the statuses, the digests and the gathered digest hold the
    reference's bytes; mid_scratch and gather_scratch are the call's to use, the bytes around them are not; and the riders' outputs stay
    as filled - the _dev entry leaves pseudonym signatures to fabgpu_idemix_nym_verify_batch_dev (fabgpu.h).
    default: sha256_p256_verify_pair_kernel / keyed p256_wide_pre + sha256_messages_coop + p256_wide_post; no-wide: keyed
    sha256_p256_verify_keyed_pair_kernel; one-lane: sha256_p256_verify_kernel / sha256_p256_verify_keyed_kernel; behind each
    gather_spans_kernel + sha256_messages_coop_kernel."""
    ctx = context_of(form)
    c = described.big_of("p256")
    rows = slice(1, 2) if n == 1 else slice(0, described.NE)
    want = c.status[rows]
    assert want[0] == 0 if n == 1 else ((want[:64] == 0).any() and (want[:64] != 0).any())   # (the last word of 65 rows holds one)
    arena = np.zeros(c.tail_base + 80 + 64, dtype=np.uint8)                 # a _dev caller places the tail's bytes in its arena, at tail_base
    arena[:c.arena.size] = c.arena
    arena[c.tail_base:c.tail_base + c.tail.size] = c.tail
    narena, noff, iid, ncols, _ = make_nym_batch(described.register_issuers(ctx), 2, 4).arrays()
    assert c.arena.size + narena.size <= c.tail_base
    arena[c.arena.size:c.arena.size + narena.size] = narena                 # the riders' messages behind the ECDSA ones
    nspans = np.stack([noff[:-1], noff[1:]], axis=1).astype(np.uint32) + np.uint32(c.arena.size)
    gather = described.GATHER
    total = sum(gather[2 * k + 1] - gather[2 * k] for k in range(3))
    two = lambda a: np.ascontiguousarray(a.reshape(described.NE, -1)[rows])
    t = dict(arena=up(arena), off=up(two(c.off)), pre_off=up(c.pre_off), pre_idx=up(two(c.pre_idx)), r=up(two(c.r)), s=up(two(c.s)),
             qx=up(two(c.qx)), qy=up(two(c.qy)), g=up(np.array(gather, dtype=np.uint32)), goff=up(np.array([0, total], dtype=np.uint32)),
             nsp=up(nspans), niss=up(iid), nf=up(np.concatenate([x.reshape(-1, 32) for x in ncols], axis=0)))
    if keyed:
        ids = [ctx.key_register(q[0].to_bytes(32, "big"), q[1].to_bytes(32, "big")) for q in c.keys]
        t["key_id"] = up(two(np.array([ids[k] for k in c.kidx], dtype=np.uint32)))
    layout = Layout([("verdict_bits", (n + 63) // 64 * 8), ("status", n), ("digests", 32 * n), ("gather_digests", 32), ("nym_verdict_bits", 8),
                     ("nym_status", 2), ("mid_scratch", 2 * 32), ("gather_scratch", total + 64)])
    written = dict(verdict_bits=verdict_words(want == 0), digests=c.digests[rows],
                   gather_digests=np.frombuffer(hashlib.sha256(bytes(c.arena[3:303]) + bytes(c.arena[310:350])).digest(), dtype=np.uint8))
    if with_status:
        written["status"] = want

    def call(p):
        b = fabgpu._IdBatch()
        b.n, b.flags = n, fabgpu.IDB_SPANS
        b.arena, b.arena_bytes, b.off = t["arena"].data_ptr(), t["arena"].numel(), t["off"].data_ptr()
        b.n_prefixes, b.pre_off, b.pre_idx = 2, t["pre_off"].data_ptr(), t["pre_idx"].data_ptr()
        b.r, b.s = t["r"].data_ptr(), t["s"].data_ptr()
        if keyed:
            b.key_id = t["key_id"].data_ptr()
        else:
            b.qx, b.qy = t["qx"].data_ptr(), t["qy"].data_ptr()
        b.verdict_bits, b.status, b.digests = p["verdict_bits"], p["status"] if with_status else None, p["digests"]
        b.n_gather, b.gather_spans, b.gather_off, b.gather_digests = 1, t["g"].data_ptr(), t["goff"].data_ptr(), p["gather_digests"]
        b.gather_scratch, b.gather_scratch_bytes = p["gather_scratch"], total + 64
        b.n_nym, b.nym_off, b.nym_issuer, b.nym_fields = 2, t["nsp"].data_ptr(), t["niss"].data_ptr(), t["nf"].data_ptr()
        b.nym_verdict_bits, b.nym_status = p["nym_verdict_bits"], p["nym_status"]
        ctx.identity_verify_batch_dev(b, p["mid_scratch"], stream())

    lines = check(layout, run_both_fills(layout, call), written, scratch=("mid_scratch", "gather_scratch"))
    assert not lines, "\n".join(lines)
