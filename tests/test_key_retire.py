"""Retiring registered P-256 keys (fabgpu_p256_key_unregister; fabric-mod_amd/csrc/key_slots.h): a retired key's slot and
tables serve later registrations, under another id, and an id never means two keys - a tuple that names a retired id gets that
key's own verdict or status 4, never another key's.  Verdicts are compared with the CPU oracle and with the fresh-key call on the same
tuples."""
import ctypes

import numpy as np
import pytest

import coracle
import fabgpu
from test_gpu_parity import ctx  # noqa: F401  (the parity file's contexts: auto, one-lane, pair-table-lds, pair-table-global, no-wide)

pytestmark = pytest.mark.gpu

SLOT_BITS = 12
ST_USE_SW = 4            # what an out-of-range key id yields (include/fabgpu.h)
# a full wavefront plus one tuple on one lane each, on two lanes each, on eight lanes each
SIZES = (65, 33, 9)


@pytest.fixture(scope="module")
def one_lane_ctx():
    """Registered keys on the ONE-lane keyed kernel at small sizes: neither two nor eight lanes per signature."""
    c = fabgpu.Context(device=0, flags=fabgpu.FLAG_ONE_LANE_ONLY | fabgpu.FLAG_NO_WIDE)
    yield c
    c.close()


_pools = {}


def _pool(seed, n, nkeys=4):
    """n valid tuples over nkeys signers (tuple i by signer i mod nkeys), followed by one tampered twin per signer (its first tuple, one
    message bit flipped), and the oracle's statuses for all of them.  Made once per (seed, n) and never changed."""
    if (seed, n) not in _pools:
        rng = np.random.default_rng(seed)

        def scalars(m):
            a = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
            a[:, 0] &= 0x7F
            a[:, 31] |= 1
            return a
        dpool = scalars(nkeys)                                                  # (first draw: the signers depend on the seed only)
        ki = (np.arange(n) % nkeys).astype(np.uint32)
        msgs = [bytes(rng.integers(0, 256, size=int(ln), dtype=np.uint8)) for ln in rng.integers(1, 200, size=n)]
        off0 = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)
        arena0 = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8)
        e0 = np.ascontiguousarray(coracle.sha256_batch(arena0, off0))
        d, k = np.ascontiguousarray(dpool[ki]), scalars(n)
        cols = {c: np.zeros((n, 32), np.uint8) for c in ("qx", "qy", "r", "s")}
        P = coracle._p
        coracle.lib().oracle_p256_make_batch(ctypes.c_size_t(n), P(d), P(k), P(e0), P(cols["qx"]), P(cols["qy"]), P(cols["r"]), P(cols["s"]))
        twins = [bytes([msgs[j][0] ^ 1]) + msgs[j][1:] for j in range(nkeys)]
        firsts = list(range(nkeys))
        msgs += twins
        off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)
        arena = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8).copy()
        e = np.ascontiguousarray(coracle.sha256_batch(arena, off))
        cols = {c: np.ascontiguousarray(np.concatenate([v, v[firsts]])) for c, v in cols.items()}
        ki = np.concatenate([ki, ki[firsts]])
        want = coracle.verify_batch(cols["qx"], cols["qy"], e, cols["r"], cols["s"])
        assert (want[:n] == 0).all() and (want[n:] != 0).all()
        pool_qx, pool_qy = cols["qx"][:nkeys].copy(), cols["qy"][:nkeys].copy()
        for a in (arena, off, e, ki, want, pool_qx, pool_qy, *cols.values()):
            a.setflags(write=False)
        _pools[(seed, n)] = dict(arena=arena, off=off, e=e, key_index=ki, want=want, pool_qx=pool_qx, pool_qy=pool_qy, **cols)
    return _pools[(seed, n)]


def _key(p, j):
    return p["pool_qx"][j].tobytes(), p["pool_qy"][j].tobytes()


def _dev(ctx, p, ids, fused, stream=None):
    """the _dev entry points on a torch stream; returns the device tensors (not synchronised)"""
    import torch
    n = len(ids)
    t = {k: torch.from_numpy(np.array(v)).cuda() for k, v in dict(arena=p["arena"], off=p["off"].view(np.int32), e=p["e"], r=p["r"], s=p["s"],
                                                                                 ids=ids.view(np.int32)).items()}
    words = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    status = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = stream or torch.cuda.current_stream()
    if fused:
        ctx.sha256_p256_verify_batch_keyed_dev(n, t["arena"].data_ptr(), t["arena"].numel(), t["off"].data_ptr(), t["ids"].data_ptr(), t["r"].data_ptr(),
                                               t["s"].data_ptr(), words.data_ptr(), status.data_ptr(), s.cuda_stream)
    else:
        ctx.p256_verify_batch_keyed_dev(n, t["ids"].data_ptr(), t["e"].data_ptr(), t["r"].data_ptr(), t["s"].data_ptr(), words.data_ptr(), status.data_ptr(),
                                        s.cuda_stream)
    return t, words, status


def _all_entry_points(ctx, p, ids):
    """(bits, status) of the tuples of p under `ids` from the plain, the fused and the two device-resident keyed entry points"""
    import torch
    n = len(ids)
    out = [ctx.p256_verify_batch_keyed(ids, p["e"], p["r"], p["s"]),
           ctx.sha256_p256_verify_batch_keyed(p["arena"], p["off"], ids, p["r"], p["s"])]
    for fused in (False, True):
        _, words, status = _dev(ctx, p, ids, fused)
        torch.cuda.synchronize()
        out.append((fabgpu.unpack_bits(words.cpu().numpy().view(np.uint64), n), status.cpu().numpy()))
    return out


def _retire_and_reuse(ctx, seed):
    pools = {n: _pool(seed, n - 4) for n in SIZES}                            # (n tuples in all: the four twins are among them)
    p0 = pools[SIZES[0]]
    assert all((pools[n]["pool_qx"] == p0["pool_qx"]).all() for n in SIZES)      # (the signers depend on the seed only)
    base = ctx.key_count()
    a, b, c = (ctx.key_register(*_key(p0, j)) for j in range(3))
    assert ctx.key_count() == base + 3
    assert ctx.key_unregister(b) is True and ctx.key_unregister(b) is False      # idempotent
    assert ctx.key_lookup(*_key(p0, 1)) is None and ctx.key_count() == base + 2
    assert ctx.key_lookup(*_key(p0, 0)) == a and ctx.key_lookup(*_key(p0, 2)) == c
    d = ctx.key_register(*_key(p0, 3))
    # the retired slot, the next generation: another id than the old tenant's
    assert d == b + (1 << SLOT_BITS) and d & ((1 << SLOT_BITS) - 1) == b & ((1 << SLOT_BITS) - 1)
    assert ctx.key_count() == base + 3 and ctx.key_lookup(*_key(p0, 3)) == d
    st = ctx.key_table_stats()
    assert st["live"] == base + 3 and st["reused"] >= 1 and st["parked"] == 0
    by_signer = np.array([a, b, c, d], dtype=np.uint32)
    for n, p in pools.items():
        ids = by_signer[p["key_index"]]
        stale = p["key_index"] == 1
        assert stale.any() and (~stale).sum() >= 6
        want = np.where(stale, ST_USE_SW, p["want"]).astype(np.uint8)
        fresh_bits, fresh_st = ctx.p256_verify_batch(p["qx"], p["qy"], p["e"], p["r"], p["s"])
        assert (fresh_st == p["want"]).all()
        for which, (bits, stt) in enumerate(_all_entry_points(ctx, p, ids)):
            assert (stt == want).all(), (n, which, stt.tolist(), want.tolist())
            assert (bits == (want == 0)).all(), (n, which)
            assert (bits[~stale] == fresh_bits[~stale]).all() and not bits[stale].any()
    return by_signer


def test_retire_and_reuse_under_every_context_of_the_parity_file(ctx):
    _retire_and_reuse(ctx, seed=7001)


def test_retire_and_reuse_on_the_one_lane_keyed_kernel(one_lane_ctx):
    _retire_and_reuse(one_lane_ctx, seed=7002)


def test_a_stale_id_before_its_slot_is_reused(ctx):
    """Between the retirement and the reuse the device still shows the key: every row answers either the key's correct verdict or
    status 4 - one of the two for the whole call, since nothing changes the slot in between - and a replacement then closes the gap."""
    p = _pool(7003, 29)
    ids4 = [ctx.key_register(*_key(p, j)) for j in range(4)]
    assert ctx.key_unregister(ids4[2]) is True
    ids = np.array(ids4, dtype=np.uint32)[p["key_index"]]
    stale = p["key_index"] == 2
    as_key = p["want"]
    as_sw = np.where(stale, ST_USE_SW, p["want"]).astype(np.uint8)
    for bits, stt in _all_entry_points(ctx, p, ids):
        assert (stt == as_key).all() or (stt == as_sw).all(), stt.tolist()
        assert (bits == (stt == 0)).all()
    again = ctx.key_register(*_key(p, 2))                                      # the same key comes back: its old slot, a new id
    assert again == ids4[2] + (1 << SLOT_BITS)
    ids_new = np.array(ids4[:2] + [again, ids4[3]], dtype=np.uint32)[p["key_index"]]
    for bits, stt in _all_entry_points(ctx, p, ids_new):
        assert (stt == p["want"]).all() and (bits == (p["want"] == 0)).all()
    for bits, stt in _all_entry_points(ctx, p, ids):                           # ... and the old id is dead for good
        assert (stt == as_sw).all() and (bits == (as_sw == 0)).all()


def test_a_batch_in_flight_when_its_key_retires_and_is_replaced(ctx):
    """A keyed _dev batch is queued on a stream; its keys are retired and other keys registered in their slots before anybody waits for
    the stream.  The batch answers for the keys it named."""
    import torch
    n = 3000
    p = _pool(7004, n)
    q = _pool(7005, 9)
    ids4 = np.array([ctx.key_register(*_key(p, j)) for j in range(4)], dtype=np.uint32)
    s = torch.cuda.Stream()
    keep, words, status = _dev(ctx, p, ids4[p["key_index"]], fused=True, stream=s)
    for j in range(4):
        assert ctx.key_unregister(int(ids4[j])) is True
    new4 = np.array([ctx.key_register(*_key(q, j)) for j in range(4)], dtype=np.uint32)
    assert sorted(new4.tolist()) == sorted((ids4 + (1 << SLOT_BITS)).tolist())
    s.synchronize()
    assert (status.cpu().numpy() == p["want"]).all()
    assert (fabgpu.unpack_bits(words.cpu().numpy().view(np.uint64), len(p["want"])) == (p["want"] == 0)).all()
    bits, stt = ctx.p256_verify_batch_keyed(new4[q["key_index"]], q["e"], q["r"], q["s"])
    assert (stt == q["want"]).all() and (bits == (q["want"] == 0)).all()
    del keep


def test_16_bit_tables_are_retired_and_rebuilt():
    c16 = fabgpu.Context(device=0, flags=fabgpu.FLAG_KEY_TABLES_16BIT)
    c8 = fabgpu.Context(device=0)
    try:
        p = _pool(7006, 65)
        a = c16.key_register(*_key(p, 0))
        assert c16.test_key_tables16(a) == 1                                   # waits for the build; cross-checks the table
        assert c16.key_table_stats()["live_16bit"] == 1
        assert c16.key_unregister(a) is True
        assert c16.key_table_stats()["live_16bit"] == 0
        b = c16.key_register(*_key(p, 1))
        assert b == a + (1 << SLOT_BITS)
        assert c16.test_key_tables16(b) == 1                                   # the reused slot's key has a 16-bit table of its own
        st = c16.key_table_stats()
        assert (st["live"], st["live_16bit"], st["reused"]) == (1, 1, 1)
        # a wavefront of the new key's tuples (16-bit path) and one that also names the stale id (falls back): the 8-bit context's answers
        b8 = c8.key_register(*_key(p, 1))
        sel = np.nonzero(p["key_index"] == 1)[0]
        for n_rep in (1, 8):
            rows = np.tile(sel, n_rep)
            got = c16.p256_verify_batch_keyed(np.full(len(rows), b, dtype=np.uint32), p["e"][rows], p["r"][rows], p["s"][rows])
            ref = c8.p256_verify_batch_keyed(np.full(len(rows), b8, dtype=np.uint32), p["e"][rows], p["r"][rows], p["s"][rows])
            assert (got[1] == ref[1]).all() and (got[0] == ref[0]).all() and (got[1] == p["want"][rows]).all()
        rows = np.nonzero(p["key_index"] <= 1)[0]
        ids = np.where(p["key_index"][rows] == 1, b, a).astype(np.uint32)
        bits, stt = c16.p256_verify_batch_keyed(ids, p["e"][rows], p["r"][rows], p["s"][rows])
        want = np.where(p["key_index"][rows] == 1, p["want"][rows], ST_USE_SW)
        assert (stt == want).all() and (bits == (want == 0)).all()
    finally:
        c16.close()
        c8.close()


# ---- the provider: an evicted identity's table goes too (retire_evicted_keys) -----------------------------------------------------------
def _churn_blocks():
    """twelve small blocks, each signed by four identities nobody has met: its creator and its three endorsers"""
    import blockgen
    if "churn" not in _pools:
        who = blockgen.fresh_identities(48, 515)
        _pools["churn"] = ([blockgen.endorser_block(6, 900 + k, creators=[who[4 * k]], endorsers=who[4 * k + 1:4 * k + 4], number=k + 1)[0] for k in range(12)], who)
    return _pools["churn"]


def _ctx_lookup(csp, d, qxy):
    kid = ctypes.c_uint32(0)
    rc = csp._L.fabgpu_p256_key_lookup(csp._L.fabgpu_csp_ctx_of(csp._h, d), qxy[:32], qxy[32:], ctypes.byref(kid))
    assert rc in (0, 1)
    return int(kid.value) if rc == 0 else None


@pytest.fixture(scope="module")
def host_answers():
    blocks, _ = _churn_blocks()
    host = fabgpu.GPUCSP(device=0, pass_device_walk=-1)
    try:
        return [{k: np.array(v) for k, v in fabgpu.preverify_block2(host, blk, block_seq=k).items() if k in ("tx_flags", "tuple_status")} for k, blk in enumerate(blocks)]
    finally:
        host.close()


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]])
def test_provider_retires_the_tables_of_evicted_identities(devices, host_answers):
    import blockgen
    blocks, who = _churn_blocks()
    csp = fabgpu.GPUCSP(devices=devices, retire_evicted_keys=1)
    try:
        assert csp.get_option("retire_evicted_keys") == 1
        csp._L.fabgpu_csp_identity_cache_limits(csp._h, 4, 2, 1)
        seq = 0
        for k, blk in enumerate(blocks):
            for _ in range(2):                                                 # (the second pass meets identities the first one registered)
                got = fabgpu.preverify_block2(csp, blk, block_seq=seq)
                seq += 1
                assert np.array_equal(got["tx_flags"], host_answers[k]["tx_flags"]) and (got["tx_flags"] == 0).all()
                assert np.array_equal(got["tuple_status"], host_answers[k]["tuple_status"])
                for d in range(len(devices)):
                    st = csp.key_table_stats(d)
                    assert csp.key_count(d) == st["live"] <= 2 + st["draining"], (k, d, st)
        per_dev = [csp.key_table_stats(d) for d in range(len(devices))]
        for st in per_dev:
            assert st["reused"] >= 8 and st["slots_used"] <= 4 and st["retired"] >= 8, st
            assert (st["live"], st["reused"], st["slots_used"]) == (per_dev[0]["live"], per_dev[0]["reused"], per_dev[0]["slots_used"])
        # the devices of the pool agree on every id after the churn
        found = 0
        for ident, d32 in who:
            ids = [_ctx_lookup(csp, d, blockgen._pubkey(d32)) for d in range(len(devices))]
            assert len(set(ids)) == 1, ids
            found += ids[0] is not None
        assert found == per_dev[0]["live"] and 1 <= found <= 2
    finally:
        csp.close()


def test_provider_without_the_option_keeps_every_table(host_answers):
    blocks, _ = _churn_blocks()
    csp = fabgpu.GPUCSP(device=0)
    try:
        assert csp.get_option("retire_evicted_keys") == 0
        csp._L.fabgpu_csp_identity_cache_limits(csp._h, 4, 2, 1)
        counts = []
        for k, blk in enumerate(blocks):
            got = fabgpu.preverify_block2(csp, blk, block_seq=k)
            assert np.array_equal(got["tx_flags"], host_answers[k]["tx_flags"])
            counts.append(csp.key_count())
        st = csp.key_table_stats()
        assert counts == sorted(counts) and counts[-1] > 2 and counts[-1] == st["slots_used"] and st["reused"] == 0 and st["retired"] == 0, (counts, st)
    finally:
        csp.close()


def test_passes_that_overlap_evictions_and_registrations_never_call_a_valid_transaction_invalid(host_answers):
    """Two callers on a pool of two contexts and a cache of four identities: one passes the same block over and over, the other passes
    eleven other blocks, each of which evicts the first block's identities, retires their tables and registers its own in their slots.
    A pass may meet an id that was retired after it read the identity table: such a tuple is "ask bccsp/sw" (tuple status 6, tx flag 4),
    never "invalid" - every other tuple and transaction answers as on the host route."""
    import threading
    TX_NEEDS_SW, TUPLE_NEEDS_SW = 4, 6                                          # (block_prepass.h)
    blocks, _ = _churn_blocks()
    csp = fabgpu.GPUCSP(devices=[0, 0], retire_evicted_keys=1)
    errs, undecided = [], [0]
    try:
        csp._L.fabgpu_csp_identity_cache_limits(csp._h, 4, 2, 1)

        def caller(which, rounds):
            try:
                for j in range(rounds):
                    k = 0 if which == 0 else 1 + j % 11
                    got = fabgpu.preverify_block2(csp, blocks[k], block_seq=1000 * which + j)
                    want = host_answers[k]
                    ts, tf = np.asarray(got["tuple_status"]), np.asarray(got["tx_flags"])
                    assert ((ts == want["tuple_status"]) | (ts == TUPLE_NEEDS_SW)).all(), (which, j, ts.tolist())
                    assert ((tf == want["tx_flags"]) | (tf == TX_NEEDS_SW)).all(), (which, j, tf.tolist())
                    undecided[0] += int((ts == TUPLE_NEEDS_SW).sum())
            except Exception as e:                                               # noqa: BLE001
                errs.append(repr(e))
        th = [threading.Thread(target=caller, args=(w, 44)) for w in (0, 1)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        st = csp.key_table_stats(0)
        assert st["reused"] >= 8 and st["live"] <= 2 + st["draining"], st         # the churn did happen
        print("tuples left to bccsp/sw: %d" % undecided[0])
    finally:
        csp.close()
