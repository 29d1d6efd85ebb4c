"""Registered P-384 keys on the device: the comb tables p384_keytab_kernels.hip builds, the keyed kernel of p384_keyed_kernels.hip and
the C entries around them, against Python integers (p384_ref.py through p384_keyed_cases.py), the host builder and the fresh-key
entries on the same tuples."""
import hashlib
import random

import numpy as np
import pytest

import fabgpu
import p384_keyed_cases as C
import p384_ref as R

pytestmark = pytest.mark.gpu
N = R.N


@pytest.fixture(scope="module")
def ctx():
    c = fabgpu.Context(device=0)
    yield c
    c.close()


def _b(q):
    return R.b48(q[0]), R.b48(q[1])


@pytest.fixture(scope="module")
def ids(ctx):
    """key -> id: the first two of the five keys registered in ONE build, the others and G, -G one by one"""
    ks = [q for _d, q in C.keys()]
    out = dict(zip(ks[:2], fabgpu.p384_key_register_batch(ctx, [_b(q) for q in ks[:2]])))
    for q in ks[2:] + [R.G, R.neg(R.G)]:
        out[q] = ctx.p384_key_register(*_b(q))
    assert sorted(out.values()) == list(range(7)) and ctx.p384_key_count() == 7
    return out


def _cols(rows, which=(2, 3, 4)):
    return [np.frombuffer(b"".join(R.b48(t[k]) for t in rows), dtype=np.uint8).copy() for k in which]


def _kid(ids, rows):
    return np.array([ids[(t[0], t[1])] for t in rows], dtype=np.uint32)


def test_device_built_tables_equal_the_host_builder_byte_for_byte(ctx, ids):
    for q in [q for _d, q in C.keys()[:2]]:                      # the two keys of one batch
        dev = fabgpu.p384_comb_device(ctx, ids[q])
        host = fabgpu.p384_comb_host(*_b(q))
        assert dev.tobytes() == host.tobytes(), np.nonzero(dev != host)[0][:4]
    assert fabgpu.p384_comb_device(ctx, generator=True).tobytes() == fabgpu.p384_comb_host().tobytes()
    assert fabgpu.p384_comb_device(ctx, ids[R.G]).tobytes() == fabgpu.p384_comb_host().tobytes()      # G as a key: the same table
    st = ctx.p384_key_table_stats()
    assert st["live"] == 7 and st["slots_used"] == 7 and st["bytes_held"] >= 8 * 4 * fabgpu.P384_COMB_WORDS


def test_registration_rules(ctx, ids):
    q = C.keys()[0][1]
    assert ctx.p384_key_register(*_b(q)) == ids[q] and ctx.p384_key_lookup(*_b(q)) == ids[q]      # twice: the first id
    with pytest.raises(fabgpu.FabgpuError):
        ctx.p384_key_register(R.b48(q[0]), R.b48((q[1] + 1) % R.P))                              # off the curve
    with pytest.raises(fabgpu.FabgpuError):
        ctx.p384_key_register(R.b48(R.P), R.b48(q[1]))
    assert ctx.p384_key_count() == 7


def _dev_words(ctx, n, cols, kid=None):
    """the _dev entry into device words pre-filled with ones and one guard word: (words, status, guard word, guard status byte)"""
    import torch
    dev = [torch.from_numpy(c).cuda() for c in cols]
    nw = (n + 63) // 64
    words = torch.full((nw + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if kid is None:
        ctx.p384_verify_batch_dev(n, *[t.data_ptr() for t in dev], words.data_ptr(), status.data_ptr(), stream)
    else:
        k = torch.from_numpy(kid.view(np.int32)).cuda()
        ctx.p384_verify_batch_keyed_dev(n, k.data_ptr(), *[t.data_ptr() for t in dev], words.data_ptr(), status.data_ptr(), stream)
    torch.cuda.synchronize()
    w = words.cpu().numpy().view(np.uint64)
    s = status.cpu().numpy()
    return w[:nw], s[:n], int(w[nw]), int(s[n])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_parity_with_the_reference_and_the_fresh_key_entry(ctx, ids, n):
    rows, want = C.mixed257()
    rows, want = rows[:n], np.array(want[:n], dtype=np.uint8)
    kid = _kid(ids, rows)
    bits, st = ctx.p384_verify_batch_keyed(kid, *_cols(rows))
    assert (st == want).all(), np.nonzero(st != want)
    assert (bits == (want == 0)).all()
    fbits, fst = ctx.p384_verify_batch(*_cols(rows, (0, 1, 2, 3, 4)))
    assert st.tobytes() == fst.tobytes() and bits.tobytes() == fbits.tobytes()
    # the _dev twin: the same bytes, word for word the fresh-key entry's, nothing at or above n, nothing behind the arrays
    w, s, gw, gs = _dev_words(ctx, n, _cols(rows), kid)
    fw, fs, _, _ = _dev_words(ctx, n, _cols(rows, (0, 1, 2, 3, 4)))
    assert s.tobytes() == st.tobytes() and w.tobytes() == fw.tobytes() and s.tobytes() == fs.tobytes()
    assert (fabgpu.unpack_bits(w, n) == bits).all()
    assert gw == 2**64 - 1 and gs == 9
    tail = n - 64 * ((n + 63) // 64 - 1)
    assert int(w[-1]) >> tail == 0                               # (the last word was all ones before the launch)


@pytest.mark.parametrize("sha3", [False, True])
def test_fused_hash_forms_at_the_block_edges(ctx, ids, sha3):
    """identity.Verify under registered keys: message lengths around the 64-byte (SHA-256) and 136-byte (SHA3-256) block edges"""
    import torch
    rng = random.Random(384064 + sha3)
    hf = hashlib.sha3_256 if sha3 else hashlib.sha256
    lens = [0, 55, 56, 63, 64, 65, 119, 120, 127, 128, 135, 136, 137, 271, 272]
    n = 65
    msgs, rows = [], []
    for i in range(n):
        m = bytes(rng.randrange(256) for _ in range(lens[i % len(lens)]))
        d, q = C.keys()[i % 5]
        sg = R.sign(d, R.hash_to_int(hf(m).digest()), rng.randrange(1, N))
        r, s = sg[0], R.low_s(sg[1])
        if i % 4 == 3:
            if i % 8 == 3:
                m = m + b"x"
            else:
                r ^= 2
        msgs.append(m)
        rows.append((q[0], q[1], R.hash_to_int(hf(m).digest()), r, s))
    want = np.array(C.want(rows), dtype=np.uint8)
    assert (want == 0).sum() >= 40 and (want == 1).sum() >= 10
    arena = np.frombuffer(b"".join(msgs) + bytes(8), dtype=np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)
    kid = _kid(ids, rows)
    r_, s_ = _cols(rows, (3, 4))
    bits, st = ctx.hash_p384_verify_batch_keyed(arena, off, kid, r_, s_, sha3=sha3)
    assert (st == want).all(), np.nonzero(st != want)
    assert (bits == (want == 0)).all()
    fbits, fst = ctx.hash_p384_verify_batch(arena, off, *_cols(rows, (0, 1)), r_, s_, sha3=sha3)
    assert st.tobytes() == fst.tobytes() and bits.tobytes() == fbits.tobytes()
    t = {k: torch.from_numpy(v).cuda() for k, v in dict(arena=arena, off=off.view(np.int32), kid=kid.view(np.int32), r=r_, s=s_).items()}
    words = torch.full(((n + 63) // 64 + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda")
    ctx.hash_p384_verify_batch_keyed_dev(n, t["arena"].data_ptr(), t["arena"].numel(), t["off"].data_ptr(), t["kid"].data_ptr(), t["r"].data_ptr(),
                                         t["s"].data_ptr(), words.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream, sha3=sha3)
    torch.cuda.synchronize()
    w, sd = words.cpu().numpy().view(np.uint64), status.cpu().numpy()
    assert sd[:n].tobytes() == st.tobytes() and sd[n] == 9 and int(w[-1]) == 2**64 - 1
    assert (fabgpu.unpack_bits(w[:-1], n) == bits).all() and int(w[-2]) >> (n - 64) == 0


def test_exceptional_sums(ctx, ids):
    """P + P in the last addition (Q = G), a sum at infinity (Q = -G), u1 = 0, u2 with empty upper windows, e >= n, x(R) in [n, p)"""
    rows, want = C.exceptional()
    want = np.array(want, dtype=np.uint8)
    mine = dict(ids)
    for t in rows:                                               # (the second branch's constructed key)
        if (t[0], t[1]) not in mine:
            mine[(t[0], t[1])] = ctx.p384_key_register(R.b48(t[0]), R.b48(t[1]))
    bits, st = ctx.p384_verify_batch_keyed(_kid(mine, rows), *_cols(rows))
    assert (st == want).all(), (st, want)
    assert (bits == (want == 0)).all()
    fbits, fst = ctx.p384_verify_batch(*_cols(rows, (0, 1, 2, 3, 4)))
    assert st.tobytes() == fst.tobytes() and bits.tobytes() == fbits.tobytes()
    for q in set(mine) - set(ids):
        assert ctx.p384_key_unregister(mine[q])


def test_ids_that_name_no_live_key_answer_4_beside_live_rows():
    """one wavefront: live rows, an id at the high-water mark, an id of a future generation, a retired id; then the slot's next tenant"""
    c = fabgpu.Context(device=0)
    try:
        rows, want = C.mixed257()
        ks = [q for _d, q in C.keys()]
        kid = {q: c.p384_key_register(*_b(q)) for q in ks[:3]}
        assert list(kid.values()) == [0, 1, 2]
        live = [(t, w) for t, w in zip(rows, want) if (t[0], t[1]) in kid and w == 0][:40]
        victim = [t for t, _w in live if (t[0], t[1]) == ks[1]][:4]
        assert len(live) == 40 and len(victim) == 4

        def run(extra):
            """the 40 live rows, then `extra` = [(row, id)]: statuses of all of them"""
            rs = [t for t, _w in live] + [t for t, _i in extra]
            k = np.array([kid[(t[0], t[1])] for t, _w in live] + [i for _t, i in extra], dtype=np.uint32)
            bits, st = c.p384_verify_batch_keyed(k, *_cols(rs))
            assert (bits == (st == 0)).all()
            return st

        st = run([(victim[0], 3), (victim[1], 1 << 12 | 1), (victim[2], 4095), (victim[3], kid[ks[1]])])
        assert (st[:40] == 0).all() and list(st[40:]) == [4, 4, 4, 0]
        stale = kid[ks[1]]
        assert c.p384_key_unregister(stale) and not c.p384_key_unregister(stale)
        assert c.p384_key_count() == 2 and c.p384_key_lookup(*_b(ks[1])) is None
        want_live = np.array([4 if (t[0], t[1]) == ks[1] else 0 for t, _w in live], dtype=np.uint8)
        st = run([(victim[0], stale)])
        assert (st[:40] == want_live).all() and st[40] == 4 and (want_live == 0).sum() >= 10
        # another key takes the slot under the next generation: the stale id still answers 4, the new id verifies under the new key only
        new = c.p384_key_register(*_b(ks[3]))
        assert new == (1 << 12 | 1)
        stats = c.p384_key_table_stats()
        assert stats["live"] == 3 and stats["reused"] == 1 and stats["draining"] == 0 and stats["slots_used"] == 3
        r3 = [t for t, w in zip(rows, want) if (t[0], t[1]) == ks[3] and w == 0][:2]
        st = run([(victim[0], stale), (r3[0], new), (victim[1], new), (r3[1], stale)])
        assert (st[:40] == want_live).all() and list(st[40:]) == [4, 0, 1, 4]
        assert fabgpu.p384_comb_device(c, new).tobytes() == fabgpu.p384_comb_host(*_b(ks[3])).tobytes()
    finally:
        c.close()


# ---- the provider layer (option p384): imported keys move the *_p384 calls onto the keyed entries ----
@pytest.fixture(scope="module")
def provider_cases():
    """(key, DER signature, digest, message, reference status) over the five keys: valid, changed digest, changed r, high S"""
    rng = random.Random(384040)
    cases = []
    for i in range(40):
        d, q = C.keys()[i % 5]
        msg = b"p384 keyed provider %d" % i
        dg = hashlib.sha256(msg).digest()
        sg = R.sign(d, R.hash_to_int(dg), rng.randrange(1, N))
        r, s = sg[0], R.low_s(sg[1])
        kind = (i // 5) % 4
        if kind == 1:
            dg = hashlib.sha256(msg + b"!").digest()
        elif kind == 2:
            r ^= 4
        elif kind == 3:
            s = N - s
        cases.append((q, R.der_sig(r, s), dg, msg, R.status(q[0], q[1], R.hash_to_int(dg), r, s)))
    want = [c[4] for c in cases]
    assert want.count(0) >= 10 and want.count(1) >= 10 and want.count(2) >= 5
    return cases


def test_provider_import_registers_nothing_while_the_option_is_off():
    csp = fabgpu.GPUCSP(device=0)
    try:
        q = C.keys()[0][1]
        assert csp.key_import_p384(q) == (True, "P-384 is served by bccsp/sw, not by the GPU provider")
        assert csp.p384_key_table_stats() == dict.fromkeys(fabgpu.P384_KEY_TABLE_STATS, 0)        # not even the generator's table
    finally:
        csp.close()


def test_provider_takes_the_keyed_road_for_imported_keys_with_the_same_answers(provider_cases):
    keys, sigs, dgs, msgs, want = zip(*provider_cases)
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        fresh = csp.verify_batch_p384(keys, sigs, dgs)
        fresh_id = csp.identity_verify_batch_p384(keys, msgs, sigs)
        assert csp.p384_key_table_stats()["keyed_launches"] == 0
        for _d, q in C.keys()[:4]:
            assert csp.key_import_p384(q) == (True, "")
        assert csp.verify_batch_p384(keys, sigs, dgs) == fresh                     # one signer is not imported: the fresh-key entry
        assert csp.p384_key_table_stats()["keyed_launches"] == 0
        assert csp.key_import_p384(C.keys()[4][1]) == (True, "") and csp.key_import_p384(C.keys()[4][1]) == (True, "")
        st = csp.p384_key_table_stats()
        assert st["live"] == 5 and st["slots_used"] == 5
        assert csp.verify_batch_p384(keys, sigs, dgs) == fresh
        assert csp.p384_key_table_stats()["keyed_launches"] == 1
        assert csp.identity_verify_batch_p384(keys, msgs, sigs) == fresh_id
        assert csp.p384_key_table_stats()["keyed_launches"] == 2
        for (valid, err), w in zip(fresh, want):
            assert valid == (w == 0) and (err is None) == (w != 2)
        # an off-curve import: KeyImport's own answer (no text, not on the curve), nothing registered; its rows are not the provider's
        q = C.keys()[0][1]
        off = (q[0], q[1] ^ 1)
        assert csp.key_import_p384(off) == (False, "") and csp.p384_key_table_stats()["live"] == 5
        bad = csp.verify_batch_p384([off, q], [sigs[0], sigs[0]], [dgs[0], dgs[0]])
        assert bad[0] == (False, "public key is not on P-384: the GPU provider does not decide this tuple (use bccsp/sw)") and bad[1] == fresh[0]
    finally:
        csp.close()


def test_provider_coalesced_entry_from_16_threads_on_the_keyed_road(provider_cases):
    import threading
    keys, sigs, dgs, msgs, want = zip(*provider_cases)
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        for _d, q in C.keys():
            assert csp.key_import_p384(q) == (True, "")
        csp.coalescer_configure(window_us=2000, max_batch=64)
        batch = csp.verify_batch_p384(keys, sigs, dgs)
        before = csp.p384_key_table_stats()["keyed_launches"]
        got = [None] * len(provider_cases)

        def worker(t):
            for i in range(t, len(provider_cases), 16):
                try:
                    got[i] = (csp.verify_coalesced_p384(keys[i], sigs[i], dgs[i]), None)
                except fabgpu.BCCSPError as x:
                    got[i] = (False, str(x))
        th = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert got == batch
        cs = csp.coalescer_stats()
        assert cs["launches"] < cs["calls"] and cs["largest_batch"] > 1
        assert csp.p384_key_table_stats()["keyed_launches"] - before == cs["launches"]      # every coalesced launch was a keyed one
    finally:
        csp.close()


def test_provider_audit_poisons_on_a_forged_valid_on_the_keyed_road(provider_cases):
    keys, sigs, dgs, msgs, want = zip(*provider_cases)
    bad = [i for i, w in enumerate(want) if w == 1][0]
    good = [i for i, w in enumerate(want) if w == 0][0]
    csp = fabgpu.GPUCSP(device=0, p384=1, audit_permille=1000)
    try:
        for k in {keys[bad], keys[good]}:
            assert csp.key_import_p384(k) == (True, "")
        assert csp.verify_batch_p384([keys[good]], [sigs[good]], [dgs[good]]) == [(True, None)]      # an honest "valid" passes the audit
        assert csp.identity_verify_batch_p384([keys[good]], [msgs[good]], [sigs[good]]) == [None]
        assert csp.p384_key_table_stats()["keyed_launches"] == 2 and not csp.poisoned()
        fabgpu.p384_corrupt(csp, 1)
        with pytest.raises(fabgpu.PoisonedError):
            csp.verify_batch_p384([keys[bad]], [sigs[bad]], [dgs[bad]])
        assert csp.poisoned() and csp.p384_key_table_stats()["keyed_launches"] == 3
    finally:
        csp.close()
