"""The optional 16-bit comb tables of registered P-384 keys (FABGPU_FLAG_P384_KEY_TABLES_16BIT; csrc/p384_tables16.h, the builder in
csrc/p384_keytab_kernels.hip, the 24-window instantiation of csrc/p384_keyed_kernels.hip) on the device: answers against Python integers
(p384_ref.py) and against a context without the flag, the table bytes against the host builder and against a device-side recomputation,
the choice per wavefront, retirement and reuse, and the provider option.  No test holds more than two keys' tables and the generator's."""
import hashlib
import random
import types

import numpy as np
import pytest

import fabgpu
import p384_blocks as pb
import p384_ref as R
import p384_tables16_cases as C

pytestmark = pytest.mark.gpu
TABLE16_BYTES = 24 * 65536 * 96
TWO = ("G", "-G")                         # the two registered keys of this file: the steering rows need exactly these


def _b(name):
    q = C.keys()[name][1]
    return R.b48(q[0]), R.b48(q[1])


def _cols(rows, which=(2, 3, 4)):
    return [np.frombuffer(b"".join(R.b48(t[k]) for t in rows), dtype=np.uint8).copy() for k in which]


@pytest.fixture(scope="module")
def on():
    c = fabgpu.Context(device=0, flags=fabgpu.FLAG_P384_KEY_TABLES_16BIT)
    ids = {k: c.p384_key_register(*_b(k)) for k in TWO}
    yield c, ids
    c.close()


@pytest.fixture(scope="module")
def off():
    c = fabgpu.Context(device=0)
    ids = {k: c.p384_key_register(*_b(k)) for k in TWO}
    yield c, ids
    c.close()


@pytest.fixture(scope="module")
def rows130():
    """130 rows - two full wavefronts and a partial one: 111 signed rows of the two keys, every fourth with a bit flipped in e, r or s,
    and the 19 steering rows; [(key, row)], statuses"""
    rows, st = C.signed(111, 38416111, TWO)
    steer = C.steering(TWO)
    allr = list(rows) + [(k, row) for _n, k, row in steer]
    want = np.array(list(st) + list(C.steering_expected(TWO)), dtype=np.uint8)
    assert len(allr) == 130 and (want == 0).sum() >= 90 and (want == 1).sum() >= 20
    return allr, want


@pytest.fixture(scope="module")
def hashed():
    """65 signed messages per hash (the E32 form of the kernels), every fourth one tampered: sha3 -> (msgs, [(key, row)], statuses)"""
    out = {}
    lens = [0, 55, 56, 63, 64, 65, 119, 120, 127, 128, 135, 136, 137, 271, 272]
    for sha3 in (False, True):
        rng = random.Random(384160 + sha3)
        hf = hashlib.sha3_256 if sha3 else hashlib.sha256
        msgs, rows = [], []
        for i in range(65):
            m = bytes(rng.randrange(256) for _ in range(lens[i % len(lens)]))
            key = TWO[i % 2]
            d, q = C.keys()[key]
            sg = None
            while not sg:
                sg = R.sign(d, R.hash_to_int(hf(m).digest()), rng.randrange(1, 2**40))
            r, s = sg[0], R.low_s(sg[1])
            if i % 4 == 3:
                if i % 8 == 3:
                    m = m + b"x"
                else:
                    r ^= 2
            msgs.append(m)
            rows.append((key, (q[0], q[1], R.hash_to_int(hf(m).digest()), r, s)))
        out[sha3] = (msgs, rows, np.array([R.status(*row) for _k, row in rows], dtype=np.uint8))
    return out


def _arena(msgs):
    arena = np.frombuffer(b"".join(msgs) + bytes(8), dtype=np.uint8).copy()
    return arena, np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)


def _dev(c, n, kid, cols):
    import torch
    dev = [torch.from_numpy(x).cuda() for x in cols]
    k = torch.from_numpy(kid.view(np.int32)).cuda()
    words = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    status = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    c.p384_verify_batch_keyed_dev(n, k.data_ptr(), *[t.data_ptr() for t in dev], words.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return words.cpu().numpy().view(np.uint64), status.cpu().numpy()


def test_a_flag_context_verifies_on_16_bit_tables(on, off, rows130, hashed):
    assert fabgpu.FLAG_P384_KEY_TABLES_16BIT == 8192
    c, ids = on
    p, pids = off
    assert fabgpu.p384_tables16_wait(c) == 2 and fabgpu.p384_tables16_wait(p) == 0
    rows, want = rows130
    kid = np.array([ids[k] for k, _row in rows], dtype=np.uint32)
    cols = _cols([row for _k, row in rows])
    before = c.p384_tables16_rows()
    bits, st = c.p384_verify_batch_keyed(kid, *cols)
    bad = np.nonzero(st != want)[0]
    assert bad.size == 0, [(int(i), int(st[i]), int(want[i])) for i in bad]
    assert (bits == (want == 0)).all()
    assert c.p384_tables16_rows() - before == 130                 # all three wavefronts qualified
    pbits, pst = p.p384_verify_batch_keyed(np.array([pids[k] for k, _row in rows], dtype=np.uint32), *cols)
    assert pst.tobytes() == st.tobytes() and (pbits == bits).all() and p.p384_tables16_rows() == 0
    # the verdict words themselves, through the _dev twin
    w, s = _dev(c, 130, kid, cols)
    pw, ps = _dev(p, 130, kid, cols)
    assert s.tobytes() == want.tobytes() and w.tobytes() == pw.tobytes() == np.packbits(want == 0, bitorder="little").tobytes().ljust(w.nbytes, b"\0")
    assert ps.tobytes() == s.tobytes() and c.p384_tables16_rows() - before == 260
    # the E32 form: the SHA-256 and SHA3-256 keyed entries
    for sha3 in (False, True):
        msgs, hrows, hwant = hashed[sha3]
        arena, offs = _arena(msgs)
        hk = np.array([ids[k] for k, _row in hrows], dtype=np.uint32)
        r_, s_ = _cols([row for _k, row in hrows], (3, 4))
        b0 = c.p384_tables16_rows()
        hb, hs = c.hash_p384_verify_batch_keyed(arena, offs, hk, r_, s_, sha3=sha3)
        assert (hs == hwant).all(), np.nonzero(hs != hwant)
        assert (hb == (hwant == 0)).all() and c.p384_tables16_rows() - b0 == 65
        qb, qs = p.hash_p384_verify_batch_keyed(arena, offs, hk, r_, s_, sha3=sha3)
        assert qs.tobytes() == hs.tobytes() and (qb == hb).all()
    stats, pstats = c.p384_key_table_stats(), p.p384_key_table_stats()
    assert (stats["tables16_live"], stats["tables16_bytes"]) == (2, 2 * TABLE16_BYTES)
    assert (pstats["tables16_live"], pstats["tables16_bytes"]) == (0, 0)
    v = (fabgpu.ctypes.c_uint64 * 9)(*([77] * 9))                 # a caller that asks for the old count gets the old values
    assert c._L.fabgpu_p384_key_table_stats(c._h, v, 7) == 9 and list(v)[:7] == [stats[k] for k in fabgpu.P384_KEY_TABLE_STATS[:7]] and list(v)[7:] == [77, 77]


@pytest.mark.parametrize("which", ["generator", "key"])
def test_table_bytes_against_the_host_builder_and_a_device_recomputation(on, which):
    c, ids = on
    gen = which == "generator"
    got = fabgpu.p384_comb16_check(c, ids["-G"], generator=gen)
    assert got is not None
    bad, wins = got
    assert bad == 0                                               # every one of the 24 x 65 536 entries, recomputed on the device
    t8 = fabgpu.p384_comb_host(*(() if gen else _b("-G")))
    assert (fabgpu.p384_comb_device(c, ids["-G"], generator=gen) == t8).all()
    W = fabgpu.P384_COMB16_WINDOW_WORDS
    for i, w in enumerate((0, 11, 23)):
        host = fabgpu.p384_comb16_host(t8, w, w + 1)
        dev = wins[i * W:(i + 1) * W]
        assert dev[:24].tolist() == [0] * 24                      # entry 0
        assert dev.tobytes() == host.tobytes(), "window %d" % w


def test_fallback_per_wavefront_with_the_cap_lowered_to_one(rows130):
    c = fabgpu.Context(device=0, flags=fabgpu.FLAG_P384_KEY_TABLES_16BIT)
    try:
        fabgpu.p384_tables16_cap(c, 1)
        k1 = c.p384_key_register(*_b("G"))
        k2 = c.p384_key_register(*_b("-G"))
        by = {"G": [], "-G": []}
        for (k, row), st in zip(*rows130):
            by[k].append((row, st))
        assert len(by["G"]) >= 64 and len(by["-G"]) >= 44
        # wavefront 0: key 1 only; wavefront 1: both keys; wavefront 2 (partial, 40 rows): key 2 only
        mixed = [("G", by["G"][i]) if i % 2 == 0 else ("-G", by["-G"][i]) for i in range(64)]
        plan = [("G", x) for x in by["G"][:64]] + mixed + [("-G", x) for x in by["-G"][:40]]
        kid = np.array([k1 if k == "G" else k2 for k, _x in plan], dtype=np.uint32)
        cols = _cols([x[0] for _k, x in plan])
        want = np.array([x[1] for _k, x in plan], dtype=np.uint8)
        # right after the registrations, before the build can be known to have finished: correct whichever stream it took
        bits, st = c.p384_verify_batch_keyed(kid, *cols)
        assert st.tobytes() == want.tobytes() and (bits == (want == 0)).all()
        assert fabgpu.p384_tables16_wait(c) == 1                  # key 2 is beyond the cap: no 16-bit table
        assert fabgpu.p384_comb16_check(c, k2, windows=False) is None and fabgpu.p384_comb16_check(c, k1, windows=False) == (0, None)
        before = c.p384_tables16_rows()
        bits, st = c.p384_verify_batch_keyed(kid, *cols)
        assert st.tobytes() == want.tobytes() and (bits == (want == 0)).all()
        assert c.p384_tables16_rows() - before == 64              # wavefront 0 alone
        # a stale id in a wavefront of key 1 answers 4 and does not send the wavefront back to the 8-bit stream
        kid2, want2 = kid[:64].copy(), want[:64].copy()
        kid2[5] = k1 | 1 << 12
        want2[5] = 4
        before = c.p384_tables16_rows()
        bits, st = c.p384_verify_batch_keyed(kid2, *[x[:64 * 48] for x in cols])
        assert st.tobytes() == want2.tobytes() and c.p384_tables16_rows() - before == 64
    finally:
        c.close()


def test_retire_and_reuse(rows130):
    c = fabgpu.Context(device=0, flags=fabgpu.FLAG_P384_KEY_TABLES_16BIT)
    try:
        k1 = c.p384_key_register(*_b("G"))
        assert fabgpu.p384_tables16_wait(c) == 1
        s1 = c.p384_key_table_stats()
        assert (s1["tables16_live"], s1["tables16_bytes"]) == (1, TABLE16_BYTES)
        assert c.p384_key_unregister(k1)
        s2 = c.p384_key_table_stats()
        assert (s2["tables16_live"], s2["tables16_bytes"]) == (0, 0)
        g_rows = [(row, st) for (k, row), st in zip(*rows130) if k == "G"]
        assert len(g_rows) > 64                                   # a full wavefront and a partial one
        cols = _cols([x[0] for x in g_rows])
        bits, st = c.p384_verify_batch_keyed(np.full(len(g_rows), k1, dtype=np.uint32), *cols)
        want_stale = np.array([4 if x[1] in (0, 1) else x[1] for x in g_rows], dtype=np.uint8)
        assert st.tobytes() == want_stale.tobytes() and not bits.any()     # the stale id answers 4
        k2 = c.p384_key_register(*_b("-G"))
        assert k2 & 0xFFF == k1 & 0xFFF and k2 != k1              # the slot, under the next generation
        assert fabgpu.p384_tables16_wait(c) == 1
        assert fabgpu.p384_comb16_check(c, k2, windows=False) == (0, None)     # a table of its own: -G's entries, not G's
        s3 = c.p384_key_table_stats()
        assert (s3["tables16_live"], s3["tables16_bytes"]) == (1, TABLE16_BYTES)
        m_rows = [(row, st) for (k, row), st in zip(*rows130) if k == "-G"][:44]
        before = c.p384_tables16_rows()
        bits, st = c.p384_verify_batch_keyed(np.full(44, k2, dtype=np.uint32), *_cols([x[0] for x in m_rows]))
        assert st.tolist() == [x[1] for x in m_rows] and c.p384_tables16_rows() - before == 44
        bits, st = c.p384_verify_batch_keyed(np.full(len(g_rows), k1, dtype=np.uint32), *cols)
        assert st.tobytes() == want_stale.tobytes()               # still stale: never -G's verdicts
    finally:
        c.close()


def test_the_provider_option():
    rnd = random.Random(3841640)
    s = pb.signers(2, 3841640)
    envs, n_tuples = [], 0
    for t in range(40):
        kw = {}
        if t == 17:
            kw["end_sig"] = lambda j, m, sig: s[1].sign(m[:-1] + bytes([m[-1] ^ 1]))
        env, tu = pb.endorser_tx(rnd, s[0], [s[1]], **kw)
        envs.append(env)
        n_tuples += len(tu)
    import blockbuilder as bb
    blk = bb.block(40, envs)
    msgs = [bytes(rnd.randrange(256) for _ in range(40 + i)) for i in range(70)]
    keys = [s[i % 2].q for i in range(70)]
    sigs = [s[i % 2].sign(m) for i, m in enumerate(msgs)]
    digs = [hashlib.sha256(m).digest() for m in msgs]
    digs[9] = hashlib.sha256(b"other").digest()
    outs = []
    for opt in (1, 0):
        csp = fabgpu.GPUCSP(device=0, p384=1, p384_key_tables16=opt, audit_permille=1000)
        try:
            assert csp.get_option("p384_key_tables16") == opt
            for sg in s:
                assert csp.key_import_p384(sg.q) == (True, "")
            ctx = types.SimpleNamespace(_h=csp._L.fabgpu_csp_ctx_of(csp._h, 0))      # (the provider's context, for the hook)
            assert fabgpu.p384_tables16_wait(ctx) == (2 if opt else 0)
            vb = csp.verify_batch_p384(keys, sigs, digs)
            csp.set_option("pass_stage_min_bytes", 1 << 40)
            r = fabgpu.preverify_block2(csp, blk, block_seq=1)
            st = csp.p384_key_table_stats()
            rows16 = csp.p384_tables16_rows()
            outs.append((vb, r["tx_flags"].tolist(), r["tuple_status"].tolist(), st, rows16, csp.audit_stats()["mismatches"]))
        finally:
            csp.close()
    a, b = outs
    assert a[0] == b[0] and [v for v, _e in a[0]].count(True) == 69
    assert a[1] == b[1] == [pb.TX_VALID] * 17 + [pb.TX_BAD_ENDORSEMENT] + [pb.TX_VALID] * 22
    assert a[2] == b[2] and len(a[2]) == n_tuples
    assert a[5] == b[5] == 0                                      # the audit recomputed every verdict on the CPU: no disagreement
    assert a[3]["tables16_live"] == 2 and b[3]["tables16_live"] == 0
    assert a[4] == 70 + n_tuples and b[4] == 0                    # both keyed launches ran on 16-bit tables, row for row
