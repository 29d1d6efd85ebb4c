"""Registered P-384 keys on eight lanes per signature (FABGPU_FLAG_P384_WIDE, csrc/p384_wide_kernels.hip) on the device: the crafted
list of p384_wide_cases.py and seeded signatures through the C entries of a context with the flag, against Python integers (p384_ref.py)
and against the same rows through a context without it; the provider option "p384_wide" through a block pass."""
import hashlib
import random

import numpy as np
import pytest

import fabgpu
import p384_blocks as pb
import p384_ref as R
import p384_wide_cases as W

pytestmark = pytest.mark.gpu
N = R.N
LIVE_KEYS = ("G", "A", "-A", "K", "B", "-B", "C", "-C", "-G")      # (the four of the issue first; then the keys of the other tree levels)


def _b(q):
    return R.b48(q[0]), R.b48(q[1])


def _register(c):
    """the keys of the crafted list in one order on every context: name -> id; "gone" is registered last and retired"""
    ids = {k: c.p384_key_register(*_b(W.keys()[k][1])) for k in LIVE_KEYS}
    assert list(ids.values()) == list(range(len(LIVE_KEYS)))
    gone = c.p384_key_register(*_b(W.keys()["gone"][1]))
    assert gone == len(LIVE_KEYS) and c.p384_key_unregister(gone)
    ids["gone"] = gone
    return ids


@pytest.fixture(scope="module")
def wide():
    c = fabgpu.Context(device=0, flags=fabgpu.FLAG_P384_WIDE)
    yield c, _register(c)
    c.close()


@pytest.fixture(scope="module")
def plain():
    c = fabgpu.Context(device=0)
    yield c, _register(c)
    c.close()


def _id(ids, key, kind):
    if kind == W.LIVE or kind == W.RETIRED:
        return ids[key]
    if kind == W.WRONG_GEN:
        return ids[key] | 1 << 12
    return len(LIVE_KEYS) + 1                                    # the high-water mark: ten slots were used


def _cols(rows, which=(2, 3, 4)):
    return [np.frombuffer(b"".join(R.b48(t[k]) for t in rows), dtype=np.uint8).copy() for k in which]


@pytest.fixture(scope="module")
def pool():
    """640 rows with their reference statuses: the 256 seeded signatures (every second one tampered) and the crafted list, repeated -
    what the row-count tests cut their n rows from; [(key, row, id kind)], statuses"""
    rows, want = W.random256()
    base = [(k, row, W.LIVE) for k, row in rows] + [(k, row, kind) for _n, k, row, kind in W.crafted()]
    st = list(want) + list(W.crafted_expected())
    rng = random.Random(384640)
    order = list(range(len(base))) + [rng.randrange(len(base)) for _ in range(640 - len(base))]
    return [base[i] for i in order], np.array([st[i] for i in order], dtype=np.uint8)


def _kid(ids, cases):
    return np.array([_id(ids, k, kind) for k, _row, kind in cases], dtype=np.uint32)


def test_the_flag_is_a_known_bit_and_off_by_default(wide, plain):
    assert fabgpu.FLAG_P384_WIDE == 4096
    assert wide[0].p384_wide_rows() == 0 and plain[0].p384_wide_rows() == 0


def test_the_crafted_list_against_the_reference(wide):
    c, ids = wide
    cases = [(k, row, kind) for _n, k, row, kind in W.crafted()]
    want = np.array(W.crafted_expected(), dtype=np.uint8)
    before = c.p384_wide_rows()
    bits, st = c.p384_verify_batch_keyed(_kid(ids, cases), *_cols([row for _k, row, _kind in cases]))
    bad = np.nonzero(st != want)[0]
    assert bad.size == 0, [(W.crafted()[i][0], int(st[i]), int(want[i])) for i in bad]
    assert (bits == (want == 0)).all()
    assert c.p384_wide_rows() - before == len(cases)
    # the verdict words themselves, through the _dev twin
    w, s = _dev(c, len(cases), _kid(ids, cases), _cols([row for _k, row, _kind in cases]))[:2]
    assert w.tobytes() == np.packbits(want == 0, bitorder="little").tobytes().ljust(w.nbytes, b"\0") and s.tobytes() == want.tobytes()


GUARD_WORDS, GUARD_BYTES = 4, 64


def _dev(c, n, kid, cols):
    """the _dev entry into buffers pre-filled with 0xA5 out to a guard region: (words, statuses, guard words, guard bytes)"""
    import torch
    dev = [torch.from_numpy(x).cuda() for x in cols]
    k = torch.from_numpy(kid.view(np.int32)).cuda()
    nw = (n + 63) // 64
    words = torch.full(((nw + GUARD_WORDS) * 8,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((n + GUARD_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")
    c.p384_verify_batch_keyed_dev(n, k.data_ptr(), *[t.data_ptr() for t in dev], words.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    w = words.cpu().numpy().view(np.uint64)
    s = status.cpu().numpy()
    return w[:nw], s[:n], w[nw:], s[n:]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 513])
def test_row_counts_around_the_wavefront_and_the_verdict_word(wide, plain, pool, n):
    cases, want = pool[0][:n], pool[1][:n]
    cols = _cols([row for _k, row, _kind in cases])
    w, s, gw, gs = _dev(wide[0], n, _kid(wide[1], cases), cols)
    assert (gw == 0xA5A5A5A5A5A5A5A5).all() and (gs == 0xA5).all()          # nothing at or above ceil(n / 64) words and n bytes
    tail = n - 64 * (len(w) - 1)
    assert tail == 64 or int(w[-1]) >> tail == 0                            # the bits at or above n in the last word are zero
    assert s.tobytes() == want.tobytes() and (fabgpu.unpack_bits(w, n) == (want == 0)).all()
    pw, ps, pgw, pgs = _dev(plain[0], n, _kid(plain[1], cases), cols)       # the one-lane form: the same bytes
    assert w.tobytes() == pw.tobytes() and s.tobytes() == ps.tobytes()
    assert (pgw == 0xA5A5A5A5A5A5A5A5).all() and (pgs == 0xA5).all()


@pytest.mark.parametrize("n", [8192, 8193])
def test_the_largest_wide_launch_and_the_first_one_lane_launch(wide, plain, pool, n):
    rng = random.Random(n)
    pick = [rng.randrange(len(pool[0])) for _ in range(n)]
    cases, want = [pool[0][i] for i in pick], pool[1][pick]
    cols = _cols([row for _k, row, _kind in cases])
    before = wide[0].p384_wide_rows()
    w, s, gw, gs = _dev(wide[0], n, _kid(wide[1], cases), cols)
    assert wide[0].p384_wide_rows() - before == (n if n <= 8192 else 0)     # 8 193 rows: the one-lane kernel
    pw, ps, _, _ = _dev(plain[0], n, _kid(plain[1], cases), cols)
    assert w.tobytes() == pw.tobytes() and s.tobytes() == ps.tobytes()
    assert s.tobytes() == want.tobytes() and (gw == 0xA5A5A5A5A5A5A5A5).all() and (gs == 0xA5).all()
    assert plain[0].p384_wide_rows() == 0


@pytest.fixture(scope="module")
def hashed():
    """65 signed messages per hash, lengths around the block edges, every fourth one tampered: sha3 -> (msgs, [(key, row)], statuses)"""
    out = {}
    lens = [0, 55, 56, 63, 64, 65, 119, 120, 127, 128, 135, 136, 137, 271, 272]
    for sha3 in (False, True):
        rng = random.Random(384650 + sha3)
        hf = hashlib.sha3_256 if sha3 else hashlib.sha256
        msgs, rows = [], []
        for i in range(65):
            m = bytes(rng.randrange(256) for _ in range(lens[i % len(lens)]))
            key = ("K", "G", "A", "-A")[i % 4]
            d, q = W.keys()[key]
            sg = None
            while not sg:
                sg = R.sign(d, R.hash_to_int(hf(m).digest()), rng.randrange(1, 2**40))      # (a short nonce: the reference multiplies bit by bit)
            r, s = sg[0], R.low_s(sg[1])
            if i % 4 == 3:
                if i % 8 == 3:
                    m = m + b"x"
                else:
                    r ^= 2
            msgs.append(m)
            rows.append((key, (q[0], q[1], R.hash_to_int(hf(m).digest()), r, s)))
        want = np.array([R.status(*row) for _k, row in rows], dtype=np.uint8)
        assert (want == 0).sum() >= 40 and (want == 1).sum() >= 10
        out[sha3] = (msgs, rows, want)
    return out


def _arena(msgs):
    arena = np.frombuffer(b"".join(msgs) + bytes(8), dtype=np.uint8).copy()
    return arena, np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)


@pytest.mark.parametrize("sha3", [False, True], ids=["sha256", "sha3_256"])
def test_the_fused_hash_entries_take_32_byte_digests(wide, hashed, sha3):
    c, ids = wide
    msgs, rows, want = hashed[sha3]
    arena, off = _arena(msgs)
    kid = np.array([ids[k] for k, _row in rows], dtype=np.uint32)
    r_, s_ = _cols([row for _k, row in rows], (3, 4))
    before = c.p384_wide_rows()
    bits, st = c.hash_p384_verify_batch_keyed(arena, off, kid, r_, s_, sha3=sha3)
    assert (st == want).all(), np.nonzero(st != want)
    assert (bits == (want == 0)).all() and c.p384_wide_rows() - before == 65


@pytest.mark.parametrize("sha3", [False, True], ids=["sha256", "sha3_256"])
def test_the_keyed_branch_of_the_described_identity_batch(wide, hashed, sha3):
    c, ids = wide
    msgs, rows, want = hashed[sha3]
    arena, off = _arena(msgs)
    kid = np.array([ids[k] for k, _row in rows], dtype=np.uint32)
    r_, s_ = _cols([row for _k, row in rows], (3, 4))
    before = c.p384_wide_rows()
    bits, st = c.identity_verify_batch_p384(arena, off, r_, s_, key_id=kid, sha3=sha3)
    assert (st == want).all(), np.nonzero(st != want)
    assert (bits == (want == 0)).all() and c.p384_wide_rows() - before == 65
    qx, qy = _cols([row for _k, row in rows], (0, 1))                        # the fresh-key branch is not the wide form's
    fbits, fst = c.identity_verify_batch_p384(arena, off, r_, s_, qx=qx, qy=qy, sha3=sha3)
    assert fst.tobytes() == st.tobytes() and c.p384_wide_rows() - before == 65


# ---- the provider: option "p384_wide" through a block pass ----
@pytest.fixture(scope="module")
def block16():
    """16 transactions of P-384 signers, one endorsement tampered: (block, signers, tuples submitted, reference flags)"""
    rnd = random.Random(16384)
    s = pb.signers(4, 16384)
    envs, tuples = [], []
    for t in range(16):
        kw = {}
        if t == 11:
            kw["end_sig"] = lambda j, m, sig: s[1].sign(m[:-1] + bytes([m[-1] ^ 1])) if j == 1 else sig      # (its second endorser is s[1])
        env, tu = pb.endorser_tx(rnd, s[0], [s[1 + t % 3], s[1 + (t + 1) % 3]], **kw)
        envs.append(env)
        tuples.append(tu)
    import blockbuilder as bb
    tx, kind, st = [], [], []
    for t, tu in enumerate(tuples):
        for k, who, msg, sig in tu:
            tx.append(t); kind.append(k); st.append(pb.tuple_status(who.q, msg, sig))
    flags = pb.fold_flags(16, [1] * 16, tx, kind, st)
    assert flags == [pb.TX_VALID] * 11 + [pb.TX_BAD_ENDORSEMENT] + [pb.TX_VALID] * 4 and len(st) == 48
    return bb.block(16, envs), s, len(st), flags


def _pass(csp, blk, seq):
    csp.set_option("pass_stage_min_bytes", 1 << 40)
    return fabgpu.preverify_block2(csp, blk, block_seq=seq)


def test_the_option_name_is_known_and_off_by_default():
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        assert csp.get_option("p384_wide") == 0 and csp.p384_pass_stats()["wide_rows"] == 0
    finally:
        csp.close()
    csp = fabgpu.GPUCSP(device=0, p384=1, p384_wide=1)
    try:
        assert csp.get_option("p384_wide") == 1
        assert csp.set_option("p384_wide", 0) == 1 and csp.set_option("p384_wide", 1) == 0
    finally:
        csp.close()


def test_block_pass_with_every_signer_imported_counts_its_rows_as_wide(block16):
    blk, signers, n_sub, flags = block16
    outs, stats = [], []
    for on in (1, 0):
        csp = fabgpu.GPUCSP(device=0, p384=1, p384_wide=on)
        try:
            for sg in signers:
                assert csp.key_import_p384(sg.q) == (True, "")
            outs.append(_pass(csp, blk, 1))
            stats.append(csp.p384_pass_stats())
        finally:
            csp.close()
    assert outs[0]["tx_flags"].tolist() == outs[1]["tx_flags"].tolist() == flags
    assert outs[0]["tuple_status"].tolist() == outs[1]["tuple_status"].tolist()
    assert stats[0]["submitted"] == stats[1]["submitted"] == n_sub and stats[0]["keyed_launches"] == stats[1]["keyed_launches"] == 1
    assert stats[0]["wide_rows"] == n_sub and stats[1]["wide_rows"] == 0


def test_block_pass_with_one_signer_not_imported_counts_no_wide_rows(block16):
    blk, signers, n_sub, flags = block16
    csp = fabgpu.GPUCSP(device=0, p384=1, p384_wide=1)
    try:
        for sg in signers[:-1]:
            assert csp.key_import_p384(sg.q) == (True, "")
        out = _pass(csp, blk, 1)
        st = csp.p384_pass_stats()
        assert out["tx_flags"].tolist() == flags
        assert (st["submitted"], st["fresh_launches"], st["keyed_launches"], st["wide_rows"]) == (n_sub, 1, 0, 0)
    finally:
        csp.close()
