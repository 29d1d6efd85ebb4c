"""SHA3-256 with 32 lanes on a message (fabric-mod_amd/csrc/sha3_coop.h, sha3_coop_kernels.hip; FABGPU_FLAG_SHA3_COOP) through the public entry
points, against hashlib.sha3_256: the small-launch road (sha3_256_coop_kernel, plain and prefixed) at every length around the 136-byte
block boundaries, at the four byte phases of a message's start, in consecutive-offset and in span form; the mixed road
(sha3_256_mixed_kernel) with long messages inside a launch above SHA3_COOP_MAX; hash -> verify; and the same inputs on a context
without the flag, which must answer the same bytes and count no row (fabgpu_sha3_coop_rows)."""
import hashlib

import numpy as np
import pytest

import coracle
import fabgpu

pytestmark = pytest.mark.gpu

SHA3_COOP_MAX = 4096                                  # csrc/kernels.h
LENGTHS = [0, 1, 7, 8, 9] + list(range(134, 139)) + list(range(270, 275)) + list(range(406, 411)) + [14 * 136 - 1, 14 * 136, 14 * 136 + 1]
PREFIX_LENS = (0, 1, 135, 136, 137, 300)
ROWS = (1, 2, 3, 63, 64, 65, 129)                     # half a wavefront, an idle second half, a partial last workgroup (eight rows each)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def coop():
    c = fabgpu.Context(device=0, flags=fabgpu.FLAG_SHA3_COOP)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain():
    c = fabgpu.Context(device=0)
    yield c
    c.close()


def _sha3(b: bytes) -> bytes:
    return hashlib.sha3_256(b).digest()


def _digests(msgs):
    return np.frombuffer(b"".join(_sha3(m) for m in msgs), dtype=np.uint8).reshape(len(msgs), 32)


def _dummy_sigs(n):
    z = np.zeros((n, 32), np.uint8)
    z[:, 31] = 1
    return z, z.copy(), z.copy(), z.copy()


def _bad_rows(got, want):
    return [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]


# ---- the grid, made once ---------------------------------------------------------------------------------------------------------------
_grid = {}


def grid():
    """Every length of LENGTHS at every byte phase of its start.  Consecutive form: a filler message of 0 .. 3 bytes in front of each
    puts its start on the phase (the fillers are messages like any other); span form: the same messages as (start, end) pairs, in
    another order and with junk between them."""
    if not _grid:
        rng = np.random.default_rng(1600)
        lens, phases = [], []
        pos = 5
        for ln in LENGTHS:
            for phase in range(4):
                fill = (phase - pos) % 4
                lens += [fill, ln]
                phases.append(((pos + fill) % 4, ln))
                pos += fill + ln
        assert sorted(set(phases)) == sorted((p, ln) for ln in LENGTHS for p in range(4))
        off = np.concatenate([[5], 5 + np.cumsum(lens)]).astype(np.uint32)
        arena = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)                  # (the last message ends on the arena's last byte)
        msgs = [arena[off[i]:off[i + 1]].tobytes() for i in range(len(lens))]
        order = rng.permutation(len(lens))
        spans = np.stack([off[:-1], off[1:]], axis=1)[order].astype(np.uint32)
        _grid.update(arena=arena, off=off, msgs=msgs, want=_digests(msgs), spans=spans, span_want=_digests([msgs[i] for i in order]))
        for v in _grid.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _grid


def test_consecutive_form_every_length_phase_and_row_count(coop, plain):
    g = grid()
    total = len(g["msgs"])
    assert total > 129
    before = coop.sha3_coop_rows()
    hashed = 0
    for n in ROWS + (total,):
        off = g["off"][:n + 1]
        got = coop.sha3_256_batch(g["arena"], off)
        assert not _bad_rows(got, g["want"][:n]), "n = %d: rows that disagree with hashlib.sha3_256: %s" % (n, _bad_rows(got, g["want"][:n])[:8])
        assert (plain.sha3_256_batch(g["arena"], off) == got).all()
        hashed += n
    assert coop.sha3_coop_rows() - before == hashed and plain.sha3_coop_rows() == 0


def test_span_form_every_length_phase_and_row_count(coop, plain):
    g = grid()
    total = len(g["msgs"])
    for n in ROWS + (total,):
        qx, qy, r, s = _dummy_sigs(n)
        sp = np.ascontiguousarray(g["spans"][:n]).reshape(-1)
        got = coop.identity_verify_batch(g["arena"], sp, r, s, qx=qx, qy=qy, spans=True, sha3=True, want_digests=True)[-1]
        assert not _bad_rows(got, g["span_want"][:n]), "n = %d: spans that disagree with hashlib.sha3_256: %s" % (n, _bad_rows(got, g["span_want"][:n])[:8])
        assert (plain.identity_verify_batch(g["arena"], sp, r, s, qx=qx, qy=qy, spans=True, sha3=True, want_digests=True)[-1] == got).all()
    assert plain.sha3_coop_rows() == 0


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def test_last_message_ends_on_the_arenas_last_byte_at_every_size_mod_4(coop):
    """the _dev form, so that arena_bytes is the caller's number: the clamp of the last dword is what keeps the reads inside"""
    import torch
    rng = np.random.default_rng(4)
    for cut in range(4):
        lens = [9, 137, 270, 136 * 3 - 2 + cut]
        off = np.concatenate([[2], 2 + np.cumsum(lens)]).astype(np.uint32)
        arena = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
        assert arena.size % 4 == cut
        d_arena, d_off = _up(arena), _up(off)
        out = torch.zeros(32 * len(lens), dtype=torch.uint8, device="cuda")
        coop.sha3_256_batch_dev(len(lens), d_arena.data_ptr(), arena.size, d_off.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want = _digests([arena[off[i]:off[i + 1]].tobytes() for i in range(len(lens))])
        assert (out.cpu().numpy().reshape(-1, 32) == want).all(), cut


# ---- prefixed: the seam at every position of a block -------------------------------------------------------------------------------------
def _prefixed_case():
    rng = np.random.default_rng(25)
    pre = [bytes(rng.integers(0, 256, size=L, dtype=np.uint8)) for L in PREFIX_LENS]
    rows = [(p, ln) for p in range(len(PREFIX_LENS)) for ln in LENGTHS] + [(NONE, 137), (NONE, 0)] + [(5, 33 + k) for k in range(5)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]                   # (prefixed rows beside rows without a prefix, in one wavefront)
    parts, pos, pspans, spans = [b"\x11" * 3], 3, [], []
    for p in pre:
        pspans.append((pos, pos + len(p))); parts.append(p + b"\x22"); pos += len(p) + 1
    sfx = []
    for _, ln in rows:
        x = bytes(rng.integers(0, 256, size=ln, dtype=np.uint8))
        sfx.append(x); spans.append((pos, pos + ln)); parts.append(x); pos += ln
    arena = np.frombuffer(b"".join(parts), dtype=np.uint8)
    msgs = [(pre[p] if p != NONE else b"") + x for (p, _), x in zip(rows, sfx)]
    return dict(arena=arena, spans=np.array(spans, dtype=np.uint32), pspans=np.array(pspans, dtype=np.uint32),
                pre_idx=np.array([p for p, _ in rows], dtype=np.uint32), want=_digests(msgs), rows=rows)


def test_prefixed_seam_at_every_position_shared_prefix_and_rows_without_one(coop, plain):
    c = _prefixed_case()
    n = len(c["rows"])
    assert n <= SHA3_COOP_MAX and sum(1 for p, _ in c["rows"] if p == 5) >= 5 + len(LENGTHS)
    qx, qy, r, s = _dummy_sigs(n)
    kw = dict(qx=qx, qy=qy, pre_off=c["pspans"].reshape(-1), pre_idx=c["pre_idx"], spans=True, sha3=True, want_digests=True)
    before = coop.sha3_coop_rows()
    got = coop.identity_verify_batch(c["arena"], c["spans"].reshape(-1), r, s, **kw)[-1]
    bad = [c["rows"][i] for i in _bad_rows(got, c["want"])]
    assert not bad, "(prefix index, suffix length) whose digest is not hashlib.sha3_256(prefix || msg): %s" % bad[:8]
    assert coop.sha3_coop_rows() - before == n
    assert (plain.identity_verify_batch(c["arena"], c["spans"].reshape(-1), r, s, **kw)[-1] == got).all() and plain.sha3_coop_rows() == 0


def test_reversed_span_hashes_as_empty_on_the_device_resident_entry(coop):
    """the host variant refuses a reversed span (FABGPU_EINVAL); the _dev entry validates nothing that lies in device memory, and the
    32-lane kernels read a reversed span as an empty one: row 1 is its prefix alone, row 3 (no prefix) the empty message"""
    import torch
    rng = np.random.default_rng(7)
    arena = rng.integers(0, 256, size=700, dtype=np.uint8)
    pspans = np.array([[10, 310]], dtype=np.uint32)
    spans = np.array([[400, 450], [500, 460], [320, 321], [690, 600], [600, 700]], dtype=np.uint32)
    pre_idx = np.array([0, 0, NONE, NONE, 0], dtype=np.uint32)
    pre = arena[10:310].tobytes()
    want = _digests([pre + arena[400:450].tobytes(), pre, arena[320:321].tobytes(), b"", pre + arena[600:700].tobytes()])
    n = 5
    qx, qy, r, s = _dummy_sigs(n)
    t = {k: _up(v) for k, v in dict(arena=arena, off=spans, pre_off=pspans, pre_idx=pre_idx, qx=qx, qy=qy, r=r, s=s).items()}
    dig = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    words = torch.zeros(8, dtype=torch.uint8, device="cuda")
    b = fabgpu._IdBatch()
    b.n, b.flags = n, fabgpu.IDB_SPANS | fabgpu.IDB_SHA3_256
    b.arena, b.arena_bytes, b.off = t["arena"].data_ptr(), arena.size, t["off"].data_ptr()
    b.n_prefixes, b.pre_off, b.pre_idx = 1, t["pre_off"].data_ptr(), t["pre_idx"].data_ptr()
    b.qx, b.qy, b.r, b.s = t["qx"].data_ptr(), t["qy"].data_ptr(), t["r"].data_ptr(), t["s"].data_ptr()
    b.verdict_bits, b.status, b.digests = words.data_ptr(), None, dig.data_ptr()
    mid = torch.zeros(200, dtype=torch.uint8, device="cuda")
    coop.identity_verify_batch_dev(b, mid.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not _bad_rows(dig.cpu().numpy().reshape(-1, 32), want)


# ---- the mixed road: launches above SHA3_COOP_MAX ----------------------------------------------------------------------------------------
def _mixed(coop, plain, lens):
    """-> rows the coop context counted for this launch; the digests are checked against hashlib and against the plain context"""
    n = len(lens)
    assert n > SHA3_COOP_MAX
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    arena = np.random.default_rng(n + int(off[-1])).integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    want = _digests([arena[off[i]:off[i + 1]].tobytes() for i in range(n)])
    before = coop.sha3_coop_rows()
    got = coop.sha3_256_batch(arena, off)
    bad = _bad_rows(got, want)
    assert not bad, "rows (length) that disagree with hashlib.sha3_256: %s" % [(i, lens[i]) for i in bad[:8]]
    assert (plain.sha3_256_batch(arena, off) == got).all() and plain.sha3_coop_rows() == 0
    return coop.sha3_coop_rows() - before


def _expected_long_rows(lens, arena_bytes):
    """launch_sha3_256_mixed's rule: long = more than max(2048, mean + mean / 4) bytes; the first two long ones of every 64 rows"""
    mean = arena_bytes // len(lens)
    long_over = max(2048, mean + mean // 4)
    return sum(min(2, sum(1 for ln in lens[g:g + 64] if ln > long_over)) for g in range(0, len(lens), 64))


def test_mixed_road_one_two_and_three_long_messages_in_a_group_of_64(coop, plain):
    n = SHA3_COOP_MAX + 64
    lens = [200] * n
    lens[64 * 3 + 17] = 4096                                            # one in group 3
    lens[64 * 9 + 0] = lens[64 * 9 + 63] = 4096                         # two in group 9: the group's first and last row
    lens[64 * 20 + 5] = lens[64 * 20 + 6] = lens[64 * 20 + 40] = 4096   # three in group 20: the third stays on one lane
    assert _expected_long_rows(lens, sum(lens)) == 5
    assert _mixed(coop, plain, lens) == 5


def test_mixed_road_a_long_message_in_the_last_partial_group(coop, plain):
    n = SHA3_COOP_MAX + 64 + 37                                         # (a row count with a partial last group of 64: 37 rows)
    lens = [200] * n
    lens[n - 1] = 4096
    assert _expected_long_rows(lens, sum(lens)) == 1
    assert _mixed(coop, plain, lens) == 1


def test_mixed_road_all_messages_long(coop, plain):
    """every message 4 KiB: none is above a quarter more than the launch's average, so the launcher's guess takes none out - and all
    4 KiB messages but one a tenth as long: still none; every row goes through the one-lane half of the mixed kernel"""
    n = SHA3_COOP_MAX + 64
    assert _expected_long_rows([4096] * n, 4096 * n) == 0
    assert _mixed(coop, plain, [4096] * n) == 0
    lens = [4096] * n
    lens[100] = 400
    assert _mixed(coop, plain, lens) == 0


# ---- hash -> verify ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 65])
def test_hash_then_verify_valid_rows_beside_twins_with_one_bit_flipped(coop, plain, n):
    rng = np.random.default_rng(n)
    base = [bytes(rng.integers(0, 256, size=int(ln), dtype=np.uint8)) for ln in rng.integers(1, 420, size=n)]
    b = coracle.make_batch(n, seed=900 + n, digests=_digests(base))
    msgs = list(base)
    for i in range(1, n, 2):                                            # odd rows: the signature is over the message, the message has one bit flipped
        m = bytearray(msgs[i]); m[len(m) // 2] ^= 0x20; msgs[i] = bytes(m)
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)
    arena = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    want = np.array([i % 2 for i in range(n)], dtype=np.uint8)
    cols = dict(qx=b["qx"], qy=b["qy"], r=b["r"], s=b["s"])
    bits, st = coop.sha3_256_p256_verify_batch(arena, off, **cols)
    bits0, st0 = plain.sha3_256_p256_verify_batch(arena, off, **cols)
    assert (st == want).all() and (bits == (want == 0)).all() and (st == st0).all() and (bits == bits0).all()
    # the described batch under FABGPU_IDB_SHA3_256: the same rows as spans, each behind one shared prefix of 137 bytes cut off its front
    pre = bytes(rng.integers(0, 256, size=137, dtype=np.uint8))
    whole = [pre + m for m in base]
    b2 = coracle.make_batch(n, seed=950 + n, digests=_digests(whole))
    body = pre + b"".join(msgs)
    spans = np.stack([137 + off[:-1], 137 + off[1:]], axis=1).astype(np.uint32).reshape(-1)
    kw = dict(qx=b2["qx"], qy=b2["qy"], pre_off=np.array([0, 137], dtype=np.uint32), pre_idx=np.zeros(n, dtype=np.uint32), spans=True, sha3=True,
              want_digests=True)
    a2 = np.frombuffer(body, dtype=np.uint8)
    res = coop.identity_verify_batch(a2, spans, b2["r"], b2["s"], **kw)
    res0 = plain.identity_verify_batch(a2, spans, b2["r"], b2["s"], **kw)
    assert (res[1] == want).all() and (res[0] == (want == 0)).all()
    assert (res[1] == res0[1]).all() and (res[0] == res0[0]).all() and (res[-1] == res0[-1]).all()
    assert not _bad_rows(res[-1], _digests([pre + m for m in msgs]))
    assert plain.sha3_coop_rows() == 0


# ---- the provider's option ---------------------------------------------------------------------------------------------------------------
def test_provider_option_sha3_coop():
    csp = fabgpu.GPUCSP(device=0, hash_sha3=1, sha3_coop=1)
    try:
        assert csp.get_option("sha3_coop") == 1 and csp.sha3_coop_rows() == 0
        for m in (b"", b"abc", bytes(range(256)) * 9):
            assert csp.hash(m, fabgpu.SHA3_256Opts()) == _sha3(m)
        assert csp.sha3_coop_rows() == 3
        assert csp.set_option("sha3_coop", 0) == 1
        assert csp.hash(b"abc", fabgpu.SHA3_256Opts()) == _sha3(b"abc") and csp.sha3_coop_rows() == 3
    finally:
        csp.close()
    csp = fabgpu.GPUCSP(device=0, hash_sha3=1)
    try:
        assert csp.get_option("sha3_coop") == 0
        assert csp.hash(b"abc", fabgpu.SHA3_256Opts()) == _sha3(b"abc") and csp.sha3_coop_rows() == 0
        assert csp.set_option("sha3_coop", 1) == 0
        assert csp.hash(b"abc", fabgpu.SHA3_256Opts()) == _sha3(b"abc") and csp.sha3_coop_rows() == 1
    finally:
        csp.close()
