"""The device hash kernels at the places random lengths at small offsets do not reach (run with -m gpu on an MI355X):

  A  arena offsets of 2^31 and more - a byte offset is a u32 and an arena may be 2^32 - 1 bytes: every hash road through the
     device-resident entry points over ONE buffer of 2^32 - 3 bytes, messages starting, ending and crossing at 2^31, at 3 * 2^30 and
     in the buffer's last bytes (one ending on its last byte), at all four byte phases, prefixes on one side of 2^31 and their
     suffixes on the other; and the host entry point over an arena just above 2^31 bytes;
  B  the long-message split of sha256_mixed_kernel: which messages of a group of 64 the scan wavefront takes and the lane wavefront
     leaves, built group by group (none, lane 0, lane 63, eight, nine, twenty, all 64, the partial last group): consecutive offsets
     and 64-thread workgroups through the hash entry point, (start, end) pairs and 256-thread workgroups through a block pass;
  C  the seam of the two-span eight-lane road (sha256_coop_ex with a prefix): prefix length x suffix length x the two byte phases.

Everything against hashlib on the exact bytes, bit for bit; verdicts and statuses against the C oracle."""
import hashlib

import numpy as np
import pytest

import coracle
import fabgpu
from test_gpu_parity import ctx  # noqa: F401  (the five context configurations of the parity file)

pytestmark = pytest.mark.gpu

T31 = 1 << 31
HIGH_BYTES = (1 << 32) - 3                     # not a multiple of 4: the last dword of the allocation is a partial one
SENTINEL = 0xA5


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _sentinel_rows(n):
    import torch
    return torch.full((n, 32), SENTINEL, dtype=torch.uint8, device="cuda")


def _digests(t, n):
    """n x 32 digest bytes off the device; every row must have been written"""
    import torch
    torch.cuda.synchronize()
    d = t.cpu().numpy()
    untouched = np.nonzero((d == SENTINEL).all(axis=1))[0]
    assert untouched.size == 0, "digest rows never written: %s" % untouched[:20].tolist()
    return d


def _rows(digests):
    return np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32)


def _mismatches(got, want):
    return np.nonzero((got != want).any(axis=1))[0].tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# A. offsets of 2^31 and more
# ---------------------------------------------------------------------------------------------------------------------------
class _HighArena:
    """2^32 - 3 device bytes, allocated and never filled; random bytes written from the host into three windows only."""
    WINDOWS = ((T31 - (64 << 10), T31 + (256 << 10)), (3 * (1 << 30) - (8 << 10), 3 * (1 << 30) + (8 << 10)), (HIGH_BYTES - (8 << 10), HIGH_BYTES))

    def __init__(self):
        import torch
        self.buf = torch.empty(HIGH_BYTES, dtype=torch.uint8, device="cuda")
        rng = np.random.default_rng(231)
        self.host = []
        for lo, hi in self.WINDOWS:
            b = rng.integers(0, 256, size=hi - lo, dtype=np.uint8)
            self.buf[lo:hi].copy_(torch.from_numpy(b))
            self.host.append(b)
        torch.cuda.synchronize()
        self.ptr = self.buf.data_ptr()

    def bytes(self, a, b):
        if b <= a:
            return b""
        for (lo, hi), h in zip(self.WINDOWS, self.host):
            if lo <= a and b <= hi:
                return h[a - lo:b - lo].tobytes()
        raise AssertionError("[%#x, %#x) is not inside a written window" % (a, b))


@pytest.fixture(scope="module")
def high():
    import torch
    torch.cuda.set_device(0)
    h = _HighArena()
    yield h
    del h.buf
    torch.cuda.empty_cache()


def _flat(rng, lo, hi, n, forced=(), hole=None):
    """n + 1 ascending offsets in [lo, hi] (consecutive messages, some empty): the forced points among them, none inside `hole`"""
    pts = set(int(p) for p in forced)
    pts.update((lo, hi))
    while len(pts) < n - 3:
        p = int(rng.integers(lo, hi))
        if hole is None or not (hole[0] < p < hole[1]):
            pts.add(p)
    pts = sorted(pts)
    pts += [pts[-1]] * (n + 1 - len(pts))                 # (empty messages at the end)
    return np.array(pts, dtype=np.uint64).astype(np.uint32)


def _high_offset_lists(n):
    """Offset lists of n consecutive messages each, as (name, off): around 2^31 with one message crossing it at each byte phase and
    with messages starting and ending on 2^31 and on the three bytes on either side; the same around 3 * 2^30; the buffer's last
    bytes, the last message ending on the last byte, the first starting at each phase."""
    rng = np.random.default_rng(232 + n)
    out = []
    span = 90 * n                                          # about 90 bytes a message, a few of several hundred (more than one eight-block chunk)
    for name, base, room in (("2^31", T31, (60 << 10, 250 << 10)), ("3*2^30", 3 * (1 << 30), (7 << 10, 7 << 10))):
        lo, hi = base - min(room[0], span // 3), base + min(room[1], span - span // 3)
        for v in range(4):                                 # a message [base - 300 + v, base + 1100 + v): crosses, 22 blocks
            hole = (base - 300 + v, base + 1100 + v)
            out.append(("%s crossing, phase %d" % (name, v), _flat(rng, lo + v, hi, n, forced=hole, hole=hole)))
        out.append(("%s on the boundary" % name, _flat(rng, lo, hi, n, forced=[base + d for d in (-64, -3, -2, -1, 0, 1, 2, 3, 4, 64, 65)])))
    lo = HIGH_BYTES - min(8 << 10, span)
    for v in range(4):
        out.append(("the last bytes, phase %d" % v, _flat(rng, lo + v, HIGH_BYTES, n, forced=[HIGH_BYTES - d for d in (1, 2, 3, 4, 5, 64, 65, 700)],
                                                          hole=(HIGH_BYTES - 700, HIGH_BYTES - 65))))
    return out


def _want(high, off, algo):
    return _rows([algo(high.bytes(int(a), int(b))).digest() for a, b in zip(off[:-1], off[1:])])


@pytest.mark.parametrize("n", [200, 2049 + 37])           # eight lanes on a message; beyond 2 048: sha256_mixed_kernel, one lane each
def test_sha256_batch_dev_at_offsets_of_2_to_the_31_and_more(ctx, high, n):
    """(With an arena of 4 GiB the mixed launch's threshold - a quarter above arena / n - lies far above every message here: its
    lanes hash them all.  Its eight-lane side has the next test.)"""
    bad = []
    for name, off in _high_offset_lists(n):
        out = _sentinel_rows(n)
        ctx.sha256_batch_dev(n, high.ptr, HIGH_BYTES, _dev(off).data_ptr(), out.data_ptr())
        got = _digests(out, n)
        bad += [(name, hex(int(off[i])), int(off[i + 1]) - int(off[i])) for i in _mismatches(got, _want(high, off, hashlib.sha256))]
    assert not bad, "(list, start, length) whose digest is not hashlib's: %s" % bad[:40]


def test_mixed_launch_hashes_its_long_messages_on_eight_lanes_at_offsets_of_2_to_the_31_and_more(ctx, high):
    """The scan side of sha256_mixed_kernel above 2^31.  The launch calls a message long from a quarter above arena_bytes / n: with the
    4 GiB arena and 100 069 messages that is 53 650 bytes, so five messages of 53 651 to 70 000 bytes - one wholly below 2^31, one
    across it, three above, at four byte phases, on lane 0 and lane 63 of one group, alone in a group, and in the last slot of the
    partial last group - go to eight lanes each; four short fillers and 100 060 empty messages stay on their lanes."""
    n = 64 * 1563 + 37
    mean = HIGH_BYTES // n
    long_over = max(2048, mean + mean // 4)                # launch_sha256_mixed
    assert long_over == 53650
    lens = np.zeros(n, dtype=np.int64)
    placed = {64 * 5: 60001, 64 * 5 + 1: 536, 64 * 5 + 63: 63002, 64 * 5 + 64: 3, 64 * 700 + 17: 61003, 64 * 700 + 18: 2,
              64 * 1500 + 8: 70000, 64 * 1500 + 9: 2, n - 1: long_over + 1}
    for i, L in placed.items():
        lens[i] = L
    start = T31 - 65535
    off64 = start + np.concatenate([[0], np.cumsum(lens)])
    off = off64.astype(np.uint64).astype(np.uint32)
    assert int(off64[-1]) <= T31 + (256 << 10) and n % 64 == 37 and int((lens > long_over).sum()) == 5
    assert off64[64 * 5 + 1] < T31 and off64[64 * 5 + 63] < T31 < off64[64 * 5 + 64] and off64[64 * 700 + 17] > T31      # below, across, above
    assert sorted(int(off64[i]) & 3 for i in (64 * 5, 64 * 5 + 63, 64 * 700 + 17, 64 * 1500 + 8)) == [0, 1, 2, 3]
    want = np.tile(np.frombuffer(hashlib.sha256(b"").digest(), dtype=np.uint8), (n, 1))
    for i in placed:
        want[i] = np.frombuffer(hashlib.sha256(high.bytes(int(off64[i]), int(off64[i + 1]))).digest(), dtype=np.uint8)
    out = _sentinel_rows(n)
    ctx.sha256_batch_dev(n, high.ptr, HIGH_BYTES, _dev(off).data_ptr(), out.data_ptr())
    bad = _mismatches(_digests(out, n), want)
    assert not bad, "(index, lane, start, length) whose digest is not hashlib's: %s" % [(i, i % 64, hex(int(off64[i])), int(lens[i])) for i in bad[:40]]


@pytest.mark.parametrize("n", [200, 2049 + 37])
def test_sha3_256_batch_dev_at_offsets_of_2_to_the_31_and_more(ctx, high, n):
    bad = []
    for name, off in _high_offset_lists(n):
        out = _sentinel_rows(n)
        ctx.sha3_256_batch_dev(n, high.ptr, HIGH_BYTES, _dev(off).data_ptr(), out.data_ptr())
        got = _digests(out, n)
        bad += [(name, hex(int(off[i])), int(off[i + 1]) - int(off[i])) for i in _mismatches(got, _want(high, off, hashlib.sha3_256))]
    assert not bad, "(list, start, length) whose digest is not hashlib's: %s" % bad[:40]


POOL_SEED, POOL_KEYS = 240, 6


def _signed(ctx, digests, seed, nkeys=POOL_KEYS):
    """Signatures by ONE pool of six signers (make_pool_batch draws the pool from its seed alone, and registering a key a context already
    holds returns its id: six keys per context whatever the number of calls): every fifth row signed over its digest with ONE BIT
    flipped, which bit by `seed` (the one-bit-off twin of a valid row: only a hash of the exact bytes tells them apart), a fifth of
    the rows broken otherwise (another signer, high S, r + 1).  -> batch, key ids, the oracle's statuses for the true digests."""
    signed_over = digests.copy()
    signed_over[::5, 31 - (seed % 32)] ^= np.uint8(1 << (seed % 8))
    b = coracle.make_pool_batch(digests.shape[0], seed=POOL_SEED, nkeys=nkeys, invalid_frac=0.2, digests=signed_over)
    ids = np.array([ctx.key_register(b["pool_qx"][j].tobytes(), b["pool_qy"][j].tobytes()) for j in range(nkeys)], dtype=np.uint32)
    want = coracle.verify_batch(b["qx"], b["qy"], digests, b["r"], b["s"])      # e = the true digest: the message is what counts
    assert (want == 0).any() and (want != 0).any()
    return b, ids[b["key_index"]], want


def _verdicts(words, status, n, want, what):
    import torch
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    bits = fabgpu.unpack_bits(words.cpu().numpy().view(np.uint64), n)
    wrong = np.nonzero(st != want)[0]
    assert wrong.size == 0, "%s: rows %s answer %s, the oracle %s" % (what, wrong[:20].tolist(), st[wrong[:20]].tolist(), want[wrong[:20]].tolist())
    assert (bits == (want == 0)).all(), what


def _out(n):
    import torch
    return torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda"), torch.full((n,), 9, dtype=torch.uint8, device="cuda")


def test_fused_verify_dev_at_offsets_of_2_to_the_31_and_more(ctx, high):
    """Fresh keys (two lanes per signature; one lane under the one-lane configuration), registered keys (eight lanes and the eight-lane
    hash under auto, the fused keyed kernel under no-wide) and the SHA3-256 twins, over the same offset lists."""
    n = 200
    for k, (name, off) in enumerate(_high_offset_lists(n)):
        d_off = _dev(off)
        for algo, fresh, keyed in ((hashlib.sha256, ctx.sha256_p256_verify_batch_dev, ctx.sha256_p256_verify_batch_keyed_dev),
                                   (hashlib.sha3_256, ctx.sha3_256_p256_verify_batch_dev, ctx.sha3_256_p256_verify_batch_keyed_dev)):
            b, key_id, want = _signed(ctx, _want(high, off, algo), seed=240 + k % 4)
            t = {f: _dev(b[f]) for f in ("qx", "qy", "r", "s")}
            words, status = _out(n)
            fresh(n, high.ptr, HIGH_BYTES, d_off.data_ptr(), t["qx"].data_ptr(), t["qy"].data_ptr(), t["r"].data_ptr(), t["s"].data_ptr(),
                  words.data_ptr(), status.data_ptr())
            _verdicts(words, status, n, want, "%s, %s, fresh keys" % (name, algo.__name__))
            words, status = _out(n)
            d_id = _dev(key_id)
            keyed(n, high.ptr, HIGH_BYTES, d_off.data_ptr(), d_id.data_ptr(), t["r"].data_ptr(), t["s"].data_ptr(), words.data_ptr(), status.data_ptr())
            _verdicts(words, status, n, want, "%s, %s, registered keys" % (name, algo.__name__))


def _identity_dev(ctx, high, off, pre_off, pre_idx, spans, keyed, sha3, gather, seed):
    """fabgpu_identity_verify_batch_dev over the high arena -> checks digests (hashlib), statuses (oracle), gathered digests (hashlib)"""
    off, pre_off = np.asarray(off, dtype=np.uint32), np.asarray(pre_off, dtype=np.uint32)
    pairs = (lambda a: a.reshape(-1, 2)) if spans else (lambda a: np.stack([a[:-1], a[1:]], axis=1))
    mo, po = pairs(off), pairs(pre_off)
    n, m = mo.shape[0], po.shape[0]
    algo = hashlib.sha3_256 if sha3 else hashlib.sha256
    pre = [high.bytes(int(a), int(b)) for a, b in po]
    msgs = [(pre[pi] if pi < m else b"") + high.bytes(int(a), int(b)) for pi, (a, b) in zip(pre_idx.tolist(), mo)]
    dig = _rows([algo(x).digest() for x in msgs])
    b, key_id, want = _signed(ctx, dig, seed)
    t = {f: _dev(b[f]) for f in ("qx", "qy", "r", "s")}
    keep = [_dev(off), _dev(pre_off), _dev(pre_idx), _dev(key_id), _sentinel_rows(n), _dev(np.zeros(m * 200 + 64, np.uint8))]
    words, status = _out(n)
    d = fabgpu._IdBatch()
    d.n, d.arena, d.arena_bytes, d.off = n, high.ptr, HIGH_BYTES, keep[0].data_ptr()
    d.n_prefixes, d.pre_off, d.pre_idx = m, keep[1].data_ptr(), keep[2].data_ptr()
    d.r, d.s = t["r"].data_ptr(), t["s"].data_ptr()
    if keyed:
        d.key_id = keep[3].data_ptr()
    else:
        d.qx, d.qy = t["qx"].data_ptr(), t["qy"].data_ptr()
    d.verdict_bits, d.status, d.digests = words.data_ptr(), status.data_ptr(), keep[4].data_ptr()
    d.flags = (1 if spans else 0) | (fabgpu.IDB_SHA3_256 if sha3 else 0)
    if gather is not None:
        g = np.asarray(gather, dtype=np.uint32).reshape(-1, 6)
        goff = np.concatenate([[0], np.cumsum((g[:, 1::2].astype(np.int64) - g[:, 0::2]).sum(axis=1))]).astype(np.uint32)
        gk = [_dev(g), _dev(goff), _sentinel_rows(g.shape[0]), _dev(np.zeros(int(goff[-1]) + 64, np.uint8))]
        d.n_gather, d.gather_spans, d.gather_off, d.gather_digests = g.shape[0], gk[0].data_ptr(), gk[1].data_ptr(), gk[2].data_ptr()
        d.gather_scratch, d.gather_scratch_bytes = gk[3].data_ptr(), int(goff[-1]) + 64
    what = "n %d %s %s %s" % (n, "spans" if spans else "offsets", "keyed" if keyed else "fresh", "sha3" if sha3 else "sha256")
    ctx.identity_verify_batch_dev(d, keep[5].data_ptr())
    got = _digests(keep[4], n)
    badd = _mismatches(got, dig)
    assert not badd, "%s: digests of rows %s (prefix %s, span %s) are not hashlib's" % (
        what, badd[:20], [int(pre_idx[i]) for i in badd[:20]], [tuple(hex(int(x)) for x in mo[i]) for i in badd[:20]])
    _verdicts(words, status, n, want, what)
    if gather is not None:
        gw = _rows([hashlib.sha256(b"".join(high.bytes(int(r[2 * p]), int(r[2 * p + 1])) for p in range(3))).digest() for r in g])   # (SHA-256 whatever the family)
        badg = _mismatches(_digests(gk[2], g.shape[0]), gw)
        assert not badg, "%s: gathered digests %s are not hashlib's" % (what, badg)


def _prefix_lists(region, lens):
    """prefixes back to back inside region -> m + 1 ascending offsets"""
    pos = region
    po = [pos]
    for L in lens:
        pos += L
        po.append(pos)
    return po


PRE_LENS = (0, 1, 55, 56, 63, 64, 65, 119, 127, 128, 129, 135, 136, 137, 272, 300, 1023, 1024, 1025)


@pytest.mark.parametrize("n", [600, 2049 + 51])          # keyed, auto: the two-span eight-lane road up to 2 048; mid-states and the tail read at a high address beyond
@pytest.mark.parametrize("keyed", [True, False])
def test_identity_dev_prefix_and_suffix_on_opposite_sides_of_2_to_the_31(ctx, high, keyed, n):
    rng = np.random.default_rng(250 + n)
    m = len(PRE_LENS)
    pre_idx = rng.integers(0, m, size=n).astype(np.uint32)
    pre_idx[rng.random(n) < 0.1] = 0xFFFFFFFF
    lo1, mid_hi = T31 - (60 << 10), T31 + (250 << 10)
    for sha3 in (False, True):
        # offsets mode, prefixes above 2^31 (one list starting on 2^31 + 1, one around 3 * 2^30), suffixes below and crossing; then the reverse
        below = _flat(rng, lo1 + 3, T31 + 700, n, forced=(T31 - 300, T31 + 700), hole=(T31 - 300, T31 + 700))
        above = _flat(rng, T31 + 9001, mid_hi, n)
        for k, (off, pre_at) in enumerate(((below, T31 + 1), (below, 3 * (1 << 30) - 1500), (above, lo1 + 2), (above, T31 - 2000))):
            _identity_dev(ctx, high, off, _prefix_lists(pre_at, PRE_LENS), pre_idx, False, keyed, sha3, None, seed=260 + k)
        # spans mode: rows in any order from both sides, the arena's end among them; prefixes as pairs from both sides; gathered
        # messages of three pieces taken from both sides of 2^31
        pairs = np.concatenate([np.stack([below[:-1], below[1:]], axis=1)[: n // 2], np.stack([above[:-1], above[1:]], axis=1)[: n - n // 2 - 4],
                                np.array([[HIGH_BYTES - L, HIGH_BYTES] for L in (1, 64, 65, 700)], dtype=np.uint32)])
        pairs = pairs[rng.permutation(n)]
        pa, pb = _prefix_lists(T31 - 5000, PRE_LENS[: m // 2]), _prefix_lists(T31 + 3, PRE_LENS[m // 2:])
        pre_pairs = np.array([[a, b] for a, b in zip(pa[:-1], pa[1:])] + [[a, b] for a, b in zip(pb[:-1], pb[1:])], dtype=np.uint32)
        gather = [[T31 - 100 - j, T31 - 3, T31 + 5 + j, T31 + 900, HIGH_BYTES - 40 - j, HIGH_BYTES] for j in range(8)] + \
                 [[T31 - 2500 + j, T31 + 2500 + j, 7, 7, T31 + 1, T31 + 1] for j in range(4)]
        _identity_dev(ctx, high, pairs.reshape(-1), pre_pairs.reshape(-1), pre_idx, True, keyed, sha3, gather, seed=270)


def test_host_arena_just_above_2_to_the_31_bytes(ctx):
    """The host entry point stages the span its offsets reference: a handful of messages at the end of an arena of 2^31 + 4 099 bytes
    (allocated, untouched but for its end)."""
    size = T31 + 4099
    arena = np.zeros(size, dtype=np.uint8)
    rng = np.random.default_rng(280)
    arena[T31 - 3000:] = rng.integers(0, 256, size=size - T31 + 3000, dtype=np.uint8)
    off = np.array([T31 - 3000, T31 - 2999, T31 - 300, T31 + 300, T31 + 300, T31 + 301, T31 + 2349, size - 65, size], dtype=np.uint64).astype(np.uint32)
    want = _rows([hashlib.sha256(arena[int(a):int(b)].tobytes()).digest() for a, b in zip(off[:-1], off[1:])])
    assert not _mismatches(ctx.sha256_batch(arena, off), want)
    want3 = _rows([hashlib.sha3_256(arena[int(a):int(b)].tobytes()).digest() for a, b in zip(off[:-1], off[1:])])
    assert not _mismatches(ctx.sha3_256_batch(arena, off), want3)


# ---------------------------------------------------------------------------------------------------------------------------
# B. which messages of a group of 64 the scan wavefront of sha256_mixed_kernel takes
# ---------------------------------------------------------------------------------------------------------------------------
LONG = (2049, 2111, 2112, 3400)
LONG_OVER = 2048


def _mixed_groups(partial_before):
    """Lengths of n messages by group of 64: each kind of group four times with its long messages at other lanes, the not-long
    neighbours 2 048 and 2 047 beside them, and a last group of 37 whose last two slots are long, behind `partial_before` earlier
    long ones (7: they are the group's 8th and 9th - the scan wavefront takes one and leaves the other to its lane)."""
    rng = np.random.default_rng(290)
    lens = []
    nlong = 0

    def group(size, long_at, near_at=()):
        nonlocal nlong
        g = [int(x) for x in rng.integers(0, 201, size=size)]
        for k in range(0, size, 3):
            g[k] = 0                                      # (empty messages keep the launch inside its byte budget)
        for k in near_at:
            g[k] = 2048 - (k & 1)
        for k in long_at:
            g[k] = LONG[nlong % 4]
            nlong += 1
        lens.extend(g)
    for rep in range(4):
        pick = (lambda c: sorted(int(x) for x in rng.choice(64, size=c, replace=False))) if rep else (lambda c: list(range(c)))
        group(64, [])
        group(64, [0], near_at=[1, 2])
        group(64, [63], near_at=[61, 62])
        group(64, pick(8), near_at=[k for k in (5, 40) if rep == 0] + ([8, 9] if rep == 0 else []))
        group(64, pick(9) if rep != 1 else list(range(55, 64)))
        group(64, pick(20))
        group(64, list(range(64)))
        group(64, [], near_at=[0, 63])                    # at the threshold and one below: nobody is long
    group(64, [0, 1, 2, 3, 4, 5, 6, 7, 63])               # the ninth long one on the last lane
    group(37, list(range(partial_before)) + [35, 36])
    return np.array(lens, dtype=np.int64)


@pytest.mark.parametrize("partial_before", [0, 7])
def test_mixed_kernel_long_message_selection_group_by_group(ctx, partial_before):
    import torch
    lens = _mixed_groups(partial_before)
    n = lens.size
    assert 2049 <= n <= 2400 and n % 64 == 37
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    arena_bytes = int(off[-1]) + 5
    assert arena_bytes <= 1638 * n and max(2048, arena_bytes // n + arena_bytes // n // 4) == LONG_OVER   # the launcher's threshold is its floor
    per_group = [(lens[g:g + 64] > LONG_OVER).sum() for g in range(0, n, 64)]
    assert {0, 1, 8, 9, 20, 64} <= set(int(x) for x in per_group) and per_group[-1] == partial_before + 2
    arena = np.random.default_rng(291).integers(0, 256, size=arena_bytes, dtype=np.uint8)
    want = _rows([hashlib.sha256(arena[int(a):int(b)].tobytes()).digest() for a, b in zip(off[:-1], off[1:])])
    d_arena, d_off, out = _dev(arena), _dev(off), _sentinel_rows(n)
    torch.cuda.synchronize()
    ctx.sha256_batch_dev(n, d_arena.data_ptr(), arena_bytes, d_off.data_ptr(), out.data_ptr())
    bad = _mismatches(_digests(out, n), want)
    assert not bad, "(group, lane, length) whose digest is not hashlib's: %s" % [(i // 64, i % 64, int(lens[i])) for i in bad[:40]]
    assert not _mismatches(ctx.sha256_batch(arena, off), want)       # and through the host entry point's staging


def _envelope_payload(env):
    """common.Envelope{1 payload, 2 signature}: the bytes of field 1 (what the creator signed and the pass hashes per envelope)"""
    assert env[0] == 0x0A
    v = s = 0
    i = 1
    while True:
        c = env[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            break
    return bytes(env[i:i + v])


@pytest.fixture(scope="module")
def grouped_block():
    """A block of 2 149 transactions whose payload lengths are chosen group by group of 64 like _mixed_groups: about 4.1 KB (short) or
    6.6 to 8.4 KB (long: the generator's extension bytes).  -> block, payloads, which transactions were built long"""
    import blockgen
    fx = blockgen.fixture_signers()
    rng = np.random.default_rng(310)
    sign = blockgen.make_signer(311)
    design = []

    def group(size, long_at):
        g = [False] * size
        for k in long_at:
            g[k] = True
        design.extend(g)
    for rep in range(4):
        pick = (lambda c: [int(x) for x in rng.choice(64, size=c, replace=False)]) if rep else (lambda c: list(range(c)))
        group(64, [])
        group(64, [0])
        group(64, [63])
        group(64, pick(8))
        group(64, pick(9) if rep != 1 else list(range(55, 64)))
        group(64, pick(20))
        group(64, list(range(64)))
        group(64, [])
    group(64, [0, 1, 2, 3, 4, 5, 6, 7, 63])
    group(37, [0, 1, 2, 3, 4, 5, 6, 35, 36])             # the last two valid slots: the partial group's 8th and 9th long
    envs, nlong = [], 0
    for t, is_long in enumerate(design):
        ext = (2600, 3100, 3101, 4400)[nlong % 4] if is_long else int(rng.integers(0, 201))
        nlong += 1 if is_long else 0
        picks = [int(j) for j in rng.choice(4, size=3, replace=False)]
        envs.append(blockgen.endorser_tx(t, rng, fx[4 + t % 2], [fx[j] for j in picks], sign, ext_bytes=ext))
    return blockgen.bb.block(1, envs), [_envelope_payload(e) for e in envs], np.array(design)


def test_block_pass_hashes_payloads_group_by_group_in_spans_mode_and_256_thread_workgroups(grouped_block):
    """The other form of sha256_mixed_kernel: (start, end) pairs instead of consecutive offsets, and workgroups of four wavefronts that
    keep CUs to themselves - how a block pass of more than 2 048 transactions hashes every envelope's payload before it has walked
    anything (the creators' digests are scattered from there).  The same groups of 64: none long, lane 0, lane 63, eight, nine, twenty,
    all 64, and the partial last group with long payloads in its last two slots as its 8th and 9th.  (A length exactly at the
    threshold is the offsets test's: a payload's length cannot be set to the byte through the generator.)  Every creator's digest
    against hashlib of its payload; a slot written by nobody, or by the wrong side, is a wrong digest."""
    blk, payloads, design = grouped_block
    n = len(payloads)
    assert 2049 <= n <= 2400 and n % 64 == 37
    lens = np.array([len(p) for p in payloads])
    arena_bytes = (len(blk) + 3) // 4 * 4 + 64                                   # what the pass hands the launch: the staged block
    mean = arena_bytes // n
    long_over = max(2048, mean + mean // 4)                                       # launch_sha256_mixed
    assert (lens[design] > long_over + 200).all() and (lens[~design] < long_over - 200).all(), (long_over, lens[design].min(), lens[~design].max())
    per_group = [int(design[g:g + 64].sum()) for g in range(0, n, 64)]
    assert {0, 1, 8, 9, 20, 64} <= set(per_group) and per_group[-1] == 9 and design[n - 2:].all()
    want = _rows([hashlib.sha256(p).digest() for p in payloads])
    csp = fabgpu.GPUCSP(device=0)
    try:
        csp.set_option("pass_stage_min_bytes", 1)
        before = fabgpu.pass_routes(csp)
        for seq in (1, 2):                                                        # (the second pass: the signers have their tables by then)
            out = fabgpu.preverify_block2(csp, blk, block_seq=seq)
            assert (out["tx_flags"] == 0).all() and (out["tuple_status"] == 0).all()
            creators = np.nonzero(out["tuple_kind"] == 0)[0]
            assert out["tuple_tx"][creators].tolist() == list(range(n))
            sp = out["tuple_spans"][creators].astype(np.int64)
            assert (sp[:, 5] == lens).all() and all(out["arena"][a:a + L] == p for a, L, p in zip(sp[:, 4].tolist(), sp[:, 5].tolist(), payloads))
            assert out["tuple_hashed"][creators].all()
            bad = _mismatches(out["tuple_digest"][creators], want)
            assert not bad, "pass %d: (group, lane, payload length, long) whose digest is not hashlib's: %s" % (
                seq, [(t // 64, t % 64, int(lens[t]), bool(design[t])) for t in bad[:40]])
        after = fabgpu.pass_routes(csp)
        assert after["device_walks"] == before["device_walks"] + 2 and after["host_walks"] == before["host_walks"], (before, after)
    finally:
        csp.close()


# ---------------------------------------------------------------------------------------------------------------------------
# C. the seam of the two-span eight-lane road
# ---------------------------------------------------------------------------------------------------------------------------
SEAM_PL = (1, 2, 3, 4, 5, 55, 56, 57, 60, 61, 62, 63, 64, 65, 67, 119, 120, 127, 128, 129, 447, 448, 449, 509, 510, 511, 512, 513, 575, 576, 577)
SEAM_B = (0, 1, 2, 3, 4, 5, 7)
SEAM_TOTAL_MOD_64 = (55, 56, 63, 64, 65)


@pytest.fixture(scope="module")
def seam_grid():
    """prefix length x suffix length x (ps & 3) x (sb & 3): one arena, prefixes as spans, rows as spans; each row once signed over its
    digest and once as a broken twin.  -> arena, row spans, prefix spans, pre_idx, hashlib digests (computed once, shared)"""
    rng = np.random.default_rng(300)
    parts, pos = [], 0
    pre_span, pre_bytes = {}, {}
    for pl in SEAM_PL:
        for pa in range(4):
            pad = (pa - pos) & 3
            parts.append(b"\x5a" * pad); pos += pad
            p = rng.integers(0, 256, size=pl, dtype=np.uint8).tobytes()
            pre_span[(pl, pa)] = (pos, pos + pl); pre_bytes[(pl, pa)] = p
            parts.append(p); pos += pl
    keys = list(pre_span)
    rows, pre_idx, msgs = [], [], []
    for pl in SEAM_PL:
        sfx = sorted(set(SEAM_B) | set((t - pl) % 64 for t in SEAM_TOTAL_MOD_64))
        for b in sfx:
            for pa in range(4):
                for sa in range(4):
                    pad = (sa - pos) & 3
                    parts.append(b"\xc3" * pad); pos += pad
                    s = rng.integers(0, 256, size=b, dtype=np.uint8).tobytes()
                    parts.append(s)
                    rows.append((pos, pos + b)); pos += b
                    pre_idx.append(keys.index((pl, pa)))
                    msgs.append(pre_bytes[(pl, pa)] + s)
    arena = np.frombuffer(b"".join(parts) + b"\0" * 3, dtype=np.uint8)
    rows = np.array(rows, dtype=np.uint32)
    assert all((int(a) & 3) == (k % 4) for k, (a, _) in enumerate(rows))
    dig = _rows([hashlib.sha256(x).digest() for x in msgs])
    return dict(arena=arena, rows=rows, pre=np.array([pre_span[k] for k in keys], dtype=np.uint32), pre_idx=np.array(pre_idx, dtype=np.uint32), dig=dig)


def test_two_span_eight_lane_seam_grid_and_the_midstate_roads_agree(ctx, request, seam_grid):
    if "auto" not in request.node.callspec.id:
        pytest.skip("the two-span eight-lane road is the auto configuration's")
    g = seam_grid
    n = g["dig"].shape[0]
    b, key_id, want = _signed(ctx, g["dig"], seed=301)
    assert 2 * 2048 < n <= 8192 < 2 * n
    # launches of at most 2 048 rows: eight lanes on a message, prefix and suffix hashed whole.  All rows at once: the mid-state kernel
    # and one lane per message in front of the eight-lane verification.  All rows twice: the fused keyed kernel behind the mid-state kernel.
    launches = [np.arange(lo, min(n, lo + 2048)) for lo in range(0, n, 2048)] + [np.arange(n), np.concatenate([np.arange(n), np.arange(n)])]
    for sl in launches:
        bits, st, dig = ctx.identity_verify_batch(g["arena"], g["rows"][sl].reshape(-1), b["r"][sl], b["s"][sl], key_id=key_id[sl],
                                                  pre_off=g["pre"].reshape(-1), pre_idx=g["pre_idx"][sl], spans=True, want_digests=True)
        bad = [int(sl[i]) for i in _mismatches(dig, g["dig"][sl])]
        assert not bad, "launch of %d rows from %d: (prefix length, ps & 3, suffix length, sb & 3) whose digest is not hashlib's: %s" % (
            sl.size, sl[0], [(int(g["pre"][g["pre_idx"][i]][1] - g["pre"][g["pre_idx"][i]][0]), int(g["pre"][g["pre_idx"][i]][0]) & 3,
                              int(g["rows"][i][1] - g["rows"][i][0]), int(g["rows"][i][0]) & 3) for i in bad[:30]])
        assert (st == want[sl]).all() and (bits == (want[sl] == 0)).all(), (sl.size, int(sl[0]))
