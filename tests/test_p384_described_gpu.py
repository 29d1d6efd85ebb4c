"""fabgpu_identity_verify_batch_p384 on the GPU: the described batch of the P-384 stage of the block pass - prefix mid-states, spans,
the tail, the arena's end, offsets at and above 2^31 - against p384_ref + hashlib.

The reference is computed once (module fixture): 48 distinct (prefix, suffix) messages signed by three keys with p384_ref.sign, the
mutated rows' statuses from p384_ref.status; 257 rows are laid over them, every row with spans of its own in the arena."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import fabgpu
import p384_ref as ref

pytestmark = pytest.mark.gpu

PREFIX_LENS = [0, 1, 55, 56, 63, 64, 65, 119, 127, 128, 129]
SUFFIX_LENS = [0, 1, 8, 55, 56, 63, 64, 65]
NONE = 0xFFFFFFFF
N_ROWS = 257


@pytest.fixture(scope="module")
def ctx():
    c = fabgpu.Context(device=0)
    yield c
    c.close()


class Case:
    pass


@pytest.fixture(scope="module")
def case():
    rnd = random.Random(20384)
    keys = []
    for _ in range(3):
        d = rnd.randrange(1, ref.N)
        keys.append((d, ref.mul(d, ref.G)))
    prefixes = [rnd.randbytes(n) for n in PREFIX_LENS]
    # 48 combinations: every prefix (and "none") with four suffix lengths, chosen so that every suffix length and every residue asked
    # for (55, 56, 63, 0 of the total length modulo 64) occurs
    combos = []
    for p in range(12):
        for k in range(4):
            combos.append((p if p < 11 else None, SUFFIX_LENS[(2 * k + p) % 8]))
    combos[0] = (0, 55); combos[1] = (0, 56); combos[2] = (0, 63); combos[3] = (0, 64)      # prefix of length 0: the suffix decides
    signed = []                                                                              # per combo: (key index, suffix bytes, r, s)
    for ci, (p, sl) in enumerate(combos):
        suffix = rnd.randbytes(sl)
        msg = (prefixes[p] if p is not None else b"") + suffix
        k = ci % 3
        e = ref.hash_to_int(hashlib.sha256(msg).digest())
        r, s = ref.sign(keys[k][0], e, rnd.randrange(1, ref.N))
        signed.append((k, suffix, r, ref.low_s(s)))
    c = Case()
    arena = bytearray(rnd.randbytes(3))                     # (rows start at an odd address)
    pre_off = []
    for pbytes in prefixes:
        pre_off += [len(arena), len(arena) + len(pbytes)]
        arena += pbytes + rnd.randbytes(5)
    rows = []
    for i in range(N_ROWS):
        ci = (i * 7) % len(combos)
        p, sl = combos[ci]
        k, suffix, r, s = signed[ci]
        q = keys[k][1]
        start = len(arena)
        arena += suffix + rnd.randbytes(i % 3)
        msg = (prefixes[p] if p is not None else b"") + suffix
        kind = {5: "msgbit", 9: "prebit", 13: "high_s", 17: "range", 21: "offcurve", 0: "valid"}.get(i % 64 if i < 64 else 0, "valid")
        if kind == "msgbit":                                # the arena holds one bit more than was signed
            assert sl > 0
            arena[start] ^= 0x10
            msg = (prefixes[p] if p is not None else b"") + bytes(arena[start:start + sl])
        if kind == "prebit":                                # signed over a prefix with one bit flipped: rows 9 names a prefix of its own
            assert p is not None and len(prefixes[p]) > 0
            e2 = ref.hash_to_int(hashlib.sha256(bytes([prefixes[p][0] ^ 1]) + prefixes[p][1:] + suffix).digest())
            r, s = ref.sign(keys[k][0], e2, rnd.randrange(1, ref.N))
            s = ref.low_s(s)
        if kind == "high_s":
            s = ref.N - s
        if kind == "range":
            r = ref.N + 5
        if kind == "offcurve":
            q = (q[0], (q[1] + 1) % ref.P)
        rows.append(dict(p=p, start=start, end=start + sl, k=k, q=q, r=r, s=s, msg=msg, kind=kind))
    # the last row's suffix ends at the arena's last byte, and the arena's size is a multiple of 4 (the _dev form's condition)
    last = rows[-1]
    suffix = bytes(arena[last["start"]:last["end"]])
    del arena[last["start"]:]
    arena += rnd.randbytes((-(len(arena) + len(suffix))) % 4) + suffix
    last["start"], last["end"] = len(arena) - len(suffix), len(arena)
    assert last["end"] == len(arena) and len(arena) % 4 == 0 and last["end"] > last["start"]
    c.arena = np.frombuffer(bytes(arena), dtype=np.uint8).copy()
    c.pre_off = np.array(pre_off, dtype=np.uint32)
    c.off = np.array([[r_["start"], r_["end"]] for r_ in rows], dtype=np.uint32).reshape(-1)
    c.pre_idx = np.array([NONE if r_["p"] is None else r_["p"] for r_ in rows], dtype=np.uint32)
    c.qx = np.frombuffer(b"".join(ref.b48(r_["q"][0]) for r_ in rows), dtype=np.uint8).copy()
    c.qy = np.frombuffer(b"".join(ref.b48(r_["q"][1]) for r_ in rows), dtype=np.uint8).copy()
    c.r = np.frombuffer(b"".join(ref.b48(r_["r"]) for r_ in rows), dtype=np.uint8).copy()
    c.s = np.frombuffer(b"".join(ref.b48(r_["s"]) for r_ in rows), dtype=np.uint8).copy()
    c.digests = np.frombuffer(b"".join(hashlib.sha256(r_["msg"]).digest() for r_ in rows), dtype=np.uint8).reshape(-1, 32).copy()
    # statuses: p384_ref.status for every distinct (key, message, r, s) - 48 valid ones and the mutated rows
    memo = {}
    st = []
    for r_ in rows:
        key = (r_["q"], r_["msg"], r_["r"], r_["s"])
        if key not in memo:
            memo[key] = ref.status(r_["q"][0], r_["q"][1], ref.hash_to_int(hashlib.sha256(r_["msg"]).digest()), r_["r"], r_["s"])
        st.append(memo[key])
    c.status = np.array(st, dtype=np.uint8)
    c.rows, c.keys = rows, keys
    return c


def _take(c, n):
    return dict(arena=c.arena, off=c.off[:2 * n], r=c.r[:48 * n], s=c.s[:48 * n], qx=c.qx[:48 * n], qy=c.qy[:48 * n], pre_off=c.pre_off, pre_idx=c.pre_idx[:n],
                spans=True, want_digests=True)


def test_the_case_covers_what_it_must(case):
    kinds = [r["kind"] for r in case.rows]
    assert {"valid", "msgbit", "prebit", "high_s", "range", "offcurve"} <= set(kinds)
    assert set(case.status.tolist()) == {0, 1, 2, 3, 4}
    assert case.status[5] == 1 and case.status[9] == 1 and case.status[13] == 2 and case.status[17] == 3 and case.status[21] == 4
    assert {len(r["msg"]) % 64 for r in case.rows} >= {55, 56, 63, 0}
    assert {r["end"] - r["start"] for r in case.rows} == set(SUFFIX_LENS)
    used = [r["p"] for r in case.rows]
    assert set(used) == set(range(11)) | {None} and min(used.count(p) for p in range(11)) >= 2


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_verdicts_statuses_and_digests_equal_the_reference(ctx, case, n):
    ok, st, dig = ctx.identity_verify_batch_p384(**_take(case, n))
    assert np.array_equal(st, case.status[:n])
    assert np.array_equal(ok, case.status[:n] == 0)
    assert np.array_equal(dig, case.digests[:n])


@pytest.mark.parametrize("n", [1, 65, 257])
def test_no_verdict_bit_at_or_above_n(ctx, case, n):
    """the raw verdict words, pre-filled with ones: bits at and above n of the last word come back clear, words beyond it untouched"""
    a = _take(case, n)
    words = (n + 63) // 64
    bits = np.full(words + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    b = fabgpu._IdBatchP384()
    b.n, b.flags = n, fabgpu.IDB_SPANS
    keep = [np.ascontiguousarray(a[k]) for k in ("arena", "off", "r", "s", "qx", "qy", "pre_off", "pre_idx")]
    b.arena, b.off, b.r, b.s, b.qx, b.qy, b.pre_off, b.pre_idx = (x.ctypes.data for x in keep)
    b.n_prefixes = len(PREFIX_LENS)
    b.verdict_bits = bits.ctypes.data
    assert ctx._L.fabgpu_identity_verify_batch_p384(ctx._h, ctypes.byref(b)) == 0
    got = fabgpu.unpack_bits(bits[:words], words * 64)
    assert np.array_equal(got[:n], case.status[:n] == 0) and not got[n:].any()
    assert bits[words] == 0xFFFFFFFFFFFFFFFF


def _dev_batch(torch, a, n, n_prefixes, tail=None, tail_base=0):
    """the _dev form's descriptor over torch tensors -> (descriptor, mid scratch, out tensors, everything kept alive)"""
    t = {k: torch.from_numpy(np.array(a[k]).view(np.uint8)).cuda() for k in ("arena", "off", "r", "s", "qx", "qy", "pre_off", "pre_idx") if a.get(k) is not None}
    words = (n + 63) // 64
    out = dict(bits=torch.full((words + 1,), -1, dtype=torch.int64, device="cuda"), st=torch.full((n + 8,), 0xEE, dtype=torch.uint8, device="cuda"),
               dig=torch.full((n + 1, 32), 0xEE, dtype=torch.uint8, device="cuda"), mid=torch.zeros(max(1, n_prefixes) * 32, dtype=torch.uint8, device="cuda"))
    b = fabgpu._IdBatchP384()
    b.n, b.flags = n, fabgpu.IDB_SPANS
    b.arena, b.arena_bytes = t["arena"].data_ptr(), t["arena"].numel()
    b.off, b.r, b.s, b.qx, b.qy = (t[k].data_ptr() for k in ("off", "r", "s", "qx", "qy"))
    if n_prefixes:
        b.n_prefixes, b.pre_off, b.pre_idx = n_prefixes, t["pre_off"].data_ptr(), t["pre_idx"].data_ptr()
    if tail is not None:
        t["tail"] = torch.from_numpy(tail).cuda()
        b.tail, b.tail_base, b.tail_len = t["tail"].data_ptr(), tail_base, tail.size
    b.verdict_bits, b.status, b.digests = out["bits"].data_ptr(), out["st"].data_ptr(), out["dig"].data_ptr()
    return b, out, t


def _dev_results(torch, out, n):
    torch.cuda.synchronize()
    words = (n + 63) // 64
    bits = out["bits"].cpu().numpy().view(np.uint64)
    st, dig = out["st"].cpu().numpy(), out["dig"].cpu().numpy()
    # rows at or above n are never written
    assert bits[words] == 0xFFFFFFFFFFFFFFFF and (st[n:] == 0xEE).all() and (dig[n:] == 0xEE).all()
    return fabgpu.unpack_bits(bits[:words].copy(), n), st[:n], dig[:n]


def test_host_staged_and_dev_forms_return_identical_bytes(ctx, case):
    import torch
    n = 257
    a = _take(case, n)
    host = ctx.identity_verify_batch_p384(**a)
    tok = ctx.arena_stage(case.arena)
    staged = ctx.identity_verify_batch_p384(**dict(a, arena=None, stage_token=tok))
    b, out, keep = _dev_batch(torch, a, n, len(PREFIX_LENS))
    ctx.identity_verify_batch_p384_dev(b, out["mid"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    dev = _dev_results(torch, out, n)
    for x, y, z in zip(host, staged, dev):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert np.array_equal(host[1], case.status)
    # a token that names no upload: what the P-256 entry answers
    with pytest.raises(fabgpu.FabgpuError):
        ctx.identity_verify_batch_p384(**dict(a, arena=None, stage_token=tok + 1000))


def test_keyed_entry_returns_what_the_fresh_entry_returns(ctx, case):
    ids = [ctx.p384_key_register(ref.b48(q[0]), ref.b48(q[1])) for _, q in case.keys]
    sel = [i for i, r in enumerate(case.rows) if r["kind"] != "offcurve"]
    n = len(sel)
    assert n > 192
    col = lambda v, w: np.ascontiguousarray(v.reshape(-1, w)[sel]).reshape(-1)
    a = dict(arena=case.arena, off=col(case.off, 2), r=col(case.r, 48), s=col(case.s, 48), pre_off=case.pre_off, pre_idx=case.pre_idx[sel], spans=True, want_digests=True)
    fresh = ctx.identity_verify_batch_p384(qx=col(case.qx, 48), qy=col(case.qy, 48), **a)
    before = ctx.p384_key_table_stats()["keyed_launches"]
    keyed = ctx.identity_verify_batch_p384(key_id=np.array([ids[case.rows[i]["k"]] for i in sel], dtype=np.uint32), **a)
    assert ctx.p384_key_table_stats()["keyed_launches"] == before + 1
    for x, y in zip(fresh, keyed):
        assert np.array_equal(x, y)
    assert np.array_equal(fresh[1], case.status[sel])


def test_consecutive_offsets_without_spans(ctx, case):
    """the n + 1 offsets form: consecutive messages behind consecutive prefixes"""
    rnd = random.Random(7)
    pre = [rnd.randbytes(n) for n in (64, 129, 0)]
    msgs = [rnd.randbytes(SUFFIX_LENS[i % 8] + (i % 5)) for i in range(65)]
    arena = b"".join(pre) + b"".join(msgs)
    pre_off = np.cumsum([0] + [len(p) for p in pre]).astype(np.uint32)
    off = (np.cumsum([0] + [len(m) for m in msgs]) + int(pre_off[-1])).astype(np.uint32)
    pre_idx = np.array([i % 4 if i % 4 < 3 else NONE for i in range(65)], dtype=np.uint32)
    one = np.frombuffer(ref.b48(1) * 65, dtype=np.uint8)
    gx, gy = np.frombuffer(ref.b48(ref.GX) * 65, dtype=np.uint8), np.frombuffer(ref.b48(ref.GY) * 65, dtype=np.uint8)
    ok, st, dig = ctx.identity_verify_batch_p384(np.frombuffer(arena, dtype=np.uint8), off, one, one, qx=gx, qy=gy, pre_off=pre_off, pre_idx=pre_idx, want_digests=True)
    want = [hashlib.sha256((pre[i % 4] if i % 4 < 3 else b"") + msgs[i]).digest() for i in range(65)]
    assert [bytes(d) for d in dig] == want and not ok.any()


def test_arena_end_and_tail(ctx, case):
    """one row ends at the arena's last byte (the fixture's last row), one row lies in the tail; host, staged and _dev forms"""
    import torch
    n = 257
    a = _take(case, n)
    assert case.rows[-1]["end"] == case.arena.size
    # row 1 moves into the tail: the same message bytes, addressed at tail_base + 3
    r1 = case.rows[1]
    assert r1["p"] is not None                            # (its prefix stays in the arena)
    suffix = bytes(case.arena[r1["start"]:r1["end"]])
    tail = np.frombuffer(b"\xAA\xBB\xCC" + suffix, dtype=np.uint8).copy()
    tail_base = (case.arena.size + 63) // 64 * 64 + 64
    off = a["off"].copy()
    off[2], off[3] = tail_base + 3, tail_base + 3 + len(suffix)
    at = dict(a, off=off, tail=tail, tail_base=tail_base)
    host = ctx.identity_verify_batch_p384(**at)
    assert np.array_equal(host[1], case.status) and np.array_equal(host[2], case.digests)
    tok = ctx.arena_stage(case.arena)
    staged = ctx.identity_verify_batch_p384(**dict(at, arena=None, stage_token=tok))
    # ... and the staged upload was only read: a second batch over it without the tail still answers the reference
    again = ctx.identity_verify_batch_p384(**dict(a, arena=None, stage_token=tok))
    assert np.array_equal(again[1], case.status) and np.array_equal(again[2], case.digests)
    pad = np.zeros((-tail.size) % 4, dtype=np.uint8)
    b, out, keep = _dev_batch(torch, dict(a, off=off), n, len(PREFIX_LENS), tail=np.concatenate([tail, pad]), tail_base=tail_base)
    b.tail_len = tail.size
    ctx.identity_verify_batch_p384_dev(b, out["mid"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    dev = _dev_results(torch, out, n)
    for x, y, z in zip(host, staged, dev):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    # defects: a span that straddles tail_base, a span that leaves the tail, a tail_base that is no multiple of 64, the SHA3 flag
    for bad_off in ([tail_base - 4, tail_base + 4], [tail_base + 2, tail_base + tail.size + 1]):
        o = off.copy()
        o[2], o[3] = bad_off
        with pytest.raises(fabgpu.FabgpuError, match="invalid"):
            ctx.identity_verify_batch_p384(**dict(at, off=o))
    with pytest.raises(fabgpu.FabgpuError, match="invalid"):
        ctx.identity_verify_batch_p384(**dict(at, tail_base=tail_base + 8))
    with pytest.raises(fabgpu.FabgpuError, match="invalid"):
        ctx.identity_verify_batch_p384(**dict(a, flags=fabgpu.IDB_SHA3_256))
    b2, out2, keep2 = _dev_batch(torch, a, n, len(PREFIX_LENS))
    b2.flags |= fabgpu.IDB_SHA3_256
    with pytest.raises(fabgpu.FabgpuError, match="invalid"):
        ctx.identity_verify_batch_p384_dev(b2, out2["mid"].data_ptr(), torch.cuda.current_stream().cuda_stream)


def test_offsets_at_and_above_2_31(ctx):
    """a device arena of 2^31 + 4096 bytes of which only the last pages are written: four messages that begin below 2^31 and end at or
    above it (one behind a prefix that itself straddles 2^31 - 4096 .. ), digests against hashlib"""
    import torch
    size = (1 << 31) + 4096
    arena = torch.empty(size, dtype=torch.uint8, device="cuda")
    rnd = random.Random(31)
    lo = (1 << 31) - 4096
    page = np.frombuffer(rnd.randbytes(8192), dtype=np.uint8).copy()
    arena[lo:] = torch.from_numpy(page).cuda()
    B = 1 << 31
    spans = [(B - 100, B + 37), (B - 1, B), (B - 64, B + 64), (B - 3001, B + 4096)]        # the last one ends at the arena's last byte
    pre = [(B - 4000, B - 4000 + 129)]
    pre_idx = [NONE, 0, NONE, 0]
    n = 4
    msg = lambda s: bytes(page[s[0] - lo:s[1] - lo])
    want = [hashlib.sha256((msg(pre[0]) if pre_idx[i] == 0 else b"") + msg(spans[i])).digest() for i in range(n)]
    one = np.frombuffer(ref.b48(1) * n, dtype=np.uint8)
    a = dict(off=np.array(spans, dtype=np.uint32).reshape(-1), r=one, s=one, qx=np.frombuffer(ref.b48(ref.GX) * n, dtype=np.uint8),
             qy=np.frombuffer(ref.b48(ref.GY) * n, dtype=np.uint8), pre_off=np.array(pre, dtype=np.uint32).reshape(-1), pre_idx=np.array(pre_idx, dtype=np.uint32),
             arena=np.zeros(4, dtype=np.uint8))
    b, out, keep = _dev_batch(torch, a, n, 1)
    b.arena, b.arena_bytes = arena.data_ptr(), size
    ctx.identity_verify_batch_p384_dev(b, out["mid"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    ok, st, dig = _dev_results(torch, out, n)
    assert [bytes(d) for d in dig] == want
    assert not ok.any() and (st == 1).all()                  # (r = s = 1 under the generator: an arithmetic reject, never a fault)
