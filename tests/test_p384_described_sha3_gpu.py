"""fabgpu_identity_verify_batch_p384_sha3 (and _dev) on the GPU: the described batch of an MSP of the SHA3 hash family -
Keccak mid-states of shared prefixes, the prefix's remainder, spans at every alignment, the tail, the ends of the arena and of the tail,
both offset forms, fresh and keyed - against hashlib.sha3_256 for the digests and p384_ref for verdicts and statuses.

The reference is computed once (module fixture): every prefix length (and "no prefix") with every span length, 72 messages signed over
their SHA3-256 digest by two keys with p384_ref.sign; 130 rows are laid over them, every row with a span of its own in the arena.  The
lengths are the smallest at which the kernel can go wrong: around one and two 136-byte rate blocks (at 135 the pad's 0x06 and 0x80 share
a byte), prefixes with no whole block, exactly one, one and a remainder, two, two and a remainder."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import fabgpu
import p384_ref as ref

pytestmark = pytest.mark.gpu

SPAN_LENS = [0, 1, 134, 135, 136, 137, 271, 272, 273]
PREFIX_LENS = [0, 1, 135, 136, 137, 272, 300]
NONE = 0xFFFFFFFF
N_ROWS = 130
SIZES = [1, 63, 64, 65, 130]
KINDS = {5: "msgbit", 9: "sha2_signed", 13: "high_s", 17: "range", 21: "offcurve", 26: "prebit"}


@pytest.fixture(scope="module")
def ctx():
    c = fabgpu.Context(device=0)
    yield c
    c.close()


class Case:
    pass


def _sign(rnd, d, digest):
    while True:
        rs = ref.sign(d, ref.hash_to_int(digest), rnd.randrange(1, ref.N))
        if rs:
            return rs[0], ref.low_s(rs[1])


@pytest.fixture(scope="module")
def case():
    rnd = random.Random(33384)
    keys = []
    for _ in range(2):
        d = rnd.randrange(1, ref.N)
        keys.append((d, ref.mul(d, ref.G)))
    prefixes = [rnd.randbytes(n) for n in PREFIX_LENS]
    combos = [(p, sl) for sl in SPAN_LENS for p in list(range(len(PREFIX_LENS))) + [None]]           # 72: every prefix with every span length
    signed = []                                                                                       # per combo: (key index, span bytes, r, s)
    for ci, (p, sl) in enumerate(combos):
        span = rnd.randbytes(sl)
        msg = (prefixes[p] if p is not None else b"") + span
        signed.append((ci % 2, span) + _sign(rnd, keys[ci % 2][0], hashlib.sha3_256(msg).digest()))
    c = Case()
    arena = bytearray()
    pre_off = []
    for j, pbytes in enumerate(prefixes):                    # prefix j starts at alignment j mod 4
        arena += rnd.randbytes((j - len(arena)) % 4)
        pre_off += [len(arena), len(arena) + len(pbytes)]
        arena += pbytes
    rows = []
    for i in range(N_ROWS):
        ci = (i * 7) % len(combos)                           # (7 and 72 are coprime: the first 72 rows meet every combination)
        p, sl = combos[ci]
        k, span, r, s = signed[ci]
        q = keys[k][1]
        arena += rnd.randbytes((i // 3 - len(arena)) % 4)    # alignments 0..3, out of step with the lengths
        start = len(arena)
        arena += span
        pre = prefixes[p] if p is not None else b""
        msg = pre + span
        kind = KINDS.get(i, "valid")
        if kind == "msgbit":                                 # the arena holds one bit more than was signed: the one invalid signature
            assert sl > 0
            arena[start + sl - 1] ^= 0x10
            msg = pre + bytes(arena[start:start + sl])
        if kind == "sha2_signed":                            # a signature over the SHA-256 digest: valid under SHA-256, invalid under SHA3-256
            r, s = _sign(rnd, keys[k][0], hashlib.sha256(msg).digest())
        if kind == "prebit":                                 # signed over a prefix with one bit flipped
            assert p is not None and len(pre) > 136
            r, s = _sign(rnd, keys[k][0], hashlib.sha3_256(pre[:140] + bytes([pre[140] ^ 1]) + pre[141:] + span).digest())
        if kind == "high_s":
            s = ref.N - s
        if kind == "range":
            r = ref.N + 5
        if kind == "offcurve":
            q = (q[0], (q[1] + 1) % ref.P)
        rows.append(dict(p=p, start=start, end=start + sl, k=k, q=q, r=r, s=s, msg=msg, kind=kind))
    # the last row's span ends at the arena's last byte, and the arena's size is a multiple of 4 (the _dev form's condition)
    last = rows[-1]
    span = bytes(arena[last["start"]:last["end"]])
    assert len(span) > 0
    del arena[last["start"]:]
    arena += rnd.randbytes((-(len(arena) + len(span))) % 4) + span
    last["start"], last["end"] = len(arena) - len(span), len(arena)
    assert len(arena) % 4 == 0
    col = lambda f: np.frombuffer(b"".join(ref.b48(f(r_)) for r_ in rows), dtype=np.uint8).copy()
    c.arena = np.frombuffer(bytes(arena), dtype=np.uint8).copy()
    c.pre_off = np.array(pre_off, dtype=np.uint32)
    c.off = np.array([[r_["start"], r_["end"]] for r_ in rows], dtype=np.uint32).reshape(-1)
    c.pre_idx = np.array([NONE if r_["p"] is None else r_["p"] for r_ in rows], dtype=np.uint32)
    c.qx, c.qy, c.r, c.s = col(lambda r_: r_["q"][0]), col(lambda r_: r_["q"][1]), col(lambda r_: r_["r"]), col(lambda r_: r_["s"])
    c.digests = np.frombuffer(b"".join(hashlib.sha3_256(r_["msg"]).digest() for r_ in rows), dtype=np.uint8).reshape(-1, 32).copy()
    memo = {}

    def status(r_, digest):
        key = (r_["q"], digest, r_["r"], r_["s"])
        if key not in memo:
            memo[key] = ref.status(r_["q"][0], r_["q"][1], ref.hash_to_int(digest), r_["r"], r_["s"])
        return memo[key]
    c.status = np.array([status(r_, hashlib.sha3_256(r_["msg"]).digest()) for r_ in rows], dtype=np.uint8)
    # under SHA-256: the first 32 rows against the host reference under SHA-256
    c.n2 = 32
    c.digests2 = np.frombuffer(b"".join(hashlib.sha256(r_["msg"]).digest() for r_ in rows[:c.n2]), dtype=np.uint8).reshape(-1, 32).copy()
    c.status2 = np.array([status(r_, hashlib.sha256(r_["msg"]).digest()) for r_ in rows[:c.n2]], dtype=np.uint8)
    c.rows, c.keys, c.prefixes, c.combos = rows, keys, prefixes, combos
    return c


def _take(c, n, **kw):
    return dict(dict(arena=c.arena, off=c.off[:2 * n], r=c.r[:48 * n], s=c.s[:48 * n], qx=c.qx[:48 * n], qy=c.qy[:48 * n], pre_off=c.pre_off,
                     pre_idx=c.pre_idx[:n], spans=True, want_digests=True, sha3=True), **kw)


def test_the_case_covers_what_it_must(case):
    rows = case.rows
    assert {(r["p"], r["end"] - r["start"]) for r in rows[:72]} == set(case.combos)
    assert {r["start"] % 4 for r in rows} == {0, 1, 2, 3} and {int(o) % 4 for o in case.pre_off[0::2]} == {0, 1, 2, 3}
    # every alignment meets a span that crosses a block and a prefix with a remainder
    assert {r["start"] % 4 for r in rows if r["p"] is not None and PREFIX_LENS[r["p"]] % 136 and r["end"] - r["start"] >= 134} == {0, 1, 2, 3}
    # the prefix's remainder and the span together cross a block boundary, end exactly on one, and end one byte short of one (0x86)
    rem = lambda r: (PREFIX_LENS[r["p"]] % 136 if r["p"] is not None else 0) + r["end"] - r["start"]
    assert any(r["p"] is not None and 0 < PREFIX_LENS[r["p"]] % 136 < 136 < rem(r) for r in rows)
    assert {len(r["msg"]) % 136 for r in rows} >= {0, 1, 134, 135}
    assert set(case.status.tolist()) == {0, 1, 2, 3, 4}
    assert [int(case.status[i]) for i in (5, 9, 13, 17, 21, 26)] == [1, 1, 2, 3, 4, 1]
    assert case.status2[9] == 0 and case.status2[5] == 1 and (case.status2[[0, 1, 2, 3]] == 1).all()
    assert rows[-1]["end"] == case.arena.size


@pytest.mark.parametrize("n", SIZES)
def test_verdicts_statuses_and_digests_equal_the_reference(ctx, case, n):
    ok, st, dig = ctx.identity_verify_batch_p384(**_take(case, n))
    bad = [i for i in range(n) if bytes(dig[i]) != bytes(case.digests[i])]
    assert not bad, [(i, case.rows[i]["p"], case.rows[i]["end"] - case.rows[i]["start"]) for i in bad[:8]]
    assert np.array_equal(st, case.status[:n])
    assert np.array_equal(ok, case.status[:n] == 0)


def test_the_sha256_entry_answers_the_sha256_reference_for_the_same_description(ctx, case):
    """the same description through fabgpu_identity_verify_batch_p384: SHA-256 digests, the SHA3 signatures invalid, the SHA-256 one valid"""
    n = case.n2
    ok, st, dig = ctx.identity_verify_batch_p384(**_take(case, n, sha3=False))
    assert np.array_equal(dig, case.digests2) and np.array_equal(st, case.status2) and np.array_equal(ok, case.status2 == 0)
    ok3, st3, _ = ctx.identity_verify_batch_p384(**_take(case, n))
    assert ok[9] and not ok3[9] and st3[9] == 1              # the signature over SHA-256: valid under SHA-256, invalid under SHA3-256
    assert ok3[0] and not ok[0] and st[0] == 1               # ... and the reverse for one over SHA3-256


def _dev_batch(torch, a, n, n_prefixes, tail=None, tail_base=0, key_id=None):
    """the _dev form's descriptor over torch tensors, canary bytes behind row n of every output -> (descriptor, out tensors, kept alive)"""
    names = ("arena", "off", "r", "s", "pre_off", "pre_idx") + (() if key_id is not None else ("qx", "qy"))
    t = {k: torch.from_numpy(np.array(a[k]).view(np.uint8)).cuda() for k in names}
    words = (n + 63) // 64
    out = dict(bits=torch.full((words + 1,), -1, dtype=torch.int64, device="cuda"), st=torch.full((n + 8,), 0xEE, dtype=torch.uint8, device="cuda"),
               dig=torch.full((n + 2, 32), 0xEE, dtype=torch.uint8, device="cuda"),
               mid=torch.full((max(1, n_prefixes) * 200 + 64,), 0xEE, dtype=torch.uint8, device="cuda"))
    b = fabgpu._IdBatchP384()
    b.n, b.flags = n, fabgpu.IDB_SPANS
    b.arena, b.arena_bytes = t["arena"].data_ptr(), t["arena"].numel()
    b.off, b.r, b.s = (t[k].data_ptr() for k in ("off", "r", "s"))
    if key_id is not None:
        t["key_id"] = torch.from_numpy(np.array(key_id, dtype=np.uint32).view(np.uint8)).cuda()
        b.key_id = t["key_id"].data_ptr()
    else:
        b.qx, b.qy = t["qx"].data_ptr(), t["qy"].data_ptr()
    if n_prefixes:
        b.n_prefixes, b.pre_off, b.pre_idx = n_prefixes, t["pre_off"].data_ptr(), t["pre_idx"].data_ptr()
    if tail is not None:
        t["tail"] = torch.from_numpy(tail).cuda()
        b.tail, b.tail_base, b.tail_len = t["tail"].data_ptr(), tail_base, tail.size
    b.verdict_bits, b.status, b.digests = out["bits"].data_ptr(), out["st"].data_ptr(), out["dig"].data_ptr()
    return b, out, t


def _dev_results(torch, out, n, n_prefixes):
    torch.cuda.synchronize()
    words = (n + 63) // 64
    bits = out["bits"].cpu().numpy().view(np.uint64)
    st, dig, mid = out["st"].cpu().numpy(), out["dig"].cpu().numpy(), out["mid"].cpu().numpy()
    # rows at or above n are never written, and no mid-state reaches behind its n_prefixes x 200 bytes
    assert bits[words] == 0xFFFFFFFFFFFFFFFF and (st[n:] == 0xEE).all() and (dig[n:] == 0xEE).all() and (mid[n_prefixes * 200:] == 0xEE).all()
    return fabgpu.unpack_bits(bits[:words].copy(), n), st[:n], dig[:n]


@pytest.mark.parametrize("n", SIZES)
def test_dev_form_writes_no_row_at_or_above_n(ctx, case, n):
    import torch
    b, out, keep = _dev_batch(torch, _take(case, n), n, len(PREFIX_LENS))
    ctx.identity_verify_batch_p384_sha3_dev(b, out["mid"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    ok, st, dig = _dev_results(torch, out, n, len(PREFIX_LENS))
    assert np.array_equal(dig, case.digests[:n]) and np.array_equal(st, case.status[:n]) and np.array_equal(ok, case.status[:n] == 0)


def test_host_staged_and_dev_forms_return_identical_bytes(ctx, case):
    import torch
    n = N_ROWS
    a = _take(case, n)
    host = ctx.identity_verify_batch_p384(**a)
    tok = ctx.arena_stage(case.arena)
    staged = ctx.identity_verify_batch_p384(**dict(a, arena=None, stage_token=tok))
    # the same staged upload serves a SHA-256 batch and a SHA3-256 batch, as the pass's two batches over one block do
    sha2 = ctx.identity_verify_batch_p384(**dict(_take(case, case.n2, sha3=False), arena=None, stage_token=tok))
    assert np.array_equal(sha2[1], case.status2) and np.array_equal(sha2[2], case.digests2)
    b, out, keep = _dev_batch(torch, a, n, len(PREFIX_LENS))
    ctx.identity_verify_batch_p384_sha3_dev(b, out["mid"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    dev = _dev_results(torch, out, n, len(PREFIX_LENS))
    for x, y, z in zip(host, staged, dev):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert np.array_equal(host[1], case.status) and np.array_equal(host[2], case.digests)
    # the verdict words and statuses are fabgpu_p384_verify_batch's over (key, the SHA3-256 digest as e, r, s)
    e48 = np.zeros((n, 48), dtype=np.uint8)
    e48[:, 16:] = case.digests
    ok_d, st_d = ctx.p384_verify_batch(case.qx, case.qy, e48.reshape(-1), case.r, case.s)
    assert np.array_equal(ok_d, host[0]) and np.array_equal(st_d, host[1])
    # a mid scratch that is not 8-byte aligned is refused before anything is launched
    with pytest.raises(fabgpu.FabgpuError, match="invalid"):
        ctx.identity_verify_batch_p384_sha3_dev(b, out["mid"].data_ptr() + 4, torch.cuda.current_stream().cuda_stream)


def test_keyed_entry_returns_what_the_fresh_entry_returns(ctx, case):
    import torch
    ids = [ctx.p384_key_register(ref.b48(q[0]), ref.b48(q[1])) for _, q in case.keys]
    sel = [i for i, r in enumerate(case.rows) if r["kind"] != "offcurve"]
    n = len(sel)
    col = lambda v, w: np.ascontiguousarray(v.reshape(-1, w)[sel]).reshape(-1)
    a = dict(arena=case.arena, off=col(case.off, 2), r=col(case.r, 48), s=col(case.s, 48), pre_off=case.pre_off, pre_idx=case.pre_idx[sel], spans=True,
             want_digests=True, sha3=True)
    key_id = np.array([ids[case.rows[i]["k"]] for i in sel], dtype=np.uint32)
    fresh = ctx.identity_verify_batch_p384(qx=col(case.qx, 48), qy=col(case.qy, 48), **a)
    before = ctx.p384_key_table_stats()["keyed_launches"]
    keyed = ctx.identity_verify_batch_p384(key_id=key_id, **a)
    assert ctx.p384_key_table_stats()["keyed_launches"] == before + 1
    for x, y in zip(fresh, keyed):
        assert np.array_equal(x, y)
    assert np.array_equal(fresh[1], case.status[sel]) and np.array_equal(fresh[2], case.digests[sel])
    b, out, keep = _dev_batch(torch, a, n, len(PREFIX_LENS), key_id=key_id)
    ctx.identity_verify_batch_p384_sha3_dev(b, out["mid"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    for x, y in zip(keyed, _dev_results(torch, out, n, len(PREFIX_LENS))):
        assert np.array_equal(x, y)


def test_consecutive_offsets_without_spans(ctx):
    """the n + 1 offsets form: consecutive messages behind consecutive prefixes, with and without prefixes"""
    rnd = random.Random(7)
    pre = [rnd.randbytes(n) for n in (136, 273, 0, 135)]
    msgs = [rnd.randbytes(SPAN_LENS[i % 9] + (i % 5)) for i in range(65)]
    arena = b"".join(pre) + b"".join(msgs)
    pre_off = np.cumsum([0] + [len(p) for p in pre]).astype(np.uint32)
    off = (np.cumsum([0] + [len(m) for m in msgs]) + int(pre_off[-1])).astype(np.uint32)
    pre_idx = np.array([i % 5 if i % 5 < 4 else NONE for i in range(65)], dtype=np.uint32)
    one = np.frombuffer(ref.b48(1) * 65, dtype=np.uint8)
    gx, gy = np.frombuffer(ref.b48(ref.GX) * 65, dtype=np.uint8), np.frombuffer(ref.b48(ref.GY) * 65, dtype=np.uint8)
    a = np.frombuffer(arena, dtype=np.uint8)
    ok, st, dig = ctx.identity_verify_batch_p384(a, off, one, one, qx=gx, qy=gy, pre_off=pre_off, pre_idx=pre_idx, want_digests=True, sha3=True)
    want = [hashlib.sha3_256((pre[i % 5] if i % 5 < 4 else b"") + msgs[i]).digest() for i in range(65)]
    assert [bytes(d) for d in dig] == want and not ok.any() and (st == 1).all()
    ok, st, dig = ctx.identity_verify_batch_p384(a, off, one, one, qx=gx, qy=gy, want_digests=True, sha3=True)
    assert [bytes(d) for d in dig] == [hashlib.sha3_256(m).digest() for m in msgs] and not ok.any()


def test_tail_and_the_ends_of_arena_and_tail(ctx, case):
    """four rows move into the tail at alignments 0..3 - the last of them ends at the tail's last byte, the tail's length no multiple of
    4 - while their prefixes stay in the arena; the fixture's last row ends at the arena's last byte; host, staged and _dev forms"""
    import torch
    n = N_ROWS
    a = _take(case, n)
    moved = [i for i in range(n) if case.rows[i]["kind"] == "valid" and case.rows[i]["p"] is not None and PREFIX_LENS[case.rows[i]["p"]] % 136
             and case.rows[i]["end"] - case.rows[i]["start"] >= 135][:4]
    assert len(moved) == 4
    tail_base = (case.arena.size + 63) // 64 * 64 + 64
    tail = bytearray()
    off = a["off"].copy()
    for j, i in enumerate(moved):
        span = bytes(case.arena[case.rows[i]["start"]:case.rows[i]["end"]])
        tail += b"\xAA" * ((j + 1 - len(tail)) % 4)          # alignments 1, 2, 3, 0
        off[2 * i], off[2 * i + 1] = tail_base + len(tail), tail_base + len(tail) + len(span)
        tail += span
    if len(tail) % 4 == 0:                                   # (keep the last span at the very end of a tail that ends inside a dword)
        tail = bytearray(b"\xAA") + tail
        for i in moved:
            off[2 * i] += 1
            off[2 * i + 1] += 1
    assert len(tail) % 4 != 0 and off[2 * moved[-1] + 1] == tail_base + len(tail)
    tail = np.frombuffer(bytes(tail), dtype=np.uint8).copy()
    at = dict(a, off=off, tail=tail, tail_base=tail_base)
    host = ctx.identity_verify_batch_p384(**at)
    assert np.array_equal(host[2], case.digests) and np.array_equal(host[1], case.status)
    tok = ctx.arena_stage(case.arena)
    staged = ctx.identity_verify_batch_p384(**dict(at, arena=None, stage_token=tok))
    pad = np.zeros((-tail.size) % 4, dtype=np.uint8)
    b, out, keep = _dev_batch(torch, dict(a, off=off), n, len(PREFIX_LENS), tail=np.concatenate([tail, pad]), tail_base=tail_base)
    b.tail_len = tail.size
    ctx.identity_verify_batch_p384_sha3_dev(b, out["mid"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    dev = _dev_results(torch, out, n, len(PREFIX_LENS))
    for x, y, z in zip(host, staged, dev):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    # malformed descriptions answer as they do at the SHA-256 entry
    for bad_off in ([tail_base - 4, tail_base + 4], [tail_base + 2, tail_base + tail.size + 1], [200, 100]):
        o = off.copy()
        o[2], o[3] = bad_off
        with pytest.raises(fabgpu.FabgpuError, match="invalid"):
            ctx.identity_verify_batch_p384(**dict(at, off=o))
    with pytest.raises(fabgpu.FabgpuError, match="invalid"):
        ctx.identity_verify_batch_p384(**dict(at, tail_base=tail_base + 8))
    for flag in (8, fabgpu.IDB_SHA3_256):                   # a flag nobody defined; the family is the entry's, not a flag's
        with pytest.raises(fabgpu.FabgpuError, match="invalid"):
            ctx.identity_verify_batch_p384(**dict(a, flags=flag))


def test_a_reversed_span_hashes_as_empty_in_the_dev_form(ctx, case):
    """the _dev form cannot see the offsets: a reversed span is the empty message behind its prefix, and nothing outside is read"""
    import torch
    n = 4
    a = _take(case, n)
    off = a["off"].copy()
    p = case.rows[2]["p"]
    assert p is not None and PREFIX_LENS[p] % 136 and case.rows[2]["end"] > case.rows[2]["start"]
    off[4], off[5] = off[5] + 5, off[4]
    b, out, keep = _dev_batch(torch, dict(a, off=off), n, len(PREFIX_LENS))
    ctx.identity_verify_batch_p384_sha3_dev(b, out["mid"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    ok, st, dig = _dev_results(torch, out, n, len(PREFIX_LENS))
    assert bytes(dig[2]) == hashlib.sha3_256(case.prefixes[p]).digest()
    assert np.array_equal(dig[[0, 1, 3]], case.digests[[0, 1, 3]])


def test_the_warm_call_launches_nothing(ctx):
    b = fabgpu._IdBatchP384()
    b.n, b.flags = 0, fabgpu.IDB_SPANS
    before = ctx.p384_key_table_stats()["keyed_launches"]
    assert ctx._L.fabgpu_identity_verify_batch_p384_sha3(ctx._h, ctypes.byref(b)) == 0
    assert ctx.p384_key_table_stats()["keyed_launches"] == before
