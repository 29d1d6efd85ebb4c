"""The three host-pointer entries of a DESCRIBED batch - fabgpu_identity_verify_batch, fabgpu_identity_verify_batch_p384 and
fabgpu_identity_verify_batch_p384_sha3 - called raw through ctypes at n = 3: they share one span plan (csrc/described_plan.h) and one
staging path, so a malformed description gets FABGPU_EINVAL from each with the caller's arrays untouched and the context fit for the
next call, and a failed allocation (FABGPU_FAULT_INJECT=oom, simulated on the host) gets FABGPU_ENOMEM likewise.  The reference is
hashlib plus the oracles of test_gpu_parity.py (coracle) and p384_ref.py, computed once."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import coracle
import fabgpu
import bccsp_sw_oracle as po
import p384_ref as ref
from idemix_common import be32, fixtures, make_batch as make_nym_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["p256", "p384", "p384_sha3"]
N = 3
NONE = 0xFFFFFFFF
SENTINEL_WORD, SENTINEL_BYTE = 0xA5A5A5A5A5A5A5A5, 0xEE
TAIL_BASE = 1024
OFF = [200, 245, TAIL_BASE + 3, TAIL_BASE + 100, 7, 7]           # (start, end) of the three rows


class Case:
    """Three messages: row 0 = prefix 0 (70 bytes) || span, row 1 = a span of the tail alone, row 2 = an empty message; row 0's
    signature is valid, the others' are row 0's (status 1)."""


def make_case(entry):
    rnd = random.Random(3 + ENTRIES.index(entry))
    c = Case()
    c.entry = entry
    c.arena = np.frombuffer(rnd.randbytes(400), dtype=np.uint8).copy()
    c.tail = np.frombuffer(rnd.randbytes(100), dtype=np.uint8).copy()
    c.pre_off = np.array([16, 86], dtype=np.uint32)
    c.pre_idx = np.array([0, NONE, NONE], dtype=np.uint32)
    c.off = np.array(OFF, dtype=np.uint32)
    msgs = [bytes(c.arena[16:86]) + bytes(c.arena[200:245]), bytes(c.tail[3:100]), b""]
    h = hashlib.sha3_256 if entry == "p384_sha3" else hashlib.sha256
    c.digests = np.frombuffer(b"".join(h(m).digest() for m in msgs), dtype=np.uint8).reshape(N, 32).copy()
    if entry == "p256":
        b = fabgpu.synth_batch(1, seed=5, invalid_permille=0, e_in=c.digests[:1])
        c.qx, c.qy, c.r, c.s = (np.tile(b[k].reshape(1, 32), (N, 1)).copy() for k in ("qx", "qy", "r", "s"))
        c.status = coracle.verify_batch(c.qx, c.qy, c.digests, c.r, c.s)
    else:
        d = rnd.randrange(1, ref.N)
        q = ref.mul(d, ref.G)
        r, s = ref.sign(d, ref.hash_to_int(bytes(c.digests[0])), rnd.randrange(1, ref.N))
        s = ref.low_s(s)
        c.qx, c.qy, c.r, c.s = (np.frombuffer(ref.b48(v) * N, dtype=np.uint8).reshape(N, 48).copy() for v in (q[0], q[1], r, s))
        c.status = np.array([ref.status(q[0], q[1], ref.hash_to_int(bytes(dg)), r, s) for dg in c.digests], dtype=np.uint8)
    assert c.status.tolist() == [0, 1, 1]
    return c


_CASES = {}


def case_of(entry):
    if entry not in _CASES:
        _CASES[entry] = make_case(entry)
    return _CASES[entry]


def call(L, h, c, **change):
    """One raw call over the case with sentinel-filled results -> (rc, verdict words, statuses, digests[, gathered digests]).
    change: off, pre_off, tail_base, tail_len, spans, gather (6 u32), arena, nym ((spans k x 2, issuer ids, six columns): P-256 only;
    then the pseudonym verdict words and statuses come last)."""
    b = fabgpu._IdBatch() if c.entry == "p256" else fabgpu._IdBatchP384()
    off = np.ascontiguousarray(change.get("off", c.off), dtype=np.uint32)
    pre_off = np.ascontiguousarray(change.get("pre_off", c.pre_off), dtype=np.uint32)
    gather = np.ascontiguousarray(change["gather"], dtype=np.uint32) if "gather" in change else None
    bits = np.full(1, SENTINEL_WORD, dtype=np.uint64)
    st = np.full(N, SENTINEL_BYTE, dtype=np.uint8)
    dig = np.full((N, 32), SENTINEL_BYTE, dtype=np.uint8)
    gdig = np.full((1, 32), SENTINEL_BYTE, dtype=np.uint8)
    b.n, b.flags = N, fabgpu.IDB_SPANS if change.get("spans", True) else 0
    arena = change.get("arena", c.arena)
    b.arena, b.off, b.n_prefixes, b.pre_off, b.pre_idx = arena.ctypes.data, off.ctypes.data, 1, pre_off.ctypes.data, c.pre_idx.ctypes.data
    b.qx, b.qy, b.r, b.s = c.qx.ctypes.data, c.qy.ctypes.data, c.r.ctypes.data, c.s.ctypes.data
    b.tail, b.tail_base, b.tail_len = c.tail.ctypes.data, change.get("tail_base", TAIL_BASE), change.get("tail_len", c.tail.size)
    b.verdict_bits, b.status, b.digests = bits.ctypes.data, st.ctypes.data, dig.ctypes.data
    if gather is not None:
        b.n_gather, b.gather_spans, b.gather_digests = 1, gather.ctypes.data, gdig.ctypes.data
    nres = ()
    if "nym" in change:
        nsp, niss = (np.ascontiguousarray(x, dtype=np.uint32) for x in change["nym"][:2])
        nf = np.ascontiguousarray(np.concatenate([x.reshape(-1, 32) for x in change["nym"][2]], axis=0))
        nres = (np.full(1, SENTINEL_WORD, dtype=np.uint64), np.full(niss.size, SENTINEL_BYTE, dtype=np.uint8))
        b.n_nym, b.nym_off, b.nym_issuer, b.nym_fields = niss.size, nsp.ctypes.data, niss.ctypes.data, nf.ctypes.data
        b.nym_verdict_bits, b.nym_status = nres[0].ctypes.data, nres[1].ctypes.data
    f = {"p256": L.fabgpu_identity_verify_batch, "p384": L.fabgpu_identity_verify_batch_p384, "p384_sha3": L.fabgpu_identity_verify_batch_p384_sha3}[c.entry]
    rc = f(h, ctypes.byref(b))
    return (rc, bits, st, dig) + ((gdig,) if gather is not None else ()) + nres


def register_issuers(ctx):
    """the two issuers of the committed idemix fixtures -> [(ipk, sk)] for make_nym_batch"""
    out = []
    for name in ("MSP1OU1", "MSP2OU1"):
        fx = fixtures()[name]
        ipk = fx["ipk"]
        ctx.idemix_issuer_register((be32(ipk.h_sk[0]), be32(ipk.h_sk[1])), (be32(ipk.h_rand[0]), be32(ipk.h_rand[1])), ipk.hash)
        out.append((ipk, fx["signer"].sk))
    return out


def untouched(res):
    return all((a == (SENTINEL_WORD if a.dtype == np.uint64 else SENTINEL_BYTE)).all() for a in res[1:])


def answers_the_reference(res, c):
    return res[0] == 0 and np.array_equal(fabgpu.unpack_bits(res[1], N), c.status == 0) and np.array_equal(res[2], c.status) and np.array_equal(res[3], c.digests)


def swap(off, row, s0, s1):
    o = np.array(off, dtype=np.uint32)
    o[2 * row], o[2 * row + 1] = s0, s1
    return o


# the refusals of the plan that reach an entry (the gathered piece: P-256 only - the P-384 entries have no gather part)
REFUSALS = {
    "reversed span": dict(off=swap(OFF, 0, 245, 200)),
    "span straddling tail_base by one byte": dict(off=swap(OFF, 0, 1000, TAIL_BASE + 1)),
    "tail span one byte past the tail's end": dict(off=swap(OFF, 1, TAIL_BASE + 3, TAIL_BASE + 101)),
    "prefix in the tail": dict(pre_off=[TAIL_BASE, TAIL_BASE + 70]),
    "tail_base not a multiple of 64": dict(tail_base=TAIL_BASE + 8, off=swap(OFF, 1, TAIL_BASE + 11, TAIL_BASE + 108)),
    "a tail without the spans flag": dict(spans=False, off=[200, 245, 245, 250], pre_off=[16, 86]),
    "consecutive offsets with a decrease": dict(spans=False, tail_len=0, off=[200, 245, 244, 250], pre_off=[16, 86]),
    "tail_base + tail_len equal to 0xFFFFFFF1": dict(tail_base=0xFFFFFFC0, tail_len=0x31, off=swap(OFF, 1, 0xFFFFFFC0, 0xFFFFFFC1)),
    "gather span reaching past tail_base": dict(gather=[1000, TAIL_BASE + 1, 0, 0, 0, 0]),
}


@pytest.fixture(scope="module")
def ctx():
    c = fabgpu.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_valid_description_answers_the_reference(ctx, entry):
    c = case_of(entry)
    assert answers_the_reference(call(fabgpu.load(), ctx.handle, c), c)
    if entry == "p256":                                    # ... and with a gathered message riding along
        res = call(fabgpu.load(), ctx.handle, c, gather=[16, 86, 0, 0, 200, 245])
        assert answers_the_reference(res, c)
        assert bytes(res[4][0]) == hashlib.sha256(bytes(c.arena[16:86]) + bytes(c.arena[200:245])).digest()


@pytest.mark.parametrize("entry,what", [(e, w) for e in ENTRIES for w in REFUSALS if e == "p256" or "gather" not in REFUSALS[w]])
def test_a_malformed_description_is_refused_and_nothing_is_written(ctx, entry, what):
    c = case_of(entry)
    res = call(fabgpu.load(), ctx.handle, c, **REFUSALS[what])
    assert res[0] == fabgpu.FABGPU_EINVAL, (entry, what, res[0])
    assert untouched(res), "%s: %s was refused and wrote to the caller's arrays" % (entry, what)
    assert answers_the_reference(call(fabgpu.load(), ctx.handle, c), c)    # the same context, straight afterwards


def oom_child():
    """Runs in a fresh process under FABGPU_FAULT_INJECT=oom (a failed allocation simulated on the host; the device is fine)."""
    L = fabgpu.load()
    ctx = fabgpu.Context(device=0)
    issuers = register_issuers(ctx)
    narena, noff, iid, cols, _ = make_nym_batch(issuers, 2, 4).arrays()
    c = case_of("p256")
    riders = dict(arena=np.concatenate([c.arena, narena]), nym=(np.stack([noff[:-1], noff[1:]], axis=1) + c.arena.size, iid, cols))
    for entry in ENTRIES:
        c = case_of(entry)
        for change in ({}, dict(gather=[16, 86, 0, 0, 200, 245]), riders, dict(riders, gather=[16, 86, 0, 0, 200, 245])) if entry == "p256" else ({},):
            res = call(L, ctx.handle, c, **change)
            assert res[0] == -3, (entry, res[0])
            assert untouched(res), "%s failed and wrote to the caller's arrays" % entry
    ctx.close()
    print("DESCRIBED_FAIL_CLEAN")


def test_the_three_entries_fail_clean_without_memory():
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import test_described_entries_gpu as t; t.oom_child()" % (
        os.path.join(ROOT, "fabric-mod_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, FABGPU_FAULT_INJECT="oom"), timeout=300)
    assert r.returncode == 0 and "DESCRIBED_FAIL_CLEAN" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- equality of forms: n = 65 (two verdict words, 63 idle lanes behind the 65th row), two prefixes - one shorter than a hash block of
# either family -, one message in the tail, one empty message: unstaged, staged (fabgpu_arena_stage) and _dev return the same bytes,
# for fresh and for registered keys; the reference is hashlib + coracle (P-256) / p384_ref (P-384), computed once per entry ------------
NE = 65
ROW_TAIL, ROW_EMPTY = 5, 8
GATHER = [3, 303, 0, 0, 310, 350]                         # one gathered message: prefix A || prefix B


class Big:
    pass


def make_big(entry):
    rnd = random.Random(65 + ENTRIES.index(entry))
    c = Big()
    c.entry = entry
    pre = [(3, 303), (310, 350)]                           # 300 bytes: whole blocks and a rest under SHA-256 and SHA3-256; 40 bytes: no whole block
    arena = bytearray(rnd.randbytes(360))
    spans = []
    for i in range(NE):
        ln = [0, 1, 55, 56, 64, 119, 136, 137][i % 8] + i % 3
        spans.append((len(arena), len(arena) + ln))
        arena += rnd.randbytes(ln + i % 2)
    arena += rnd.randbytes((-len(arena)) % 4)
    c.tail = np.frombuffer(rnd.randbytes(77), dtype=np.uint8).copy()
    c.tail_base = (len(arena) + 63) // 64 * 64 + 2048       # (room for the pseudonym messages of the riders' test below it)
    spans[ROW_TAIL] = (c.tail_base + 2, c.tail_base + 77)
    spans[ROW_EMPTY] = (9, 9)
    c.arena = np.frombuffer(bytes(arena), dtype=np.uint8).copy()
    c.off = np.array(spans, dtype=np.uint32).reshape(-1)
    c.pre_off = np.array(pre, dtype=np.uint32).reshape(-1)
    c.pre_idx = np.array([[0, 1, NONE][i % 3] for i in range(NE)], dtype=np.uint32)
    assert c.pre_idx[ROW_TAIL] == NONE and c.pre_idx[ROW_EMPTY] == NONE

    def body(i):
        s0, s1 = spans[i]
        return bytes(c.tail[s0 - c.tail_base:s1 - c.tail_base]) if s0 >= c.tail_base else bytes(c.arena[s0:s1])

    msgs = [(bytes(c.arena[slice(*pre[c.pre_idx[i]])]) if c.pre_idx[i] != NONE else b"") + body(i) for i in range(NE)]
    h = hashlib.sha3_256 if entry == "p384_sha3" else hashlib.sha256
    dg = [h(m).digest() for m in msgs]
    c.digests = np.frombuffer(b"".join(dg), dtype=np.uint8).reshape(NE, 32).copy()
    w = 32 if entry == "p256" else 48
    col = lambda v: np.frombuffer(b"".join(x.to_bytes(w, "big") for x in v), dtype=np.uint8).reshape(NE, w).copy()
    ds = [rnd.randrange(1, po.N if entry == "p256" else ref.N) for _ in range(3)]
    rs = []
    if entry == "p256":
        c.keys = [po.pt_mul(d, (po.GX, po.GY)) for d in ds]
        for i in range(NE):                                # every fourth row carries its neighbour's signature
            rs.append(po.sign_raw(ds[i % 3], dg[i], 7000 + i) if i % 4 else rs[-1] if rs else (1, 1))
    else:
        c.keys = [ref.mul(d, ref.G) for d in ds]
        for i in range(NE):                                # 22 signed rows, the others carry row i - 3's signature
            if i % 3 == 0:
                r, s = ref.sign(ds[i % 3], ref.hash_to_int(dg[i]), rnd.randrange(1, ref.N))
                rs.append((r, ref.low_s(s)))
            else:
                rs.append(rs[i - i % 3])
    c.kidx = [i % 3 for i in range(NE)]
    c.qx, c.qy = col([c.keys[k][0] for k in c.kidx]), col([c.keys[k][1] for k in c.kidx])
    c.r, c.s = col([a for a, _ in rs]), col([b for _, b in rs])
    if entry == "p256":
        c.status = np.asarray(coracle.verify_batch(c.qx, c.qy, c.digests, c.r, c.s), dtype=np.uint8)
    else:
        c.status = np.array([ref.status(c.keys[c.kidx[i]][0], c.keys[c.kidx[i]][1], ref.hash_to_int(dg[i]), *rs[i]) for i in range(NE)], dtype=np.uint8)
    assert 10 < int((c.status == 0).sum()) < NE and c.status[64] in (0, 1)
    return c


_BIG = {}


def big_of(entry):
    if entry not in _BIG:
        _BIG[entry] = make_big(entry)
    return _BIG[entry]


def host_form(ctx, c, keys, **more):
    f = ctx.identity_verify_batch if c.entry == "p256" else ctx.identity_verify_batch_p384
    if c.entry == "p384_sha3":
        more["sha3"] = True
    return f(more.pop("arena", c.arena), c.off, c.r, c.s, pre_off=c.pre_off, pre_idx=c.pre_idx, spans=True, want_digests=True, tail=c.tail,
             tail_base=c.tail_base, **keys, **more)


def dev_form(ctx, c, key_id, gather):
    """the _dev entry over torch tensors, every output with a sentinel row behind it -> the host forms' tuple"""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    p256 = c.entry == "p256"
    arena = c.arena
    if p256:                                               # a _dev caller places the tail's bytes in its device arena, at tail_base
        arena = np.zeros(c.tail_base + 80 + 64, dtype=np.uint8)
        arena[:c.arena.size] = c.arena
        arena[c.tail_base:c.tail_base + c.tail.size] = c.tail
    t = dict(arena=up(arena), off=up(c.off), pre_off=up(c.pre_off), pre_idx=up(c.pre_idx), r=up(c.r), s=up(c.s), qx=up(c.qx), qy=up(c.qy),
             tail=up(np.concatenate([c.tail, np.zeros(3, dtype=np.uint8)])))
    bits = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((NE + 8,), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    dig = torch.full((NE + 1, 32), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    mid = torch.zeros(2 * 200, dtype=torch.uint8, device="cuda")
    b = fabgpu._IdBatch() if p256 else fabgpu._IdBatchP384()
    b.n, b.flags = NE, fabgpu.IDB_SPANS
    b.arena, b.arena_bytes, b.off = t["arena"].data_ptr(), t["arena"].numel(), t["off"].data_ptr()
    b.n_prefixes, b.pre_off, b.pre_idx = 2, t["pre_off"].data_ptr(), t["pre_idx"].data_ptr()
    b.r, b.s = t["r"].data_ptr(), t["s"].data_ptr()
    if key_id is not None:
        t["key_id"] = up(key_id)
        b.key_id = t["key_id"].data_ptr()
    else:
        b.qx, b.qy = t["qx"].data_ptr(), t["qy"].data_ptr()
    if not p256:
        b.tail, b.tail_base, b.tail_len = t["tail"].data_ptr(), c.tail_base, c.tail.size
    b.verdict_bits, b.status, b.digests = bits.data_ptr(), st.data_ptr(), dig.data_ptr()
    gdig = None
    if gather is not None:
        total = sum(gather[2 * k + 1] - gather[2 * k] for k in range(3))
        t["g"], t["goff"] = up(np.array(gather, dtype=np.uint32)), up(np.array([0, total], dtype=np.uint32))
        t["gscr"] = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        gdig = torch.full((2, 32), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
        b.n_gather, b.gather_spans, b.gather_off, b.gather_digests = 1, t["g"].data_ptr(), t["goff"].data_ptr(), gdig.data_ptr()
        b.gather_scratch, b.gather_scratch_bytes = t["gscr"].data_ptr(), total + 64
    f = {"p256": ctx.identity_verify_batch_dev, "p384": ctx.identity_verify_batch_p384_dev, "p384_sha3": ctx.identity_verify_batch_p384_sha3_dev}[c.entry]
    f(b, mid.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    w = bits.cpu().numpy().view(np.uint64)
    st, dig = st.cpu().numpy(), dig.cpu().numpy()
    assert w[2] == 0xFFFFFFFFFFFFFFFF and (st[NE:] == SENTINEL_BYTE).all() and (dig[NE:] == SENTINEL_BYTE).all()      # nothing at or above n
    out = (fabgpu.unpack_bits(w[:2].copy(), NE), st[:NE])
    if gdig is not None:
        g = gdig.cpu().numpy()
        assert (g[1:] == SENTINEL_BYTE).all()
        out += (g[:1],)
    return out + (dig[:NE],)


def same(x, y):
    return len(x) == len(y) and all(np.array_equal(a, b) for a, b in zip(x, y))


@pytest.mark.parametrize("keyed", [False, True], ids=["fresh", "keyed"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_unstaged_staged_and_dev_forms_return_the_same_bytes(ctx, entry, keyed):
    c = big_of(entry)
    key_id, keys = None, dict(qx=c.qx, qy=c.qy)
    if keyed:
        reg = ctx.key_register if entry == "p256" else ctx.p384_key_register
        ids = [reg(*(v.to_bytes(c.qx.shape[1], "big") for v in q)) for q in c.keys]
        key_id = np.array([ids[k] for k in c.kidx], dtype=np.uint32)
        keys = dict(key_id=key_id)
    gather = dict(gather_spans=GATHER) if entry == "p256" else {}
    host = host_form(ctx, c, keys, **gather)
    assert np.array_equal(host[1], c.status) and np.array_equal(host[0], c.status == 0) and np.array_equal(host[-1], c.digests)
    assert host[0][64] == (c.status[64] == 0)              # the second verdict word's one row
    if gather:
        assert bytes(host[2][0]) == hashlib.sha256(bytes(c.arena[3:303]) + bytes(c.arena[310:350])).digest()
    staged = host_form(ctx, c, keys, stage_token=ctx.arena_stage(c.arena), **gather)
    assert same(host, staged)
    if entry != "p256":                                    # the P-384 entries only read a staged upload, and need no arena pointer with one
        assert same(host, host_form(ctx, c, keys, stage_token=ctx.arena_stage(c.arena), arena=None))
    assert same(host, dev_form(ctx, c, key_id, GATHER if gather else None))


@pytest.mark.parametrize("keyed", [False, True], ids=["fresh", "keyed"])
def test_p256_with_pseudonym_rows_and_a_gathered_message(ctx, keyed):
    """two pseudonym signatures over messages behind the ECDSA ones in the same arena, on the second stream: unstaged and staged agree,
    the pseudonym statuses are the oracle's (idemix_common), and the ECDSA rows do not notice the riders"""
    c = big_of("p256")
    keys = dict(qx=c.qx, qy=c.qy)
    if keyed:
        ids = [ctx.key_register(q[0].to_bytes(32, "big"), q[1].to_bytes(32, "big")) for q in c.keys]
        keys = dict(key_id=np.array([ids[k] for k in c.kidx], dtype=np.uint32))
    nb = make_nym_batch(register_issuers(ctx), 2, 4)
    narena, noff, iid, cols, expect = nb.arrays()
    arena = np.concatenate([c.arena, narena])
    assert arena.size <= c.tail_base
    nym = (np.stack([noff[:-1], noff[1:]], axis=1).astype(np.uint32) + np.uint32(c.arena.size), iid, cols)
    alone = host_form(ctx, c, keys, gather_spans=GATHER)
    host = host_form(ctx, c, keys, gather_spans=GATHER, arena=arena, nym=nym)
    staged = host_form(ctx, c, keys, gather_spans=GATHER, arena=arena, nym=nym, stage_token=ctx.arena_stage(arena))
    assert same(alone, host[:-1]) and same(host[:-1], staged[:-1]) and same(host[-1], staged[-1])
    assert np.array_equal(host[1], c.status) and np.array_equal(host[-1][1], expect) and np.array_equal(host[-1][0], expect == 0)
