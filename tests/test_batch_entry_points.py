"""The nine host-pointer batch entry points of the C ABI (fabgpu_p256_verify_batch ... fabgpu_sha3_256_p256_verify_batch_keyed), called
raw through ctypes: they share one staging path - [u32 ids padded to 64 bytes |] k fields of n x 32 bytes in one pinned buffer, verdict
words and status bytes at round_up(words * 8, 64) in another - and one failure rule.  Checked here: the layout at the sizes where its
padding changes, one call after another on one context, a NULL arena, and the failure contract of all nine under FABGPU_FAULT_INJECT."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import coracle
import fabgpu
import idemix_oracle as io
from idemix_common import NymBatch, be32, fixtures, make_batch as make_nym_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NINE = ["p256_verify_batch", "p256_verify_batch_keyed", "sha256_batch", "sha256_p256_verify_batch", "sha256_p256_verify_batch_keyed",
        "idemix_nym_verify_batch", "sha3_256_batch", "sha3_256_p256_verify_batch", "sha3_256_p256_verify_batch_keyed"]
HASH_ONLY = ("sha256_batch", "sha3_256_batch")
TAKES_MESSAGES = [x for x in NINE if not x.startswith("p256_")]
# 16 | 17: round_up(n * 4, 64), the id column's padding; 64 | 65: the verdict words and where the status bytes start behind them
SIZES = [1, 15, 16, 17, 63, 64, 65, 129]
BASE = 1000                                            # off[0]: the entry points rebase the offsets to the span they copy
N_INT = coracle.N_INT
_u8, _u32, _u64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64))
SENTINEL_WORD, SENTINEL_BYTE = 0xA5A5A5A5A5A5A5A5, 0xEE


def _p(a, t=_u8):
    return None if a is None else a.ctypes.data_as(t)


def call(L, h, name, n, arena, off, ids, cols, bits, out):
    """One raw call.  cols: the entry point's n x 32 fields in its own order; ids: key ids / issuer ids; out: the status bytes (None:
    not wanted) - for the two hash-only calls the digests."""
    f = getattr(L, "fabgpu_" + name)
    c = [_p(x) for x in cols]
    if name in HASH_ONLY:
        return f(h, n, _p(arena), _p(off, _u32), _p(out))
    if name == "p256_verify_batch":
        return f(h, n, *c, _p(bits, _u64), _p(out))
    if name == "p256_verify_batch_keyed":
        return f(h, n, _p(ids, _u32), *c, _p(bits, _u64), _p(out))
    if ids is not None or name == "idemix_nym_verify_batch":
        return f(h, n, _p(arena), _p(off, _u32), _p(ids, _u32), *c, _p(bits, _u64), _p(out))
    return f(h, n, _p(arena), _p(off, _u32), *c, _p(bits, _u64), _p(out))


def verdicts(ctx, name, n, arena, off, ids, cols, want_status=True):
    bits = np.full((n + 63) // 64, SENTINEL_WORD, dtype=np.uint64)
    st = np.full(n, SENTINEL_BYTE, dtype=np.uint8) if want_status else None
    rc = call(fabgpu.load(), ctx.handle, name, n, arena, off, ids, cols, bits, st)
    assert rc == 0, (name, n, rc)
    return fabgpu.unpack_bits(bits, n), st


def digests(ctx, name, n, arena, off):
    out = np.full((n, 32), SENTINEL_BYTE, dtype=np.uint8)
    rc = call(fabgpu.load(), ctx.handle, name, n, arena, off, None, (), None, out)
    assert rc == 0, (name, n, rc)
    return out


# ---- inputs and what the oracles say of them: made once per size, never changed -----------------------------------------------------
_HASH = {"sha256": lambda m: hashlib.sha256(m).digest(), "sha3_256": lambda m: hashlib.sha3_256(m).digest()}
KEY_D = np.frombuffer(bytes(range(1, 33)) + bytes(range(101, 133)), dtype=np.uint8).reshape(2, 32).copy()   # two signers' private scalars


def _hashes(family, msgs):
    return np.frombuffer(b"".join(_HASH[family](m) for m in msgs), dtype=np.uint8).reshape(len(msgs), 32).copy()


def key_pool():
    qx, qy = np.zeros((2, 32), np.uint8), np.zeros((2, 32), np.uint8)
    for j in range(2):
        coracle.lib().oracle_p256_pubkey(coracle._p(KEY_D[j:j + 1]), coracle._p(qx[j:j + 1]), coracle._p(qy[j:j + 1]))
    return qx, qy


def two_key_batch(n, seed, e):
    """coracle.make_batch for two signers that alternate: key_index[i] = i % 2 names the key a row is SUBMITTED under.  One row in
    five is broken: a flipped digest bit / the other signer's key / the high-S mirror / r + 1, in turn (`kind` 1..4)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    k[:, 0] &= 0x7F
    k[:, 31] |= 1
    ki = (np.arange(n) % 2).astype(np.uint32)
    e = e.copy()
    qx, qy, r, s = (np.zeros((n, 32), np.uint8) for _ in range(4))
    P = coracle._p
    coracle.lib().oracle_p256_make_batch(ctypes.c_size_t(n), P(np.ascontiguousarray(KEY_D[ki])), P(k), P(e), P(qx), P(qy), P(r), P(s))
    kind = np.zeros(n, dtype=np.uint8)
    for j, i in enumerate(rng.choice(n, size=int(round(n * 0.2)), replace=False)):
        kind[i] = m = 1 + j % 4
        if m == 1:
            e[i, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        elif m == 2:
            ki[i] ^= 1
        elif m == 3:
            s[i] = np.frombuffer((N_INT - int.from_bytes(s[i].tobytes(), "big")).to_bytes(32, "big"), dtype=np.uint8)
        else:
            r[i] = np.frombuffer(((int.from_bytes(r[i].tobytes(), "big") + 1) % (1 << 256)).to_bytes(32, "big"), dtype=np.uint8)
    return dict(e=e, r=r, s=s, kind=kind, key_index=ki)


def _arena(msgs):
    lens = [len(m) for m in msgs]
    off = (BASE + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint32)
    arena = np.frombuffer((bytes(range(256)) * 4)[:BASE] + b"".join(msgs) + b"\0", dtype=np.uint8).copy()   # BASE bytes nobody refers to in front
    return arena, off


def _flip_messages(msgs, rows):
    """a row whose DIGEST the batch maker flipped is, for an entry point that hashes, a row whose MESSAGE has a flipped bit"""
    out = list(msgs)
    for i in rows:
        m = bytearray(out[i])
        m[len(m) // 2] ^= 0x10
        out[i] = bytes(m)
    return out


_nym_base = []
_cases = {}
NYM_BASE = 48


def _nym_rows(n):
    """n rows out of NYM_BASE seeded pseudonym signatures by one issuer (signing is pure Python: seconds per hundred), taken round and
    round from where the broken ones are - the first 17 of a seeded batch are all valid, behind them every second one is broken some
    way.  The verdict of a copy is the verdict of its original."""
    if not _nym_base:
        fx = fixtures()["MSP1OU1"]
        _nym_base.append(make_nym_batch([(fx["ipk"], fx["signer"].sk)], NYM_BASE, 21))
    b = _nym_base[0]
    rows = [i % NYM_BASE for i in range(129 - n, 129)]
    cols = [np.frombuffer(b"".join(b.rows[i][k] for i in rows), dtype=np.uint8).reshape(n, 32).copy() for k in range(6)]
    return [b.msgs[i] for i in rows], cols, np.array([b.expect[i] for i in rows], dtype=np.uint8)


def cases(n):
    """name -> dict(arena, off, ids (indices into the registered pair, or None), cols, want): every entry point's inputs at n rows, about
    one row in five invalid, and the oracle's status bytes (for the hash-only calls: hashlib's digests)"""
    if n in _cases:
        return _cases[n]
    rng = np.random.default_rng(5000 + n)
    msgs = [bytes(rng.integers(0, 256, size=int(ln), dtype=np.uint8)) for ln in rng.integers(1, 200, size=n)]
    pool_qx, pool_qy = key_pool()
    out = {}
    for family in ("sha256", "sha3_256"):
        e = _hashes(family, msgs)
        f = coracle.make_batch(n, seed=7000 + n, invalid_frac=0.2, digests=e)
        sent = _flip_messages(msgs, np.nonzero(f["kind"] == 1)[0])
        arena, off = _arena(sent)
        out[family + "_batch"] = dict(arena=arena, off=off, ids=None, cols=(), want=_hashes(family, sent))
        out[family + "_p256_verify_batch"] = dict(arena=arena, off=off, ids=None, cols=(f["qx"], f["qy"], f["r"], f["s"]),
                                                  want=coracle.verify_batch(f["qx"], f["qy"], _hashes(family, sent), f["r"], f["s"]))
        k = two_key_batch(n, 8000 + n, e)
        sent = _flip_messages(msgs, np.nonzero(k["kind"] == 1)[0])
        arena, off = _arena(sent)
        kq = (pool_qx[k["key_index"]], pool_qy[k["key_index"]])
        out[family + "_p256_verify_batch_keyed"] = dict(arena=arena, off=off, ids=k["key_index"], cols=(k["r"], k["s"]),
                                                        want=coracle.verify_batch(*kq, _hashes(family, sent), k["r"], k["s"]))
        if family == "sha256":                        # the two digest-given forms: the same tuples, e as the batch maker left it
            out["p256_verify_batch"] = dict(arena=None, off=None, ids=None, cols=(f["qx"], f["qy"], f["e"], f["r"], f["s"]),
                                            want=coracle.verify_batch(f["qx"], f["qy"], f["e"], f["r"], f["s"]))
            out["p256_verify_batch_keyed"] = dict(arena=None, off=None, ids=k["key_index"], cols=(k["e"], k["r"], k["s"]),
                                                  want=coracle.verify_batch(*kq, k["e"], k["r"], k["s"]))
    nmsgs, ncols, nwant = _nym_rows(n)
    arena, off = _arena(nmsgs)
    out["idemix_nym_verify_batch"] = dict(arena=arena, off=off, ids=np.zeros(n, dtype=np.uint32), cols=tuple(ncols), want=nwant)
    assert sorted(out) == sorted(NINE)
    for c in out.values():
        for v in [c["arena"], c["off"], c["ids"], c["want"], *c["cols"]]:
            if v is not None:
                v.setflags(write=False)
    _cases[n] = out
    return out


@pytest.fixture(scope="module")
def env():
    """one default context with two registered keys and one registered issuer: (ctx, the two key ids)"""
    c = fabgpu.Context(device=0)
    qx, qy = key_pool()
    key_ids = np.array([c.key_register(qx[j].tobytes(), qy[j].tobytes()) for j in range(2)], dtype=np.uint32)
    ipk = fixtures()["MSP1OU1"]["ipk"]
    assert c.idemix_issuer_register((be32(ipk.h_sk[0]), be32(ipk.h_sk[1])), (be32(ipk.h_rand[0]), be32(ipk.h_rand[1])), ipk.hash) == 0
    yield c, key_ids
    c.close()


def _ids(name, case, key_ids):
    if case["ids"] is None or name == "idemix_nym_verify_batch":
        return case["ids"]
    return np.ascontiguousarray(key_ids[case["ids"]])


def _check(ctx, key_ids, name, n):
    c = cases(n)[name]
    if name in HASH_ONLY:
        got = digests(ctx, name, n, c["arena"], c["off"])
        bad = [i for i in range(n) if got[i].tobytes() != c["want"][i].tobytes()]
        assert not bad, (name, n, bad[:8])
        return
    ids, want = _ids(name, c, key_ids), c["want"]
    bits, st = verdicts(ctx, name, n, c["arena"], c["off"], ids, c["cols"])
    assert (st == want).all(), (name, n, np.nonzero(st != want)[0][:8], st[st != want][:8], want[st != want][:8])
    assert (bits == (want == 0)).all(), (name, n)
    bits_only, _ = verdicts(ctx, name, n, c["arena"], c["off"], ids, c["cols"], want_status=False)
    assert (bits_only == (want == 0)).all(), (name, n)
    if name == "idemix_nym_verify_batch":              # issuer ids are optional (NULL: issuer 0); the fields stay behind the column's room
        bits, st = verdicts(ctx, name, n, c["arena"], c["off"], None, c["cols"])
        assert (st == want).all() and (bits == (want == 0)).all(), (name, n, "no issuer ids")


# ---- 1. the layout where its padding changes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", NINE)
def test_layout_at_the_padding_edges(env, name, n):
    ctx, key_ids = env
    want = cases(n)[name]["want"]
    if name not in HASH_ONLY and n >= 15:
        assert (want == 0).any() and (want != 0).any()
    _check(ctx, key_ids, name, n)


# ---- 2. one call after another on one context: nothing of a call's sizes or offsets may outlive it --------------------------------------
@pytest.mark.parametrize("keyed", ["p256_verify_batch_keyed", "sha256_p256_verify_batch_keyed", "sha3_256_p256_verify_batch_keyed"])
def test_keyed_65_then_fresh_17_then_keyed_1_on_one_context(env, keyed):
    ctx, key_ids = env
    _check(ctx, key_ids, keyed, 65)
    _check(ctx, key_ids, "p256_verify_batch", 17)
    _check(ctx, key_ids, keyed, 1)


# ---- 3. NULL arena ----------------------------------------------------------------------------------------------------------------------
_empty = {}


def _empty_message_cases():
    """n = 5 rows per message-taking entry point whose messages are all EMPTY: signatures over H(""), one row broken"""
    if _empty:
        return _empty
    n = 5
    pool_qx, pool_qy = key_pool()
    for family in ("sha256", "sha3_256"):
        e = _hashes(family, [b""] * n)
        f = coracle.make_batch(n, seed=91, digests=e)
        r = f["r"].copy()
        r[3, 7] ^= 2
        _empty[family + "_batch"] = dict(ids=None, cols=(), want=e)
        _empty[family + "_p256_verify_batch"] = dict(ids=None, cols=(f["qx"], f["qy"], r, f["s"]), want=coracle.verify_batch(f["qx"], f["qy"], e, r, f["s"]))
        k = two_key_batch(n, 92, e)
        assert (k["kind"] == 1).sum() == 1             # (its one broken row is a flipped digest bit: with the message hashed, a valid row)
        _empty[family + "_p256_verify_batch_keyed"] = dict(ids=k["key_index"], cols=(k["r"], k["s"]),
                                                           want=coracle.verify_batch(pool_qx[k["key_index"]], pool_qy[k["key_index"]], e, k["r"], k["s"]))
        assert (_empty[family + "_p256_verify_batch"]["want"] == [0, 0, 0, 1, 0]).all() and (_empty[family + "_p256_verify_batch_keyed"]["want"] == 0).all()
    import random
    fx = fixtures()["MSP1OU1"]
    ipk, sk, rng, b = fx["ipk"], fx["signer"].sk, random.Random(93), NymBatch()
    for i in range(n):
        nym, r_nym = io.make_nym(sk, ipk, rng)
        sig = io.nym_sign(sk, nym, r_nym, ipk, b"", rng)
        if i == 2:
            sig = dict(sig, nonce=be32(int.from_bytes(sig["nonce"], "big") ^ 4))
        b.add(0, ipk, nym, sig, b"")
    _, _, iid, cols, expect = b.arrays()
    assert (expect[[0, 1, 3, 4]] == 0).all() and expect[2] != 0
    _empty["idemix_nym_verify_batch"] = dict(ids=iid, cols=tuple(cols), want=expect)
    return _empty


@pytest.mark.parametrize("name", TAKES_MESSAGES)
def test_null_arena_serves_empty_messages_and_refuses_others(env, name):
    ctx, key_ids = env
    n = 5
    c = _empty_message_cases()[name]
    ids = _ids(name, c, key_ids)
    flat = np.full(n + 1, 7, dtype=np.uint32)          # every message empty (and not at offset 0)
    if name in HASH_ONLY:
        assert (digests(ctx, name, n, None, flat) == c["want"]).all()
    else:
        for want_status in (True, False):
            bits, st = verdicts(ctx, name, n, None, flat, ids, c["cols"], want_status=want_status)
            assert (bits == (c["want"] == 0)).all() and (st is None or (st == c["want"]).all()), (name, want_status)
    rising = np.array([7, 7, 7, 7, 7, 8], dtype=np.uint32)   # one byte of message and no arena to take it from
    bits = np.full(1, SENTINEL_WORD, dtype=np.uint64)
    out = np.full((n, 32) if name in HASH_ONLY else n, SENTINEL_BYTE, dtype=np.uint8)
    assert call(fabgpu.load(), ctx.handle, name, n, None, rising, ids, c["cols"], bits, out) == fabgpu.FABGPU_EINVAL
    assert (bits == SENTINEL_WORD).all() and (out == SENTINEL_BYTE).all()


# ---- 4. the failure contract of all nine: non-zero return, the caller's arrays untouched, the context usable for the next call ----------
def fault_contract_child(want):
    """Runs in a fresh process under FABGPU_FAULT_INJECT (a simulated failed submission / allocation on the host; the device is fine)."""
    L = fabgpu.load()
    ctx = fabgpu.Context(device=0)
    qx, qy = key_pool()
    try:
        key_ids = np.array([ctx.key_register(qx[j].tobytes(), qy[j].tobytes()) for j in range(2)], dtype=np.uint32)
    except fabgpu.FabgpuError:                        # "oom": no room for a key table either
        assert want == -3
        key_ids = np.array([0, 1], dtype=np.uint32)
    ipk = fixtures()["MSP1OU1"]["ipk"]
    assert ctx.idemix_issuer_register((be32(ipk.h_sk[0]), be32(ipk.h_sk[1])), (be32(ipk.h_rand[0]), be32(ipk.h_rand[1])), ipk.hash) == 0
    assert ctx.idemix_issuer_count() == 1 and (want == -3 or ctx.key_count() == 2)
    n_fields = {"p256_verify_batch": 5, "p256_verify_batch_keyed": 3, "idemix_nym_verify_batch": 6, "sha256_p256_verify_batch": 4,
                "sha3_256_p256_verify_batch": 4, "sha256_p256_verify_batch_keyed": 2, "sha3_256_p256_verify_batch_keyed": 2}
    for name in NINE:
        for n in (70, 5):                             # the second, differently sized call: the first one's failure left nothing behind
            rng = np.random.default_rng(n)
            b = coracle.make_batch(n, seed=n)
            cols = [b[k] for k in ("qx", "qy", "e", "r", "s")] + [rng.integers(0, 256, size=(n, 32), dtype=np.uint8)]
            cols = () if name in HASH_ONLY else cols[:n_fields[name]]
            keyed = name.endswith("_keyed")
            ids = np.ascontiguousarray(key_ids[np.arange(n) % 2]) if keyed else (np.zeros(n, np.uint32) if name.startswith("idemix") else None)
            off = (BASE + 40 * np.arange(n + 1)).astype(np.uint32)
            arena = rng.integers(0, 256, size=BASE + 40 * n + 64, dtype=np.uint8)
            bits = np.full((n + 63) // 64, SENTINEL_WORD, dtype=np.uint64)
            out = np.full((n, 32) if name in HASH_ONLY else n, SENTINEL_BYTE, dtype=np.uint8)
            rc = call(L, ctx.handle, name, n, arena, off, ids, cols, bits, out)
            assert rc == want, (name, n, rc)
            assert (bits == SENTINEL_WORD).all() and (out == SENTINEL_BYTE).all(), "%s (n = %d) failed and wrote to the caller's arrays" % (name, n)
    ctx.close()
    print("NINE_FAIL_CLEAN")


@pytest.mark.parametrize("mode,want", [("launch", -4), ("oom", -3)])
def test_all_nine_fail_clean_and_leave_the_context_usable(mode, want):
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import test_batch_entry_points as t; t.fault_contract_child(%d)" % (
        os.path.join(ROOT, "fabric-mod_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), want)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, FABGPU_FAULT_INJECT=mode), timeout=300)
    assert r.returncode == 0 and "NINE_FAIL_CLEAN" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
