"""SHA3-256 on the device (fabric-mod_amd/csrc/sha3_256.h, sha3_kernels.hip) through the public entry points: the batched hash against
hashlib.sha3_256 at every length and alignment around the 136-byte rate, hash + verify against the CPU oracle for e = SHA3-256(msg),
the described batch with FABGPU_IDB_SHA3_256 (mid-states of shared prefixes, spans, tail, staged arena; gathered digests stay
SHA-256), and the provider's hash_sha3 option: Hash, identity.Verify by hash family, the coalescer's two queues, the CPU audit."""
import hashlib
import threading

import numpy as np
import pytest

import bccsp_sw_oracle as po
import coracle
import fabgpu

pytestmark = pytest.mark.gpu

N_INT = coracle.N_INT
LENGTHS = list(range(274)) + [4097, 65537]          # two rate blocks and a byte, then many blocks
PREFIX_LENS = (0, 1, 135, 136, 137, 271, 272, 273, 300)
SUFFIX_LENS = (0, 1, 134, 135, 136, 137)


@pytest.fixture(scope="module")
def ctx():
    c = fabgpu.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_lane_ctx():
    c = fabgpu.Context(device=0, flags=fabgpu.FLAG_ONE_LANE_ONLY)
    yield c
    c.close()


def _sha3(b: bytes) -> bytes:
    return hashlib.sha3_256(b).digest()


def _digests(msgs):
    return np.frombuffer(b"".join(_sha3(m) for m in msgs), dtype=np.uint8).reshape(len(msgs), 32)


def _dummy_sigs(n):
    """(qx, qy, r, s) that mean nothing: for calls whose digests are what is looked at"""
    z = np.zeros((n, 32), np.uint8)
    z[:, 31] = 1
    return z, z.copy(), z.copy(), z.copy()


# ---- 1. hash only ------------------------------------------------------------------------------------------------------------------
_SOURCE = np.random.default_rng(136).integers(0, 256, size=70000, dtype=np.uint8)


def _consecutive(lens, lead=3):
    """offsets mode: `lead` bytes of junk, then the messages back to back (off[0] != 0; starts fall on every alignment)"""
    off = np.concatenate([[lead], lead + np.cumsum(lens)]).astype(np.uint32)
    arena = np.random.default_rng(int(sum(lens)) + len(lens)).integers(0, 256, size=int(off[-1]) + 1, dtype=np.uint8)
    return arena, off


def test_hash_offsets_mode_every_length_and_wave_shape(ctx):
    at, aligns = 0, set()
    for n in (1, 63, 64, 65, 257):                    # partial wave, wave boundary, one lane of a second wave, second workgroup
        lens = [LENGTHS[(at + i) % len(LENGTHS)] for i in range(n)]
        at += n
        arena, off = _consecutive(lens)
        aligns |= {int(o) % 8 for o in off[:-1]}
        got = ctx.sha3_256_batch(arena, off)
        want = _digests([arena[off[i]:off[i + 1]].tobytes() for i in range(n)])
        bad = [(i, lens[i]) for i in range(n) if got[i].tobytes() != want[i].tobytes()]
        assert not bad, "n = %d: (message, length) that disagree with hashlib.sha3_256: %s" % (n, bad[:8])
    assert at >= len(LENGTHS) and aligns == set(range(8))


def test_hash_one_wave_with_lengths_0_135_136_65537_side_by_side(ctx):
    lens = [0, 135, 136, 65537]
    arena, off = _consecutive(lens, lead=5)
    got = ctx.sha3_256_batch(arena, off)
    for i, ln in enumerate(lens):
        assert got[i].tobytes() == _sha3(arena[off[i]:off[i + 1]].tobytes()), ln
    assert got[0].tobytes().hex() == "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a"


def test_hash_spans_mode_alignments_empty_and_overlapping(ctx):
    """spans mode is the described batch's (FABGPU_IDB_SPANS | FABGPU_IDB_SHA3_256, digests asked for): every message a (start, end)
    pair into one arena - message i starts at alignment i mod 8, every seventh is empty, every fifth lies inside its predecessor"""
    arena = _SOURCE
    for n in (1, 63, 64, 65, 257):
        spans, pos = [], 11
        for i in range(n):
            ln = LENGTHS[(7 * n + i) % 274] if i % 7 != 3 else 0
            if i % 5 == 4 and spans:
                s0 = spans[-1][0] + 1                                            # overlaps the previous message
            else:
                s0 = pos + (i % 8 - pos % 8) % 8
                pos = s0 + ln
            spans.append((s0, s0 + ln))
        if n == 257:
            spans[100] = (1, 1 + 4097)                                           # (and the long ones, overlapping everything)
            spans[200] = (2, 2 + 65537)
        assert {s0 % 8 for s0, _ in spans} == set(range(8)) or n < 8
        assert max(e for _, e in spans) < arena.size
        qx, qy, r, s = _dummy_sigs(n)
        res = ctx.identity_verify_batch(arena, np.array(spans, dtype=np.uint32).reshape(-1), r, s, qx=qx, qy=qy, spans=True, sha3=True, want_digests=True)
        got = res[-1]
        bad = [(i, spans[i]) for i in range(n) if got[i].tobytes() != _sha3(arena[spans[i][0]:spans[i][1]].tobytes())]
        assert not bad, "n = %d: spans that disagree with hashlib.sha3_256: %s" % (n, bad[:8])


# ---- 2. hash + verify, statuses 0-4 --------------------------------------------------------------------------------------------------
_tuples = {}


def _signed_tuples():
    """320 tuples by 4 signers over SHA3-256 of their messages, about a third broken one way each, and the oracle's status for
    e = SHA3-256(message as submitted).  Made once, never changed."""
    if not _tuples:
        n, nkeys = 320, 4
        rng = np.random.default_rng(320)
        msgs = [bytes(rng.integers(0, 256, size=int(ln), dtype=np.uint8)) for ln in rng.integers(1, 300, size=n)]
        b = coracle.make_pool_batch(n, seed=321, nkeys=nkeys, digests=_digests(msgs))
        qx, qy, r, s, ki = b["qx"].copy(), b["qy"].copy(), b["r"].copy(), b["s"].copy(), b["key_index"].copy()
        off_curve = np.zeros(n, bool)
        kinds = ("msg", "r", "high_s", "r_ge_n", "r_zero", "off_curve")
        for j, i in enumerate(range(0, n, 3)):
            k = kinds[j % len(kinds)]
            if k == "msg":
                m = bytearray(msgs[i]); m[len(m) // 2] ^= 0x10; msgs[i] = bytes(m)
            elif k == "r":
                r[i, 20] ^= 0x04
            elif k == "high_s":
                s[i] = np.frombuffer((N_INT - int.from_bytes(s[i].tobytes(), "big")).to_bytes(32, "big"), dtype=np.uint8)
            elif k == "r_ge_n":
                r[i] = np.frombuffer((N_INT + j).to_bytes(32, "big"), dtype=np.uint8)
            elif k == "r_zero":
                r[i] = 0
            else:
                qy[i, 31] ^= 1
                off_curve[i] = True
        off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)
        arena = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8).copy()
        want = coracle.verify_batch(qx, qy, _digests(msgs), r, s)
        assert set(want.tolist()) == {0, 1, 2, 3, 4} and 0.6 < (want == 0).mean() < 0.7
        out = dict(arena=arena, off=off, qx=qx, qy=qy, r=r, s=s, key_index=ki, off_curve=off_curve, want=want, pool_qx=b["pool_qx"], pool_qy=b["pool_qy"], msgs=msgs)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _tuples.update(out)
    return _tuples


@pytest.mark.parametrize("which", ["auto", "one-lane"])
def test_hash_then_verify_fresh_keys_vs_oracle(ctx, one_lane_ctx, which):
    t = _signed_tuples()
    c = ctx if which == "auto" else one_lane_ctx
    bits, st = c.sha3_256_p256_verify_batch(t["arena"], t["off"], qx=t["qx"], qy=t["qy"], r=t["r"], s=t["s"])
    assert (st == t["want"]).all() and (bits == (t["want"] == 0)).all()


def test_hash_then_verify_registered_keys_vs_oracle(ctx):
    t = _signed_tuples()
    ids = np.array([ctx.key_register(t["pool_qx"][j].tobytes(), t["pool_qy"][j].tobytes()) for j in range(4)], dtype=np.uint32)
    key_id = ids[t["key_index"]]
    key_id[t["off_curve"]] = 4000                    # a registered key is on the curve: "not a point" by id is a slot nobody holds - status 4 too
    bits, st = ctx.sha3_256_p256_verify_batch(t["arena"], t["off"], r=t["r"], s=t["s"], key_id=key_id)
    assert (st == t["want"]).all() and (bits == (t["want"] == 0)).all()


# ---- 3. the families do not cross ----------------------------------------------------------------------------------------------------
def test_a_signature_over_one_family_is_invalid_under_the_other(ctx):
    n = 70
    rng = np.random.default_rng(3)
    msgs = [bytes(rng.integers(0, 256, size=int(ln), dtype=np.uint8)) for ln in rng.integers(1, 200, size=n)]
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)
    arena = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8)
    d2 = np.frombuffer(b"".join(hashlib.sha256(m).digest() for m in msgs), dtype=np.uint8).reshape(n, 32)
    b2 = coracle.make_batch(n, seed=32, digests=d2)
    b3 = coracle.make_batch(n, seed=33, digests=_digests(msgs))
    _, st = ctx.sha3_256_p256_verify_batch(arena, off, qx=b2["qx"], qy=b2["qy"], r=b2["r"], s=b2["s"])
    assert (st == 1).all()                            # signed over SHA-256(msg)
    _, st = ctx.sha256_p256_verify_batch(arena, off, b3["qx"], b3["qy"], b3["r"], b3["s"])
    assert (st == 1).all()                            # signed over SHA3-256(msg)
    _, st = ctx.sha3_256_p256_verify_batch(arena, off, qx=b3["qx"], qy=b3["qy"], r=b3["r"], s=b3["s"])
    assert (st == 0).all()
    _, st = ctx.sha256_p256_verify_batch(arena, off, b2["qx"], b2["qy"], b2["r"], b2["s"])
    assert (st == 0).all()


# ---- 4. the described batch with FABGPU_IDB_SHA3_256 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("keyed", [False, True])
def test_described_batch_prefix_grid_spans_tail_digests_and_gather(ctx, keyed):
    rng = np.random.default_rng(44)
    pre_bytes = [bytes(rng.integers(0, 256, size=L, dtype=np.uint8)) for L in PREFIX_LENS]
    grid = [(p, L) for p in range(len(PREFIX_LENS)) for L in SUFFIX_LENS] + [(0xFFFFFFFF, L) for L in SUFFIX_LENS]   # ... and no prefix at all
    n = len(grid)
    sfx = [bytes(rng.integers(0, 256, size=L, dtype=np.uint8)) for _, L in grid]
    # arena: junk, the prefixes (two bytes apart), junk, the suffixes; the last six suffixes live in the TAIL
    parts, pos, pspans, spans = [b"\x11" * 3], 3, [], []
    for p in pre_bytes:
        pspans.append((pos, pos + len(p))); parts.append(p + b"\x22\x22"); pos += len(p) + 2
    n_tail = 6
    for x in sfx[:n - n_tail]:
        spans.append((pos, pos + len(x))); parts.append(x); pos += len(x)
    body = b"".join(parts)
    tail_base = (len(body) + 63) // 64 * 64 + 64
    tail, tpos = b"\x33", 1
    for x in sfx[n - n_tail:]:
        spans.append((tail_base + tpos, tail_base + tpos + len(x))); tail += x; tpos += len(x)
    arena = np.frombuffer(body + b"\0", dtype=np.uint8)
    msgs = [(pre_bytes[p] if p != 0xFFFFFFFF else b"") + x for (p, _), x in zip(grid, sfx)]
    want_dig = _digests(msgs)
    b = coracle.make_pool_batch(n, seed=45, nkeys=4, invalid_frac=0.25, digests=want_dig)
    want = coracle.verify_batch(b["qx"], b["qy"], b["e"], b["r"], b["s"])
    want[b["kind"] == 1] = 0                          # kind 1 flipped e only: in hash mode the message decides
    assert (want == 0).any() and (want == 1).any() and (want == 2).any()
    perm = rng.permutation(n)
    kw = dict(qx=b["qx"][perm], qy=b["qy"][perm])
    if keyed:
        ids = np.array([ctx.key_register(b["pool_qx"][j].tobytes(), b["pool_qy"][j].tobytes()) for j in range(4)], dtype=np.uint32)
        kw = dict(key_id=ids[b["key_index"]][perm])
    sp = np.array(spans, dtype=np.uint32)[perm].reshape(-1)
    pre_idx = np.array([p for p, _ in grid], dtype=np.uint32)[perm]
    g, want_g = [], []
    for j in range(9):
        a0, a1 = 5 + 17 * j, 5 + 17 * j + 40 * j
        g.append([a0, a1, 7, 7, a1 + 3, a1 + 3 + j])
        want_g.append(hashlib.sha256(arena[a0:a1].tobytes() + arena[a1 + 3:a1 + 3 + j].tobytes()).digest())
    common = dict(pre_off=np.array(pspans, dtype=np.uint32).reshape(-1), pre_idx=pre_idx, spans=True, gather_spans=np.array(g, dtype=np.uint32),
                  want_digests=True, **kw)
    bits, st, gdig, dig = ctx.identity_verify_batch(arena, sp, b["r"][perm], b["s"][perm], tail=np.frombuffer(tail, dtype=np.uint8), tail_base=tail_base,
                                                    sha3=True, **common)
    bad = [grid[perm[i]] for i in range(n) if dig[i].tobytes() != want_dig[perm[i]].tobytes()]
    assert not bad, "(prefix index, suffix length) whose digest is not hashlib.sha3_256(prefix || msg): %s" % bad
    assert [d.tobytes() for d in gdig] == want_g                                  # TxID / proposal hash stay SHA-256
    assert (st == want[perm]).all() and (bits == (want[perm] == 0)).all()
    # the same bytes staged ahead (the tail's bytes part of the upload, where its spans point)
    whole = np.frombuffer(body + bytes(tail_base - len(body)) + tail + b"\0", dtype=np.uint8)
    tok = ctx.arena_stage(whole)
    bits2, st2, gdig2, dig2 = ctx.identity_verify_batch(whole, sp, b["r"][perm], b["s"][perm], stage_token=tok, sha3=True, **common)
    assert (dig2 == dig).all() and (st2 == st).all() and (bits2 == bits).all() and [d.tobytes() for d in gdig2] == want_g
    # without the flag the very same batch is a SHA-256 batch: other digests, and no signature over a SHA3 digest verifies
    _, st3, _, dig3 = ctx.identity_verify_batch(arena, sp, b["r"][perm], b["s"][perm], tail=np.frombuffer(tail, dtype=np.uint8), tail_base=tail_base, **common)
    assert [d.tobytes() for d in dig3] == [hashlib.sha256(msgs[i]).digest() for i in perm] and not (st3 == 0).any()
    # an unknown flag bit is refused
    with pytest.raises(fabgpu.FabgpuError) as ei:
        ctx.identity_verify_batch(arena, sp, b["r"][perm], b["s"][perm], tail=np.frombuffer(tail, dtype=np.uint8), tail_base=tail_base, flags=8, **common)
    assert "(%d)" % fabgpu.FABGPU_EINVAL in str(ei.value)


# ---- 5. the provider -----------------------------------------------------------------------------------------------------------------
def _keypair(seed):
    d = 1 + seed * 7919
    return d, fabgpu.ECDSAPublicKey(*po.pt_mul(d, (po.GX, po.GY)))


def _sign(d, digest, k):
    return po.marshal_ecdsa_signature(*po.sign_raw(d, digest, k))


@pytest.fixture(scope="module")
def csp3():
    c = fabgpu.GPUCSP(device=0, hash_sha3=1)
    yield c
    c.close()


def test_provider_option_on_hash_and_identity_by_family(csp3):
    assert csp3.get_option("hash_sha3") == 1
    for m in (b"", b"abc", bytes(range(256)) * 3):
        assert csp3.hash(m, fabgpu.SHA3_256Opts()) == _sha3(m)
        assert csp3.hash(m, fabgpu.SHA256Opts()) == hashlib.sha256(m).digest()

    class SHA3_384Opts:
        algorithm = "SHA3_384"
    with pytest.raises(fabgpu.BCCSPError, match=r"Unsupported 'HashOpt' provided \[SHA3_384\]"):
        csp3.hash(b"x", SHA3_384Opts())
    d, pk = _keypair(11)
    msg = b"an MSP whose SignatureHashFamily is SHA3"
    sig3, sig2 = _sign(d, _sha3(msg), 0xBEEF), _sign(d, hashlib.sha256(msg).digest(), 0xBEEF)
    id3 = fabgpu.Identity(csp3, pk, "SHA3")
    assert id3.verify(msg, sig3) is None
    with pytest.raises(fabgpu.BCCSPError, match="The signature is invalid"):
        id3.verify(msg, sig2)
    id2 = fabgpu.Identity(csp3, pk, "SHA2")
    assert id2.verify(msg, sig2) is None
    with pytest.raises(fabgpu.BCCSPError, match="The signature is invalid"):
        id2.verify(msg, sig3)
    with pytest.raises(fabgpu.BCCSPError, match=r"hash familiy not recognized \[barf\]"):
        fabgpu.Identity(csp3, pk, "barf").verify(msg, sig3)
    assert csp3.identity_verify_batch([pk, pk], [msg, msg], [sig3, sig2], hash_family="barf") == ["hash familiy not recognized [barf]"] * 2
    assert csp3.identity_verify_batch([pk, pk], [msg, msg], [sig3, sig2], hash_family="SHA3") == [None, "The signature is invalid"]
    # registered signers: the keyed road
    csp3.key_import((pk.x, pk.y))
    assert csp3.identity_verify_batch([pk, pk], [msg, msg], [sig3, sig2], hash_family="SHA3") == [None, "The signature is invalid"]


def test_provider_coalescer_keeps_the_families_apart(csp3):
    nthreads = 32
    d, pk = _keypair(12)
    errors = []
    barrier = threading.Barrier(nthreads)

    def worker(t):
        family = "SHA3" if t % 2 else "SHA2"
        msg = b"caller %d of family %s" % (t, family.encode())
        own = _sha3(msg) if t % 2 else hashlib.sha256(msg).digest()
        other = hashlib.sha256(msg).digest() if t % 2 else _sha3(msg)
        sig_own, sig_other = _sign(d, own, 1000 + t), _sign(d, other, 2000 + t)
        barrier.wait()
        try:
            for _ in range(3):
                got = (csp3.identity_verify_coalesced(pk, msg, sig_own, hash_family=family), csp3.identity_verify_coalesced(pk, msg, sig_other, hash_family=family))
                if got != (None, "The signature is invalid"):
                    errors.append((t, family, got))
        except Exception as x:                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((t, family, repr(x)))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(nthreads)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[:4]
    assert csp3.identity_verify_coalesced(pk, b"m", b"\x30\x00", hash_family="barf") == "hash familiy not recognized [barf]"


def test_provider_option_off_answers_as_before():
    csp = fabgpu.GPUCSP(device=0)
    try:
        assert csp.get_option("hash_sha3") == 0
        d, pk = _keypair(13)
        msg = b"default provider"
        with pytest.raises(fabgpu.BCCSPError, match="failed computing digest: SHA3 is served by bccsp/sw, not by the GPU provider"):
            fabgpu.Identity(csp, pk, "SHA3").verify(msg, _sign(d, _sha3(msg), 77))
        with pytest.raises(fabgpu.BCCSPError, match=r"hash familiy not recognized \[barf\]"):
            fabgpu.Identity(csp, pk, "barf").verify(msg, b"\x30\x00")
        with pytest.raises(fabgpu.BCCSPError, match=r"Unsupported 'HashOpt' provided \[SHA3_256\]"):
            csp.hash(msg, fabgpu.SHA3_256Opts())
        assert csp.identity_verify_batch([pk], [msg], [_sign(d, _sha3(msg), 77)], hash_family="SHA3") == \
            ["failed computing digest: SHA3 is served by bccsp/sw, not by the GPU provider"]
        # ... and the switch works on the living provider
        assert csp.set_option("hash_sha3", 1) == 0
        assert csp.hash(msg, fabgpu.SHA3_256Opts()) == _sha3(msg)
        assert fabgpu.Identity(csp, pk, "SHA3").verify(msg, _sign(d, _sha3(msg), 77)) is None
    finally:
        csp.close()


# ---- 6. the CPU audit re-hashes with the call's family --------------------------------------------------------------------------------
def test_audit_rehashes_sha3_calls_with_sha3():
    d, pk = _keypair(14)
    msgs = [b"audited message %d " % i * (1 + i % 9) for i in range(64)]

    def run(family, h):
        csp = fabgpu.GPUCSP(device=0, hash_sha3=1, audit_permille=1000)
        try:
            sigs = [_sign(d, h(m), 5000 + i) for i, m in enumerate(msgs)]
            assert csp.identity_verify_batch([pk] * 64, msgs, sigs, hash_family=family) == [None] * 64
            for m in msgs[:8]:
                assert csp.hash(m, fabgpu.SHA3_256Opts() if family == "SHA3" else fabgpu.SHA256Opts()) == h(m)
            return csp.audit_stats(), csp.poisoned()
        finally:
            csp.close()

    st2, p2 = run("SHA2", lambda m: hashlib.sha256(m).digest())
    st3, p3 = run("SHA3", _sha3)
    # audit_host / bccsp_host.cpp AuditDirect: every "valid" of a direct call is sampled (permille 1000) - the 64 identity verifications;
    # bccsp.Hash hands out no memo entry and is not sampled under either family
    assert st2["direct_audits"] == 64 and st2["mismatches"] == 0 and p2 is None
    assert st3["direct_audits"] == 64 and st3["mismatches"] == 0 and p3 is None
    assert st3["digest_audits"] == st2["digest_audits"] and st3["verdict_audits"] == st2["verdict_audits"]
