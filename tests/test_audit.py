"""The sampled CPU audit of what the provider hands out from the device, and poisoning (include/fabgpu_bccsp.h "CPU audit";
fabric-mod_amd/csrc/audit_host.h; DESIGN.md 4.4e addendum).

With audit_permille > 0 the provider re-computes, in host code on the calling thread, a fixed share of the digest-memo hits
(fabgpu_csp_hash_lookup), of the verdict-memo hits (fabgpu_csp_memo_lookup) and of the "valid" answers of the direct calls; the first
disagreement poisons it for good.

CPU tests: the audit's SHA-256 against hashlib, its bccsp.Verify against the restated bccsp/sw (oracle/bccsp_sw_oracle.py csp_verify)
on every committed vector, the sampling rule.
GPU tests: a 4-transaction block with 2 endorsements each from tests/blockgen.py - 12 tuples, both memo kinds - and a variant with one
endorsement signature made invalid; corruption comes from the test hook fabgpu_csp_test_memo_corrupt, which edits host memory of the
library (nothing is launched, nothing faults)."""
import functools
import hashlib
import json
import os
import threading

import numpy as np
import pytest

import bccsp_sw_oracle as po
import blockbuilder as bb
import blockgen
import fabgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _load(name):
    d = json.load(open(os.path.join(G, name)))
    return d["vectors"] if isinstance(d, dict) and "vectors" in d else d


def _want(qx: int, qy: int, sig: bytes, digest: bytes) -> bool:
    """accept / reject of the restated bccsp/sw: (true, nil) is accept, (false, nil) and (false, err) are reject"""
    try:
        return po.csp_verify((qx, qy), sig, digest)
    except po.BCCSPError:
        return False


def _got(qx: int, qy: int, sig: bytes, digest: bytes) -> bool:
    return fabgpu.audit_p256_verify(qx.to_bytes(32, "big"), qy.to_bytes(32, "big"), sig, digest)


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_audit_sha256_equals_hashlib():
    rng = np.random.default_rng(31)
    for n in (0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, (1 << 20) + 1):
        msg = bytes(rng.integers(0, 256, size=n, dtype=np.uint8))
        assert fabgpu.audit_sha256(msg) == hashlib.sha256(msg).digest(), n


def test_audit_verify_equals_bccsp_sw_on_edge_vectors():
    n_accept = 0
    for v in _load("edge_kats.json"):
        qx, qy = int(v["qx"], 16), int(v["qy"], 16)
        if qx >> 256 or qy >> 256:
            continue                                     # (not a key the 32-byte boundary can carry)
        sig, dg = po.marshal_ecdsa_signature(int(v["r"], 16), int(v["s"], 16)), bytes.fromhex(v["e"])
        # the restated bccsp/sw assumes what KeyImport enforced: a key that is not on the curve never reaches Verify - the audit rejects it
        want = po.on_curve(qx, qy) and _want(qx, qy, sig, dg)
        assert _got(qx, qy, sig, dg) == want, v["name"]
        n_accept += want
    assert n_accept >= 20


def test_audit_verify_equals_bccsp_sw_on_der_vectors_and_digest_lengths():
    d = 1 + 5 * 7919
    qx, qy = po.pt_mul(d, (po.GX, po.GY))
    n = 0
    for v in _load("der_kats.json"):
        raw = bytes.fromhex(v["der"])
        for dg in (b"\x07", b"\x01" * 32, b"\xff" * 40):
            assert _got(qx, qy, raw, dg) == _want(qx, qy, raw, dg), (v["name"], len(dg))
            n += 1
    # ... and signatures that DO verify under each digest length, in each encoding the reference accepts
    good = [bytes.fromhex(v["der"]) for v in _load("der_kats.json") if v["ok"]]
    for k, dg in enumerate((b"\x07", b"\x01" * 32, b"\xff" * 40)):
        r, s = po.sign_raw(d, dg, 0x5EED + k)
        sig = po.marshal_ecdsa_signature(r, s)
        for how in ("trailing", "third"):
            enc = blockgen.crafted(sig, how)
            assert _want(qx, qy, enc, dg) is True and _got(qx, qy, enc, dg) is True
        assert _got(qx, qy, sig, dg) is True and _got(qx, qy, sig, dg + b"\x00") == _want(qx, qy, sig, dg + b"\x00")
        assert _got(qx, qy, po.marshal_ecdsa_signature(r, po.N - s), dg) is False         # high S
        for how in ("long_r", "long_s", "neg_r", "nonminimal"):
            enc = blockgen.crafted(sig, how)
            assert _got(qx, qy, enc, dg) is False and _want(qx, qy, enc, dg) is False
    assert n == 3 * 34 and len(good) == 7
    # the argument checks of CSP.Verify (bccsp/sw/impl.go:249-257)
    assert _got(qx, qy, b"", b"\x01") is False and _got(qx, qy, good[0], b"") is False


def test_audit_verify_equals_bccsp_sw_on_rfc6979_and_reference_certificates():
    f = json.load(open(os.path.join(G, "rfc6979_p256_sha256.json")))
    qx, qy = int(f["qx"], 16), int(f["qy"], 16)
    for v in f["vectors"]:
        dg = hashlib.sha256(v["message"].encode()).digest()
        r, s = int(v["r"], 16), int(v["s"], 16)
        sig = po.marshal_ecdsa_signature(r, s)
        assert _got(qx, qy, sig, dg) == _want(qx, qy, sig, dg) == (s <= po.HALF_N)
        assert _got(qx, qy, po.marshal_ecdsa_signature(r, po.N - s), dg) == (s > po.HALF_N)
    n_accept = 0
    for v in _load("ref_cert_kats.json"):
        qx, qy, sig, dg = int(v["qx"], 16), int(v["qy"], 16), bytes.fromhex(v["sig_der"]), bytes.fromhex(v["e"])
        want = _want(qx, qy, sig, dg)
        assert want == (v["low_s"] and v["expect_valid"])
        assert _got(qx, qy, sig, dg) == want, v["source"]
        n_accept += want
    assert n_accept == 65


def test_sampling_rule_is_exact():
    for permille in (0, 1, 250, 999, 1000):
        a = fabgpu.audit_sample(permille, 4000)
        assert int(a.sum()) == 4000 * permille // 1000
        want = [h * permille // 1000 != (h - 1) * permille // 1000 for h in range(1, 4001)]
        assert a.tolist() == want, permille
    assert fabgpu.audit_sample(250, 16).nonzero()[0].tolist() == [3, 7, 11, 15]          # exactly every fourth hit


def test_audit_permille_field_is_the_headers():
    """the appended field of fabgpu_csp_opts as ctypes lays it out = as the C compiler lays it out; an older, shorter struct stays valid"""
    import ctypes
    import subprocess
    import tempfile
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "fabgpu_bccsp.h"\nint main(void) { printf("%zu %zu %zu %d\\n", sizeof(fabgpu_csp_opts), ' \
          'offsetof(fabgpu_csp_opts, hash_memo_blocks), offsetof(fabgpu_csp_opts, audit_permille), FABGPU_EPOISONED); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "o.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), os.path.join(d, "o.c"), "-o", os.path.join(d, "o")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "o")], capture_output=True, text=True, check=True).stdout.split()]
    O = fabgpu._CspOptsAudit
    assert got == [ctypes.sizeof(O), O.hash_memo_blocks.offset, O.audit_permille.offset, fabgpu.FABGPU_EPOISONED]
    assert O._fields_[:-1] == fabgpu._CspOpts._fields_ and O._fields_[-1][0] == "audit_permille"


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
SEQ = 7


@functools.lru_cache(maxsize=None)
def _block(bad_endorsement=None, seed=901):
    """4 transactions x (creator + 2 endorsements) = 12 tuples; bad_endorsement = (tx, j): that endorsement signs other bytes"""
    fx = blockgen.fixture_signers()
    rng = np.random.default_rng(seed)
    sign = blockgen.make_signer(seed + 1)

    def craft(t, j, sig):
        return sign(fx[j][1], b"another message") if (t, j) == bad_endorsement else sig
    envs = [blockgen.endorser_tx(t, rng, fx[4 + t % 2], [fx[(t + j) % 4] for j in range(2)], sign, craft) for t in range(4)]
    return bb.block(SEQ, envs)


def clean():
    return _block()


def one_bad():
    return _block(bad_endorsement=(2, 1))


def _pass(csp, blk, seq=SEQ):
    """the block's memo-seeding pass -> [(message, key X, key Y, signature, status, device digest)] per tuple"""
    out = fabgpu.preverify_block2(csp, blk, block_seq=seq, seed_memo=True)
    assert out["memo_seeded"] == len(out["tuple_status"]) == 12
    tuples = []
    for i in range(12):
        sp = [int(x) for x in out["tuple_spans"][i]]
        msg = out["arena"][sp[2]:sp[2] + sp[3]] + out["arena"][sp[4]:sp[4] + sp[5]]
        q = bytes(out["tuple_qxy"][i])
        tuples.append((msg, q[:32], q[32:], out["arena"][sp[6]:sp[6] + sp[7]], int(out["tuple_status"][i]), bytes(out["tuple_digest"][i])))
    return tuples


def _seeded(blk=None, **kw):
    blk = clean() if blk is None else blk
    csp = fabgpu.GPUCSP(device=0, **kw)
    fabgpu.preverify_block(csp, blk)                     # first sight: the identities are learned
    return csp, _pass(csp, blk)


def _lookups(csp, tuples):
    """what the validators ask, in their order: Hash(msg) then Verify(k, sig, digest) per signature -> [(digest or None, status or None)]"""
    out = []
    for msg, qx, qy, sig, _, _ in tuples:
        d = fabgpu.hash_lookup(csp, msg)
        out.append((d, fabgpu.memo_lookup(csp, qx, qy, sig, d if d is not None else hashlib.sha256(msg).digest())))
    return out


def _assert_retired(csp, tuples, blk):
    """a poisoned provider: every lookup misses, every verify and pass entry point refuses, nothing new is seeded"""
    assert all(d is None and st is None for d, st in _lookups(csp, tuples))
    msg, qx, qy, sig, _, _ = tuples[0]
    k = fabgpu.ECDSAPublicKey(int.from_bytes(qx, "big"), int.from_bytes(qy, "big"))
    with pytest.raises(fabgpu.PoisonedError):
        csp.verify(k, sig, hashlib.sha256(msg).digest())
    with pytest.raises(fabgpu.PoisonedError):
        csp.verify_batch([k], [sig], [hashlib.sha256(msg).digest()])
    with pytest.raises(fabgpu.PoisonedError):
        csp.identity_verify_batch([k], [msg], [sig])
    with pytest.raises(fabgpu.PoisonedError):
        fabgpu.preverify_block(csp, blk)
    with pytest.raises(fabgpu.PoisonedError):
        fabgpu.preverify_block2(csp, blk, block_seq=SEQ + 1, seed_memo=True)
    assert fabgpu.memo_has_block(csp, SEQ + 1) == 0
    assert "poisoned" in fabgpu.strerror(fabgpu.FABGPU_EPOISONED)


@pytest.mark.gpu
def test_clean_pass_fully_audited_answers_as_unaudited():
    plain, tuples0 = _seeded()
    want = _lookups(plain, tuples0)
    assert plain.get_option("audit_permille") == 0 and plain.audit_stats()["digest_audits"] == 0
    plain.close()
    csp, tuples = _seeded(audit_permille=1000)
    assert tuples == tuples0 and csp.get_option("audit_permille") == 1000
    got = _lookups(csp, tuples)
    assert got == want and all(d == hashlib.sha256(t[0]).digest() and st == 0 for (d, st), t in zip(got, tuples))
    st = csp.audit_stats()
    assert st["digest_audits"] == 12 == fabgpu.hash_memo_stats(csp)["hits"] and st["verdict_audits"] == 12 == fabgpu.memo_stats(csp)["hits"]
    assert st["mismatches"] == 0 and st["skipped_nym"] == 0 and st["audit_ns"] > 0 and csp.poisoned() is None
    # the option's range
    with pytest.raises(fabgpu.FabgpuError):
        csp.set_option("audit_permille", 1001)
    with pytest.raises(fabgpu.FabgpuError):
        csp.set_option("audit_permille", -1)
    assert csp.set_option("audit_permille", 250) == 1000 and csp.get_option("audit_permille") == 250
    with pytest.raises(fabgpu.FabgpuError):
        fabgpu.GPUCSP(device=0, audit_permille=1001)
    csp.close()


@pytest.mark.gpu
def test_corrupted_digest_poisons():
    csp, tuples = _seeded(audit_permille=1000)
    assert fabgpu.memo_corrupt(csp, SEQ, 0, 1) == 0
    assert fabgpu.hash_lookup(csp, tuples[0][0]) == tuples[0][5] and csp.poisoned() is None
    assert fabgpu.hash_lookup(csp, tuples[1][0]) is None                    # the corrupted entry: a miss, the caller hashes for itself
    why = csp.poisoned()
    assert why is not None and "digest" in why and "entry 1" in why
    st = csp.audit_stats()
    assert st["mismatches"] == 1 and st["digest_audits"] == 2
    _assert_retired(csp, tuples, clean())
    assert csp.poisoned() == why                                             # the first reason stays
    csp.poison("again")
    assert csp.poisoned() == why
    csp.close()                                                              # fabgpu_csp_free still works


@pytest.mark.gpu
@pytest.mark.parametrize("make,entry,was", [(clean, 5, 0), (one_bad, 8, 1)], ids=["valid_to_bad", "bad_to_valid"])
def test_corrupted_verdict_poisons(make, entry, was):
    blk = make()
    csp, tuples = _seeded(blk, audit_permille=1000)
    assert [t[4] for t in tuples] == [was if i == entry else 0 for i in range(12)]      # (2, 1) is tuple 3 * 2 + 1 + 1 = 8
    assert fabgpu.memo_corrupt(csp, SEQ, 1, entry) == 0
    for i, (msg, qx, qy, sig, status, dg) in enumerate(tuples):
        got = fabgpu.memo_lookup(csp, qx, qy, sig, dg)
        if i < entry:
            assert got == status and csp.poisoned() is None
        else:
            assert got is None
    why = csp.poisoned()
    assert "verdict" in why and "entry %d" % entry in why and ("says valid" in why) == (was == 0)
    st = csp.audit_stats()
    assert st["mismatches"] == 1 and st["verdict_audits"] == entry + 1
    _assert_retired(csp, tuples, blk)
    csp.close()


@pytest.mark.gpu
def test_corruption_goes_unnoticed_without_the_switch():
    csp, tuples = _seeded()                                                  # audit_permille = 0: the default
    assert fabgpu.memo_corrupt(csp, SEQ, 0, 1) == 0 and fabgpu.memo_corrupt(csp, SEQ, 1, 5) == 0
    for i, (msg, qx, qy, sig, status, dg) in enumerate(tuples):
        d = fabgpu.hash_lookup(csp, msg)
        if i == 1:
            assert d is not None and d != dg and bytes(a ^ b for a, b in zip(d, dg)).count(b"\0") == 31   # one flipped bit, handed out
        else:
            assert d == dg
            assert fabgpu.memo_lookup(csp, qx, qy, sig, dg) == (1 if i == 5 else 0)                      # the toggled status, handed out
    assert csp.poisoned() is None and csp.audit_stats()["mismatches"] == 0
    assert sum(csp.audit_stats().values()) == 0
    csp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("meets_sample", [False, True])
def test_exact_sampling_at_250_permille(meets_sample):
    csp, tuples = _seeded(audit_permille=250)
    assert fabgpu.memo_corrupt(csp, SEQ, 1, 5) == 0
    order = [i for i in range(12) if i != 5]
    # 64 verdict hits; hits 4, 8, .. are audited.  The corrupted entry is asked as hit 62 (not sampled) or as hit 64 (sampled).
    asks = [order[h % 11] for h in range(64)]
    asks[61 if not meets_sample else 63] = 5
    for h, i in enumerate(asks, 1):
        msg, qx, qy, sig, status, dg = tuples[i]
        got = fabgpu.memo_lookup(csp, qx, qy, sig, dg)
        if i == 5:
            assert got == (None if meets_sample else 1), h                  # passes unseen on a hit that is not sampled
        else:
            assert got == 0, h
    st = csp.audit_stats()
    assert st["verdict_audits"] == 16 and st["mismatches"] == (1 if meets_sample else 0)
    assert (csp.poisoned() is not None) == meets_sample
    csp.close()


@pytest.mark.gpu
def test_direct_calls_fully_audited():
    vs = _load("ref_cert_kats.json")
    good = [v for v in vs if v["low_s"] and v["expect_valid"]][:64]
    bad = [v for v in vs if v["low_s"] and not v["expect_valid"]][:6] + [v for v in vs if not v["low_s"]][:2]
    use = good[:30] + bad[:4] + good[30:] + bad[4:]
    keys = [fabgpu.ECDSAPublicKey(int(v["qx"], 16), int(v["qy"], 16)) for v in use]
    sigs, digs = [bytes.fromhex(v["sig_der"]) for v in use], [bytes.fromhex(v["e"]) for v in use]
    want = [_want(k.x, k.y, s, d) for k, s, d in zip(keys, sigs, digs)]
    assert sum(want) == 64 and len(want) == 72
    csp = fabgpu.GPUCSP(device=0, audit_permille=1000)
    got = csp.verify_batch(keys, sigs, digs)
    assert [g[0] for g in got] == want
    st = csp.audit_stats()
    assert st["direct_audits"] == 64 and st["mismatches"] == 0 and csp.poisoned() is None
    # the one-signature verbs and identity.Verify (the message is hashed again by the audit) go through the same audit
    d, pk = 1 + 9 * 7919, None
    pk = fabgpu.ECDSAPublicKey(*po.pt_mul(d, (po.GX, po.GY)))
    msg = b"audited message " * 9
    sig = po.marshal_ecdsa_signature(*po.sign_raw(d, hashlib.sha256(msg).digest(), 0xABCDEF))
    assert csp.verify(keys[0], sigs[0], digs[0]) is True and csp.verify_coalesced(keys[1], sigs[1], digs[1]) is True
    assert csp.identity_verify_batch([pk, pk], [msg, msg + b"!"], [sig, sig]) == [None, "The signature is invalid"]
    assert csp.identity_verify_coalesced(pk, msg, sig) is None
    st = csp.audit_stats()
    assert st["direct_audits"] == 64 + 4 and st["mismatches"] == 0 and csp.poisoned() is None
    csp.close()


@pytest.mark.gpu
def test_poison_is_shared_by_the_pool():
    csp, tuples = _seeded(devices=[0, 0], audit_permille=1000)
    assert csp.device_count() == 2
    assert fabgpu.memo_corrupt(csp, SEQ, 0, 1) == 0
    assert fabgpu.hash_lookup(csp, tuples[1][0]) is None and "digest" in csp.poisoned()
    served = csp.passes_per_device()
    for seq in (SEQ + 1, SEQ + 2):                                           # whichever context the next passes would go to
        with pytest.raises(fabgpu.PoisonedError):
            fabgpu.preverify_block2(csp, clean(), block_seq=seq, seed_memo=True)
    assert csp.passes_per_device() == served                                 # refused before anything was routed or launched
    csp.close()


@pytest.mark.gpu
def test_threads_all_see_the_poison():
    csp, tuples = _seeded(audit_permille=1000)
    k = fabgpu.ECDSAPublicKey(int.from_bytes(tuples[0][1], "big"), int.from_bytes(tuples[0][2], "big"))
    start, met = threading.Barrier(8), threading.Event()
    after, reasons, errors = [[] for _ in range(8)], [], []

    def worker(w):
        try:
            start.wait()
            rounds_after = 0
            for rnd in range(100000):                                        # (ends five rounds after the poison; the bound is a safety net)
                if w == 0 and rnd == 3:
                    assert fabgpu.memo_corrupt(csp, SEQ, 0, 1) == 0
                    assert fabgpu.hash_lookup(csp, tuples[1][0]) is None     # this thread meets the corrupted entry
                    met.set()
                seen = met.is_set()                                          # (read BEFORE the lookups: they come after the poison)
                for i in (0, 2, 3, 4):
                    msg, qx, qy, sig, status, dg = tuples[i]
                    r = (fabgpu.hash_lookup(csp, msg), fabgpu.memo_lookup(csp, qx, qy, sig, dg))
                    if seen:
                        after[w].append(r)
                    else:
                        assert r in ((dg, 0), (None, None), (dg, None), (None, 0))
                if seen:
                    with pytest.raises(fabgpu.PoisonedError):
                        csp.verify(k, tuples[0][3], tuples[0][5])
                    reasons.append(csp.poisoned())
                    rounds_after += 1
                    if rounds_after == 5:
                        return
            raise AssertionError("the poison was never seen")
        except BaseException as e:                                           # noqa: BLE001 - reported by the main thread
            errors.append(repr(e))
            met.set()

    th = [threading.Thread(target=worker, args=(w,)) for w in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert all(len(a) == 20 and all(r == (None, None) for r in a) for a in after)
    assert len(set(reasons)) == 1 and "digest" in reasons[0]
    assert csp.audit_stats()["mismatches"] == 1
    csp.close()
