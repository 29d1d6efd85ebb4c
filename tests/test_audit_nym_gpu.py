"""The provider audits idemix pseudonym verdicts on the CPU and retires itself on a mismatch (include/fabgpu_bccsp.h "CPU audit";
DESIGN.md 4.4e addendum).  The feature has no kernel of its own: the values come from the existing idemix kernels and the block pass,
and these tests check that the provider re-verifies them (fabric-mod_amd/csrc/audit_host.h audit_nym_verify), counts what it did, and
reacts to a wrong one.  Wrong values are made by the test hook fabgpu_csp_test_memo_corrupt, which edits host memory of the library:
nothing is launched, nothing faults.

The block: 8 transactions x (creator + 2 endorsements) = 24 tuples; transactions 0, 2, 4, 6 have idemix creators of IdemixMSP1 (tuples
0, 6, 12, 18), and the creator of transaction 4 signed another payload (status 1, proof invalid)."""
import functools
import hashlib
import json
import os
import random

import numpy as np
import pytest

import blockbuilder as bb
import blockgen
import fabgpu
import idemix_oracle as io
from idemix_common import be32, fixtures

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ = 11
MSP = "MSP1OU1"
NYM_TUPLES = (0, 6, 12, 18)
BAD_TUPLE = 12
COUNTERS = ("digest_audits", "verdict_audits", "direct_audits", "mismatches", "skipped_nym", "audit_ns", "nym_audits")


def _raw_ipk():
    return bytes.fromhex(json.load(open(os.path.join(ROOT, "tests", "golden", "idemix_fixtures.json")))["msps"][MSP]["ipk"])


@functools.lru_cache(maxsize=None)
def _block():
    fx = blockgen.fixture_signers()
    ipk, sk = fixtures()[MSP]["ipk"], fixtures()[MSP]["signer"].sk
    rng = np.random.default_rng(1201)
    prng = random.Random(1202)
    sign = blockgen.make_signer(1203)
    envs = []
    for t in range(8):
        ends = [fx[(t + j) % 4] for j in range(2)]
        if t % 2:
            envs.append(blockgen.endorser_tx(t, rng, fx[4 + (t // 2) % 2], ends, sign))
            continue
        nym, r_nym = io.make_nym(sk, ipk, prng)
        creator = bb.serialized_idemix_identity("IdemixMSP1", be32(nym[0]), be32(nym[1]))
        payload, _ = bb.consistent_endorser_tx("mychannel", creator, bytes(rng.integers(0, 256, size=24, dtype=np.uint8)),
                                               bytes(rng.integers(0, 256, size=300, dtype=np.uint8)), bytes(rng.integers(0, 256, size=990, dtype=np.uint8)),
                                               lambda prp: [(eid, sign(ed, prp + eid)) for eid, ed in ends])
        sig = io.nym_sign(sk, nym, r_nym, ipk, payload + (b"!" if t == 4 else b""), prng)
        envs.append(bb.envelope(payload, io.nym_signature_marshal(sig)))
    return bb.block(SEQ, envs)


def _pass(csp, seq=SEQ):
    """the memo-seeding pass -> per tuple (message, key or pseudonym X, Y, signature bytes, status, device digest)"""
    out = fabgpu.preverify_block2(csp, _block(), block_seq=seq, seed_memo=True)
    assert out["memo_seeded"] == len(out["tuple_status"]) == 24                # every tuple has an entry: entry index = tuple index
    tuples = []
    for i in range(24):
        sp = [int(x) for x in out["tuple_spans"][i]]
        msg = out["arena"][sp[2]:sp[2] + sp[3]] + out["arena"][sp[4]:sp[4] + sp[5]]
        q = bytes(out["tuple_qxy"][i])
        tuples.append((msg, q[:32], q[32:], out["arena"][sp[6]:sp[6] + sp[7]], int(out["tuple_status"][i]), bytes(out["tuple_digest"][i])))
    assert [t[4] for t in tuples] == [1 if i == BAD_TUPLE else 0 for i in range(24)]
    assert all(t[5] == hashlib.sha256(t[0]).digest() for t in tuples)
    return tuples


def _seeded(**kw):
    csp = fabgpu.GPUCSP(device=0, devices=[0], **kw)
    assert csp.idemix_msp_register("IdemixMSP1", _raw_ipk()) >= 0
    fabgpu.preverify_block(csp, _block())                                      # first sight: the identities are learned
    return csp, _pass(csp)


def _nym_lookup(csp, t):
    msg, nx, ny, sig, _, dg = t
    return fabgpu.memo_lookup_nym(csp, bytes(fixtures()[MSP]["ipk"].hash), nx, ny, sig, dg)


def _assert_retired(csp, tuples):
    """a poisoned provider: every lookup misses, every later entry point answers FABGPU_EPOISONED"""
    assert all(_nym_lookup(csp, tuples[i]) is None for i in NYM_TUPLES)
    msg, qx, qy, sig, _, dg = tuples[1]
    assert fabgpu.memo_lookup(csp, qx, qy, sig, dg) is None and fabgpu.hash_lookup(csp, msg) is None
    k = fabgpu.ECDSAPublicKey(int.from_bytes(qx, "big"), int.from_bytes(qy, "big"))
    for call in (lambda: csp.verify(k, sig, dg), lambda: csp.verify_batch([k], [sig], [dg]), lambda: csp.identity_verify_batch([k], [msg], [sig]),
                 lambda: csp.idemix_nym_verify_batch(0, [tuples[0][1] + tuples[0][2]], [tuples[0][3]], [tuples[0][0]]),
                 lambda: fabgpu.preverify_block(csp, _block()), lambda: fabgpu.preverify_block2(csp, _block(), block_seq=SEQ + 5, seed_memo=True)):
        with pytest.raises(fabgpu.PoisonedError):
            call()
    assert fabgpu.memo_has_block(csp, SEQ + 5) == 0


# ---- 5. / 10. the batch entry point ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch():
    """65 pseudonym signatures - one full wavefront and one lane of the next: 33 valid ones, and a tampered twin behind each of the first
    32 -> (nym keys, signatures, messages, the oracle's status for each)"""
    ipk, sk = fixtures()[MSP]["ipk"], fixtures()[MSP]["signer"].sk
    rng = random.Random(1301)
    rows = []
    for i in range(33):
        nym, r_nym = io.make_nym(sk, ipk, rng)
        msg = bytes(rng.getrandbits(8) for _ in range((0, 1, 26, 27, 90, 91, 500)[i % 7] + i))
        sig = io.nym_sign(sk, nym, r_nym, ipk, msg, rng)
        rows.append((nym, sig, msg))
        if i == 32:
            break
        kind = i % 6
        if kind == 0:                                        # one bit of the message
            rows.append((nym, sig, msg[:-1] + bytes([msg[-1] ^ 0x10]) if msg else b"\x01"))
        elif kind in (1, 2, 3):                              # one bit of a signature field
            f = ("proof_c", "proof_s_sk", "nonce")[kind - 1]
            v = bytearray(sig[f])
            v[1 + i % 31] ^= 1 << (i % 8)
            rows.append((nym, dict(sig, **{f: bytes(v)}), msg))
        elif kind == 4:                                      # somebody else's pseudonym
            rows.append((io.make_nym(sk, ipk, rng)[0], sig, msg))
        else:                                                # an s-value outside the domain the device decides: left to bccsp/idemix
            rows.append((nym, dict(sig, proof_s_r_nym=be32(io.R + 7 + i)), msg))
    assert len(rows) == 65
    keys = [be32(n[0]) + be32(n[1]) for n, _, _ in rows]
    return keys, [io.nym_signature_marshal(s) for _, s, _ in rows], [m for _, _, m in rows], [io.nym_verify(s, n, ipk, m) for n, s, m in rows]


def _run_batch(csp):
    keys, sigs, msgs, want = _batch()
    iid = csp.idemix_issuer_import(_raw_ipk())
    assert iid >= 0
    got = csp.idemix_nym_verify_batch(iid, keys, sigs, msgs)
    assert [g[0] for g in got] == [w == io.NYM_VALID for w in want]
    assert [g[1] for g in got] == [w == io.NYM_NEEDS_SW for w in want]
    assert all((g[2] == "pseudonym signature invalid: zero-knowledge proof is invalid") == (w == io.NYM_BAD_PROOF) for g, w in zip(got, want))
    assert want.count(io.NYM_VALID) == 33 and want.count(io.NYM_NEEDS_SW) >= 5 and want.count(io.NYM_BAD_PROOF) >= 20
    return want.count(io.NYM_VALID)


def test_batch_of_65_fully_audited_is_clean():
    csp = fabgpu.GPUCSP(device=0, devices=[0], audit_permille=1000)
    n_valid = _run_batch(csp)
    st = csp.audit_stats()
    assert tuple(st) == COUNTERS
    assert st["nym_audits"] == n_valid == 33 and st["mismatches"] == 0 and st["skipped_nym"] == 0 and st["audit_ns"] > 0
    assert csp.poisoned() is None
    # every fourth "valid" at 250 permille: 33 more hits of the same counter -> 8 more audits
    assert csp.set_option("audit_permille", 250) == 1000
    _run_batch(csp)
    assert csp.audit_stats()["nym_audits"] == 33 + 8 and csp.poisoned() is None
    csp.close()


# ---- 6. the pass and the memo, clean ---------------------------------------------------------------------------------------------------------
def test_pass_and_memo_fully_audited_is_clean():
    plain, tuples0 = _seeded()
    want = [_nym_lookup(plain, tuples0[i]) for i in NYM_TUPLES]
    assert want == [0, 0, 1, 0]
    plain.close()
    csp, tuples = _seeded(audit_permille=1000)
    assert tuples == tuples0
    assert [_nym_lookup(csp, tuples[i]) for i in NYM_TUPLES] == want         # answers as the unaudited provider does
    st = csp.audit_stats()
    assert st["nym_audits"] == 4 and st["mismatches"] == 0 and st["skipped_nym"] == 0 and st["verdict_audits"] == 0 and csp.poisoned() is None
    # a lookup that misses (another digest, another issuer) is no hit and no audit
    msg, nx, ny, sig, _, dg = tuples[0]
    assert fabgpu.memo_lookup_nym(csp, bytes(fixtures()[MSP]["ipk"].hash), nx, ny, sig, hashlib.sha256(msg + b"!").digest()) is None
    assert fabgpu.memo_lookup_nym(csp, bytes(fixtures()["MSP2OU1"]["ipk"].hash), nx, ny, sig, dg) is None
    assert csp.audit_stats()["nym_audits"] == 4
    # the P-256 entries of the same table go through their own kind
    for i in (1, 2, 3):
        msg, qx, qy, sig, _, dg = tuples[i]
        assert fabgpu.memo_lookup(csp, qx, qy, sig, dg) == 0
    st = csp.audit_stats()
    assert st["verdict_audits"] == 3 and st["nym_audits"] == 4 and st["mismatches"] == 0 and csp.poisoned() is None
    csp.close()


# ---- 7. a stored status that is wrong --------------------------------------------------------------------------------------------------------
def test_corrupted_pseudonym_status_poisons():
    csp, tuples = _seeded(audit_permille=1000)
    assert fabgpu.memo_corrupt(csp, SEQ, 1, BAD_TUPLE) == 0                  # invalid -> valid, in the library's host memory
    assert _nym_lookup(csp, tuples[0]) == 0 and _nym_lookup(csp, tuples[6]) == 0 and csp.poisoned() is None
    assert _nym_lookup(csp, tuples[BAD_TUPLE]) is None                        # a miss: the caller verifies for itself
    why = csp.poisoned()
    assert why is not None and why.startswith("pseudonym audit") and "entry %d" % BAD_TUPLE in why and "holds status 0" in why and "says invalid" in why
    st = csp.audit_stats()
    assert st["mismatches"] == 1 and st["nym_audits"] == 3 and st["skipped_nym"] == 0
    _assert_retired(csp, tuples)
    assert csp.poisoned() == why                                              # the first reason stays
    csp.close()


def test_corrupted_pseudonym_status_goes_unnoticed_without_the_switch():
    csp, tuples = _seeded()
    assert fabgpu.memo_corrupt(csp, SEQ, 1, BAD_TUPLE) == 0 and fabgpu.memo_corrupt(csp, SEQ, 2, 0) == 0
    assert _nym_lookup(csp, tuples[BAD_TUPLE]) == 0 and _nym_lookup(csp, tuples[0]) == 0     # the toggled status, handed out
    assert csp.poisoned() is None and sum(csp.audit_stats().values()) == 0
    csp.close()


# ---- 8. a held message byte that is wrong ----------------------------------------------------------------------------------------------------
def test_corrupted_held_message_byte_poisons_through_the_digest_check():
    csp, tuples = _seeded(audit_permille=1000)
    assert fabgpu.memo_corrupt(csp, SEQ, 2, 18) == 0
    assert _nym_lookup(csp, tuples[6]) == 0 and csp.poisoned() is None
    assert _nym_lookup(csp, tuples[18]) is None
    why = csp.poisoned()
    assert why is not None and why.startswith("pseudonym audit") and "entry 18" in why and "holds digest " + tuples[18][5][:8].hex() in why
    st = csp.audit_stats()
    assert st["mismatches"] == 1 and st["nym_audits"] == 2
    _assert_retired(csp, tuples)
    csp.close()


# ---- 9. a hit that cannot be audited ---------------------------------------------------------------------------------------------------------
def test_hit_without_a_held_block_copy_is_answered_and_counted():
    """hash_memo_blocks = 1: the second block seeded finds the copy pool exhausted - its verdict entries stand, its messages are not held"""
    csp, tuples = _seeded(audit_permille=1000, hash_memo_blocks=1)
    assert _pass(csp, seq=SEQ + 1) == tuples
    hm = fabgpu.hash_memo_stats(csp)
    assert hm["blocks_held"] == 1 and hm["refused"] == 1
    assert fabgpu.memo_has_block(csp, SEQ) == 24 == fabgpu.memo_has_block(csp, SEQ + 1)
    assert _nym_lookup(csp, tuples[6]) == 0                                   # the newest table answers: as today
    st = csp.audit_stats()
    assert st["skipped_nym"] == 1 and st["nym_audits"] == 0 and st["mismatches"] == 0 and csp.poisoned() is None
    assert _nym_lookup(csp, tuples[BAD_TUPLE]) == 1
    assert csp.audit_stats()["skipped_nym"] == 2
    # ... and once that table is gone the same question meets the block whose copy is held: audited
    assert fabgpu.memo_evict_block(csp, SEQ + 1) == 24
    assert _nym_lookup(csp, tuples[6]) == 0
    st = csp.audit_stats()
    assert st["skipped_nym"] == 2 and st["nym_audits"] == 1 and st["mismatches"] == 0 and csp.poisoned() is None
    csp.close()


# ---- 10. off by default ----------------------------------------------------------------------------------------------------------------------
def test_off_by_default_counts_nothing():
    csp, tuples = _seeded()
    assert csp.get_option("audit_permille") == 0
    _run_batch(csp)
    assert [_nym_lookup(csp, tuples[i]) for i in NYM_TUPLES] == [0, 0, 1, 0]
    st = csp.audit_stats()
    assert tuple(st) == COUNTERS and all(v == 0 for v in st.values()) and csp.poisoned() is None
    csp.close()
