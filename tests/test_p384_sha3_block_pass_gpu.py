"""The P-384 stage of the block pass with an MSP of the SHA3 hash family, on the GPU: fabgpu_csp_msp_hash_family tells the pass the
family, the stage splits its rows and hashes the SHA3 MSP's P-384 tuples with SHA3-256.  Both routes, forced as
tests/test_p384_block_pass_gpu.py forces them, against p384_ref + hashlib + the flag fold restated in tests/p384_blocks.py.

The block: three transactions, P-384 creators of Org1MSP (SHA2), P-384 endorsers of Org3MSP (SHA3, signing over SHA3-256) - one of
their endorsements forged - and one P-256 endorser of Org3MSP (signing over SHA3-256 too; the routes hash P-256 messages with SHA-256
whatever the MSP, so its tuple is "not valid" with and without the registry entry and bccsp/sw decides it)."""
import hashlib
import random

import pytest

import blockbuilder as bb
import fabgpu
import p384_blocks as pb
import p384_ref as ref
import p384_sha3_blocks as pb3

pytestmark = pytest.mark.gpu

SHA3_MSP = "Org3MSP"


@pytest.fixture(scope="module")
def blk():
    rnd = random.Random(3384)
    creator = pb3.Signer(rnd, "client.org1.example.com", "Org1MSP", sha3=False)
    e1 = pb3.Signer(rnd, "peer0.org3.example.com", SHA3_MSP, sha3=True)
    e2 = pb3.Signer(rnd, "peer1.org3.example.com", SHA3_MSP, sha3=True)
    p256 = pb3.P256Sha3Signer(0, SHA3_MSP, seed=11)
    envs, tuples = [], []

    def add(endorsers, **kw):
        env, tu = pb.endorser_tx(rnd, creator, endorsers, **kw)
        envs.append(env)
        tuples.append(tu)
    add([e1, e2])                                                                                        # 0: all genuine
    add([e1, e2], end_sig=lambda j, m, sig: e1.sign(m[:-1] + bytes([m[-1] ^ 1])) if j == 0 else sig)     # 1: e1's endorsement forged (signed over another message)
    add([e2, p256])                                                                                      # 2: the P-256 endorser of the SHA3 MSP
    tx, kind, who_, unset, set_ = [], [], [], [], []
    for t, tu in enumerate(tuples):
        for k, who, msg, sig in tu:
            tx.append(t)
            kind.append(k)
            who_.append((who, msg, sig))
            if who is p256:
                unset.append(1); set_.append(1)              # SHA-256 of the message is not what was signed: an arithmetic reject either way
            else:
                unset.append(pb3.tuple_status(who.q, msg, sig, False))
                set_.append(pb3.tuple_status(who.q, msg, sig, who.sha3))
    und = [1] * 3
    return dict(block=bb.block(9, envs), tx=tx, kind=kind, tuples=who_, unset=unset, set=set_, flags_unset=pb.fold_flags(3, und, tx, kind, unset),
                flags_set=pb.fold_flags(3, und, tx, kind, set_), creator=creator, e=[e1, e2], p256=p256)


def test_the_block_is_what_the_issue_asks_for(blk):
    sha3_rows = [i for i, (who, _, _) in enumerate(blk["tuples"]) if getattr(who, "sha3", False)]
    assert len(sha3_rows) == 5
    assert [blk["unset"][i] for i in sha3_rows] == [1] * 5   # without the entry every SHA3 tuple is "not valid": the parent's answer
    assert [blk["set"][i] for i in sha3_rows] == [0, 0, 1, 0, 0]
    assert blk["flags_unset"] == [pb.TX_BAD_ENDORSEMENT] * 3
    assert blk["flags_set"] == [pb.TX_VALID, pb.TX_BAD_ENDORSEMENT, pb.TX_BAD_ENDORSEMENT]
    assert [blk["set"][i] for i, (who, _, _) in enumerate(blk["tuples"]) if who is blk["creator"]] == [0, 0, 0]


def _run(csp, block, device, seq, **kw):
    csp.set_option("pass_stage_min_bytes", 1 if device else 1 << 40)
    before = fabgpu.pass_routes(csp)
    out = fabgpu.preverify_block2(csp, block, block_seq=seq, **kw)
    after = fabgpu.pass_routes(csp)
    assert after["device_walks"] - before["device_walks"] == (1 if device else 0), after
    return out


def _check(out, blk, which):
    assert out["tuple_tx"].tolist() == blk["tx"] and out["tuple_kind"].tolist() == blk["kind"]
    assert out["tuple_status"].tolist() == blk[which]
    assert out["tx_flags"].tolist() == blk["flags_" + which]


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def test_the_registry_through_the_provider():
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        assert csp.msp_hash_family_get(SHA3_MSP) == "SHA2"
        with pytest.raises(fabgpu.BCCSPError, match="SHA3 is served by bccsp/sw, not by the GPU provider"):
            csp.msp_hash_family(SHA3_MSP, "SHA3")            # the hash_sha3 option is off
        with pytest.raises(fabgpu.BCCSPError, match=r"hash familiy not recognized \[SHA4\]"):
            csp.msp_hash_family(SHA3_MSP, "SHA4")
        csp.msp_hash_family(SHA3_MSP, "SHA2")
        csp.set_option("hash_sha3", 1)
        csp.msp_hash_family(SHA3_MSP, "SHA3")
        assert csp.msp_hash_family_get(SHA3_MSP) == "SHA3" and csp.msp_hash_family_get("Org1MSP") == "SHA2"
        csp.msp_hash_family(SHA3_MSP, "SHA2")
        assert csp.msp_hash_family_get(SHA3_MSP) == "SHA2"
        # a caller of the seven-value form gets the seven it always got; the count is eight now
        import ctypes
        v = (ctypes.c_uint64 * 9)(*([77] * 9))
        assert csp._L.fabgpu_csp_p384_pass_stats(csp._h, v, 7) == 8 and list(v)[:7] == [0] * 7 and list(v)[7:] == [77, 77]
        assert csp._L.fabgpu_csp_p384_pass_stats(csp._h, v, 9) == 8 and list(v) == [0] * 8 + [77]
    finally:
        csp.close()


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_without_a_registry_entry_the_pass_answers_as_before(blk, device):
    csp = fabgpu.GPUCSP(device=0, p384=1, hash_sha3=1)
    try:
        csp.msp_hash_family("SomeOtherMSP", "SHA3")          # (an entry for an MSP the block does not name changes nothing)
        _run(csp, blk["block"], False, 1)
        base = csp.p384_pass_stats()
        out = _run(csp, blk["block"], device, 2)
        _check(out, blk, "unset")
        d = _delta(base, csp.p384_pass_stats())
        assert (d["submitted"], d["fresh_launches"], d["keyed_launches"], d["sha3_rows"]) == (8, 1, 0, 0)
    finally:
        csp.close()


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_registered_sha3_fresh_mixed_and_keyed(blk, device):
    csp = fabgpu.GPUCSP(device=0, p384=1, hash_sha3=1)
    try:
        csp.msp_hash_family(SHA3_MSP, "SHA3")
        _run(csp, blk["block"], False, 1)                    # (the host route meets the identities; the device route serves those it knows)
        base = csp.p384_pass_stats()
        out = _run(csp, blk["block"], device, 2)
        _check(out, blk, "set")
        d = _delta(base, csp.p384_pass_stats())
        assert (d["stages"], d["seen"], d["submitted"], d["sha3_rows"]) == (1, 8, 8, 5)
        assert (d["fresh_launches"], d["keyed_launches"]) == (2, 0)          # two batches: the creators' and the SHA3 endorsers'
        # only the creator's key registered: its batch goes keyed, the SHA3 batch stays fresh
        csp.key_import_p384(blk["creator"].q)
        mid = csp.p384_pass_stats()
        _check(_run(csp, blk["block"], device, 3), blk, "set")
        d = _delta(mid, csp.p384_pass_stats())
        assert (d["fresh_launches"], d["keyed_launches"], d["sha3_rows"]) == (1, 1, 5)
        for e in blk["e"]:
            csp.key_import_p384(e.q)
        mid = csp.p384_pass_stats()
        _check(_run(csp, blk["block"], device, 4), blk, "set")
        d = _delta(mid, csp.p384_pass_stats())
        assert (d["fresh_launches"], d["keyed_launches"], d["sha3_rows"]) == (0, 2, 5)
        # the lean form (the stage walks the block itself) gives the same flags
        assert _run(csp, blk["block"], device, 5, lean=True)["tx_flags"].tolist() == blk["flags_set"]
        # set back to SHA2, for the passes that start now: the earlier answer
        csp.msp_hash_family(SHA3_MSP, "SHA2")
        _check(_run(csp, blk["block"], device, 6), blk, "unset")
        # set SHA3 with the hash_sha3 option switched off afterwards: the MSP counts as SHA2 while it is off
        csp.msp_hash_family(SHA3_MSP, "SHA3")
        csp.set_option("hash_sha3", 0)
        _check(_run(csp, blk["block"], device, 7), blk, "unset")
    finally:
        csp.close()


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_every_valid_sha3_row_is_audited_without_poisoning(blk, device):
    csp = fabgpu.GPUCSP(device=0, p384=1, hash_sha3=1, audit_permille=1000)
    try:
        csp.msp_hash_family(SHA3_MSP, "SHA3")
        _run(csp, blk["block"], False, 1)
        base = csp.p384_pass_stats()
        _check(_run(csp, blk["block"], device, 2), blk, "set")
        n_valid = sum(1 for (who, _, _), st in zip(blk["tuples"], blk["set"]) if st == 0 and who is not blk["p256"])
        assert n_valid == 7 and csp.p384_pass_stats()["audited"] - base["audited"] == n_valid and csp.poisoned() is None
    finally:
        csp.close()


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_seeding_keys_sha3_rows_on_the_sha3_digest(blk, device):
    csp = fabgpu.GPUCSP(device=0, p384=1, hash_sha3=1)
    try:
        csp.msp_hash_family(SHA3_MSP, "SHA3")
        _run(csp, blk["block"], False, 1)
        out = _run(csp, blk["block"], device, 21, seed_memo=True)
        _check(out, blk, "set")
        for (who, msg, sig), st in zip(blk["tuples"], blk["set"]):
            if who is blk["p256"]:
                continue
            qx, qy = ref.b48(who.q[0]), ref.b48(who.q[1])
            d2, d3 = hashlib.sha256(msg).digest(), hashlib.sha3_256(msg).digest()
            if who.sha3:                                     # what the validator's bccsp.Verify presents is the SHA3-256 digest
                assert fabgpu.memo_lookup_p384(csp, qx, qy, sig, d3) == (st, 21)
                assert fabgpu.memo_lookup_p384(csp, qx, qy, sig, d2) is None
            else:
                assert fabgpu.memo_lookup_p384(csp, qx, qy, sig, d2) == (st, 21)
                assert fabgpu.memo_lookup_p384(csp, qx, qy, sig, d3) is None
        assert csp.p384_pass_stats()["memo_seeded"] == 8 and csp.poisoned() is None
    finally:
        csp.close()


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_an_all_sha2_block_launches_what_it_launched(device):
    """P-384 creators and endorsers of Org1MSP (and one P-256 endorser, so that the device route has a signature of its own to decide)
    while another MSP is registered SHA3: one batch, no SHA3 row"""
    rnd = random.Random(2384)
    s = pb.signers(3, 2384)
    p256 = pb3.P256Sha3Signer(1, "Org1MSP", seed=12)         # (signs over SHA3-256: "not valid" to the routes)
    envs, want = [], []
    for t in range(3):
        env, tu = pb.endorser_tx(rnd, s[0], [s[1], s[2] if t < 2 else p256])
        envs.append(env)
        want += [1 if who is p256 else pb.tuple_status(who.q, msg, sig) for _, who, msg, sig in tu]
    block = bb.block(10, envs)
    csp = fabgpu.GPUCSP(device=0, p384=1, hash_sha3=1)
    try:
        csp.msp_hash_family(SHA3_MSP, "SHA3")
        _run(csp, block, False, 1)
        base = csp.p384_pass_stats()
        out = _run(csp, block, device, 2)
        assert out["tuple_status"].tolist() == want == [0] * 8 + [1] and out["tx_flags"].tolist() == [0, 0, pb.TX_BAD_ENDORSEMENT]
        d = _delta(base, csp.p384_pass_stats())
        assert (d["submitted"], d["fresh_launches"], d["keyed_launches"], d["sha3_rows"]) == (8, 1, 0, 0)
    finally:
        csp.close()
