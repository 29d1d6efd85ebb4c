"""The P-384 stage of the block pass on the GPU (option p384): both routes, forced as tests/test_device_walk.py forces them, against
p384_ref + hashlib + the flag fold restated in tests/p384_blocks.py."""
import random

import numpy as np
import pytest

import blockbuilder as bb
import blockgen
import fabgpu
import p384_blocks as pb
import p384_ref as ref

pytestmark = pytest.mark.gpu

ZERO_STATS = dict.fromkeys(fabgpu.P384_PASS_STATS, 0)


class P256Signer:
    def __init__(self, ident, d32, sign):
        self.ident, self.d32, self._sign = ident, d32, sign

    def sign(self, msg):
        return self._sign(self.d32, msg)


class Fixed:
    """an identity that signs nothing itself: the signature bytes are given"""
    def __init__(self, ident, sig=b"\x30\x06\x02\x01\x01\x02\x01\x01"):
        self.ident, self._sig = ident, sig

    def sign(self, msg):
        return self._sig


@pytest.fixture(scope="module")
def small():
    """the 8-transaction block, and what every tuple and transaction of it must come back as with the option on and off"""
    rnd = random.Random(8384)
    s = pb.signers(4, 8384)                                  # 0 creator, 1..3 endorsers
    fx = blockgen.fixture_signers()
    sign256 = blockgen.make_signer(5)
    p256 = P256Signer(fx[0][0], fx[0][1], sign256)
    offc = Fixed(pb.off_curve_identity(99))
    envs, tuples = [], []

    def add(creator, endorsers, **kw):
        env, tu = pb.endorser_tx(rnd, creator, endorsers, **kw)
        envs.append(env)
        tuples.append(tu)
    add(s[0], [s[1], s[2]])                                                                              # 0: all valid
    add(s[0], [s[2], s[3], offc])                                                                        # 1: all valid - and, third, the endorser whose key is off the curve
    add(s[0], [s[1], s[2]], end_sig=lambda j, m, sig: s[1].sign(m[:-1] + bytes([m[-1] ^ 1])) if j == 0 else sig)   # 2: one flipped message bit
    add(s[0], [s[1], s[2]], creator_sig=lambda m, sig: (lambda r, t: ref.der_sig(r, ref.N - t))(*pb.parse_der_sig(sig)))   # 3: creator high S
    add(s[0], [s[1], s[2]], end_sig=lambda j, m, sig: sig[:-3] if j == 1 else sig)                      # 4: bad DER
    add(s[0], [s[1], s[2]], end_sig=lambda j, m, sig: ref.der_sig(ref.N + 5, pb.parse_der_sig(sig)[1]) if j == 0 else sig)   # 5: r >= n
    add(s[0], [s[1], s[2]], end_sig=lambda j, m, sig: b"" if j == 1 else sig)                           # 6: empty signature
    add(s[0], [p256, s[3]])                                                                              # 7: a P-256 endorser beside a P-384 one
    blk = bb.block(7, envs)
    tx, kind, on, off = [], [], [], []
    for t, tu in enumerate(tuples):
        for k, who, msg, sig in tu:
            tx.append(t)
            kind.append(k)
            if isinstance(who, pb.Signer):
                on.append(pb.tuple_status(who.q, msg, sig))
                off.append(pb.TUPLE_ST_NEEDS_SW)
            elif who is p256:
                on.append(0); off.append(0)
            else:
                on.append(pb.TUPLE_ST_NEEDS_SW); off.append(pb.TUPLE_ST_NEEDS_SW)
    und = [1] * 8
    return dict(block=blk, tx=tx, kind=kind, on=on, off=off, flags_on=pb.fold_flags(8, und, tx, kind, on), flags_off=pb.fold_flags(8, und, tx, kind, off), signers=s)


def test_the_small_block_is_what_the_issue_asks_for(small):
    assert small["flags_on"] == [pb.TX_VALID, pb.TX_NEEDS_SW, pb.TX_BAD_ENDORSEMENT, pb.TX_BAD_CREATOR, pb.TX_BAD_ENDORSEMENT, pb.TX_BAD_ENDORSEMENT,
                                 pb.TX_BAD_ENDORSEMENT, pb.TX_VALID]
    assert small["flags_off"] == [pb.TX_NEEDS_SW] * 8
    assert set(small["on"]) == {0, 1, 2, 3, 5, 6, 7}


def _run(csp, blk, device, seq, **kw):
    csp.set_option("pass_stage_min_bytes", 1 if device else 1 << 40)
    before = fabgpu.pass_routes(csp)
    out = fabgpu.preverify_block2(csp, blk, block_seq=seq, **kw)
    after = fabgpu.pass_routes(csp)
    assert after["device_walks"] - before["device_walks"] == (1 if device else 0), after
    return out


def _check_small(out, small, which):
    assert out["tuple_tx"].tolist() == small["tx"] and out["tuple_kind"].tolist() == small["kind"]
    assert out["tuple_status"].tolist() == small[which]
    assert out["tx_flags"].tolist() == small["flags_" + which]


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_small_block_option_on(small, device):
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        _run(csp, small["block"], False, 1)                  # (the host route meets the identities; the device route serves those it knows)
        base = csp.p384_pass_stats()
        out = _run(csp, small["block"], device, 2)
        _check_small(out, small, "on")
        st = csp.p384_pass_stats()
        pairs = list(zip(small["on"], small["off"]))
        n384 = sum(1 for a, b in pairs if b == pb.TUPLE_ST_NEEDS_SW and a != pb.TUPLE_ST_NEEDS_SW)     # every tuple of a P-384 signer; not the off-curve endorser's
        n_sub = sum(1 for a, b in pairs if b == pb.TUPLE_ST_NEEDS_SW and a in (0, 1, 3))                # ... of which the host gate lets these through
        assert st["stages"] - base["stages"] == 1 and st["seen"] - base["seen"] == n384
        assert st["submitted"] - base["submitted"] == n_sub and st["fresh_launches"] - base["fresh_launches"] == 1
        assert st["keyed_launches"] == 0 and st["audited"] == 0
        # P-384 tuples enter no memo: not hashed, no key, no digest
        sw_rows = [i for i, v in enumerate(small["off"]) if v == pb.TUPLE_ST_NEEDS_SW]
        assert not out["tuple_hashed"][sw_rows].any() and not out["tuple_qxy"][sw_rows].any() and not out["tuple_digest"][sw_rows].any()
        # the lean form (no tuple records come back from the device: the stage walks the block itself) gives the same flags
        lean = _run(csp, small["block"], device, 3, lean=True)
        assert lean["tx_flags"].tolist() == small["flags_on"]
    finally:
        csp.close()


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_small_block_option_off_is_todays_answer(small, device):
    csp = fabgpu.GPUCSP(device=0)
    try:
        _run(csp, small["block"], False, 1)
        out = _run(csp, small["block"], device, 2)
        _check_small(out, small, "off")
        assert csp.p384_pass_stats() == ZERO_STATS
    finally:
        csp.close()


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_all_p256_block_is_untouched_by_the_option(device):
    blk, _ = blockgen.endorser_block(40, seed=3)
    outs = []
    for p384 in (0, 1):
        csp = fabgpu.GPUCSP(device=0, p384=p384)
        try:
            _run(csp, blk, False, 1)
            outs.append(_run(csp, blk, device, 2))
            assert csp.p384_pass_stats() == ZERO_STATS
        finally:
            csp.close()
    for k in ("tx_flags", "tx_type", "tuple_tx", "tuple_kind", "tuple_status", "tuple_spans", "tuple_digest", "tuple_hashed", "tuple_qxy"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert (outs[1]["tx_flags"] == 0).all()


def _off_by_one(sig: bytes) -> bytes:
    """the same signature with s one lower (still low-S): an arithmetic reject"""
    r, s = pb.parse_der_sig(sig)
    return ref.der_sig(r, s - 1 if s > 1 else s + 1)


@pytest.fixture(scope="module")
def big():
    """100 transactions, a P-256 creator and three P-384 endorsers each: 300 P-384 tuples, a partial last wavefront.  Ten distinct
    transactions (30 signatures from p384_ref.sign) are laid out over the block - the same bytes at other offsets - and ten seeded
    transactions are made afresh with one endorsement's s changed.  p384_ref.status decides every DISTINCT tuple (the ten base
    transactions' and the corrupted transactions'); a copy has its original's status."""
    rnd = random.Random(100384)
    s = pb.signers(5, 100384)
    fx = blockgen.fixture_signers()
    creator = P256Signer(fx[4][0], fx[4][1], blockgen.make_signer(9))
    made = {t: pb.endorser_tx(rnd, creator, rnd.sample(s, 3)) for t in range(10)}
    corrupt = sorted(rnd.sample(range(10, 100), 10))
    for t in corrupt:
        j = rnd.randrange(3)
        made[t] = pb.endorser_tx(rnd, creator, rnd.sample(s, 3), end_sig=lambda jj, m, sig, j=j: _off_by_one(sig) if jj == j else sig)
    status_of = {t: [0 if who is creator else pb.tuple_status(who.q, msg, sig) for _, who, msg, sig in tu] for t, (_, tu) in made.items()}
    envs, tx, kind, want = [], [], [], []
    for t in range(100):
        src = t if t in made else t % 10
        env, tu = made[src]
        envs.append(env)
        for (k, _, _, _), st in zip(tu, status_of[src]):
            tx.append(t)
            kind.append(k)
            want.append(st)
    flags = pb.fold_flags(100, [1] * 100, tx, kind, want)
    assert sorted(t for t in range(100) if flags[t] == pb.TX_BAD_ENDORSEMENT) == corrupt and want.count(1) == 10 and want.count(0) == 390
    return dict(block=bb.block(11, envs), tx=tx, kind=kind, want=want, flags=flags, signers=s)


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_hundred_transactions_fresh_then_keyed(big, device):
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        _run(csp, big["block"], False, 1)
        base = csp.p384_pass_stats()
        fresh = _run(csp, big["block"], device, 2)
        assert fresh["tuple_status"].tolist() == big["want"] and fresh["tx_flags"].tolist() == big["flags"]
        st = csp.p384_pass_stats()
        assert (st["fresh_launches"] - base["fresh_launches"], st["keyed_launches"], st["submitted"] - base["submitted"]) == (1, 0, 300)
        for sg in big["signers"]:
            csp.key_import_p384(sg.q)
        assert csp.p384_key_table_stats()["live"] == len(big["signers"])
        keyed = _run(csp, big["block"], device, 3)
        st2 = csp.p384_pass_stats()
        assert (st2["fresh_launches"] - st["fresh_launches"], st2["keyed_launches"], st2["submitted"] - st["submitted"]) == (0, 1, 300)
        assert keyed["tuple_status"].tolist() == big["want"] and keyed["tx_flags"].tolist() == big["flags"]
    finally:
        csp.close()


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_audit_catches_a_corrupted_verdict_and_poisons(small, device):
    csp = fabgpu.GPUCSP(device=0, p384=1, audit_permille=1000)
    try:
        _run(csp, small["block"], False, 1)                  # every "valid" audited, all agree
        n_valid = sum(1 for a, b in zip(small["on"], small["off"]) if a == 0 and b == pb.TUPLE_ST_NEEDS_SW)
        assert csp.p384_pass_stats()["audited"] == n_valid and csp.poisoned() is None
        fabgpu.p384_corrupt(csp, 1)                          # the next arithmetic reject (transaction 2's endorsement) is read as "valid"
        with pytest.raises(fabgpu.PoisonedError):
            _run(csp, small["block"], device, 2)
        assert "P-384" in csp.poisoned()
        with pytest.raises(fabgpu.PoisonedError):            # the next pass answers as a poisoned provider does
            fabgpu.preverify_block2(csp, small["block"], block_seq=3)
    finally:
        csp.close()
