"""The verdict memo of the P-384 tuples of a block pass on the GPU (option p384, FABGPU_PASS_SEED_MEMO): what the pass's P-384 stage
seeds, what fabgpu_csp_memo_lookup_p384 answers, lifetime, switches and audit.  Blocks from tests/p384_blocks.py; expected answers from
p384_ref + hashlib (the digest a validator computes on the CPU is the digest the entries are keyed on)."""
import hashlib
import random

import numpy as np
import pytest

import blockbuilder as bb
import blockgen
import fabgpu
import p384_blocks as pb
import p384_ref as ref

pytestmark = pytest.mark.gpu

ARRAYS = ("tx_flags", "tx_type", "tuple_tx", "tuple_kind", "tuple_status", "tuple_spans", "tuple_digest", "tuple_hashed", "tuple_qxy")


class P256Signer:
    def __init__(self, ident, d32, sign):
        self.ident, self.d32, self._sign = ident, d32, sign

    def sign(self, msg):
        return self._sign(self.d32, msg)


def _off_by_one(sig: bytes) -> bytes:
    """the same signature with s one lower (still low-S): an arithmetic reject"""
    r, s = pb.parse_der_sig(sig)
    return ref.der_sig(r, s - 1 if s > 1 else s + 1)


def _block24(seed, number):
    """8 transactions, a P-384 creator and two P-384 endorsers each: 24 tuples, three of them with a wrong s that is still low"""
    rnd = random.Random(seed)
    s = pb.signers(3, seed)
    envs, tuples = [], []
    for t in range(8):
        kw = {}
        if t == 2:
            kw["end_sig"] = lambda j, m, sig: _off_by_one(sig) if j == 0 else sig
        if t == 4:
            kw["creator_sig"] = lambda m, sig: _off_by_one(sig)
        if t == 6:
            kw["end_sig"] = lambda j, m, sig: _off_by_one(sig) if j == 1 else sig
        env, tu = pb.endorser_tx(rnd, s[0], [s[1], s[2]], **kw)
        envs.append(env)
        tuples += tu
    want = [pb.tuple_status(who.q, msg, sig) for _, who, msg, sig in tuples]
    assert len(tuples) == 24 and want.count(0) == 21 and want.count(1) == 3
    return dict(block=bb.block(number, envs), tuples=tuples, want=want, signers=s)


@pytest.fixture(scope="module")
def blk():
    return _block24(24384, 7)


@pytest.fixture(scope="module")
def blk_b():
    return _block24(24385, 8)


def _ask(csp, tu):
    """the validator's question for one P-384 tuple: bccsp.Verify(k, sig, SHA-256(msg)), the digest computed here on the CPU"""
    _, who, msg, sig = tu
    return fabgpu.memo_lookup_p384(csp, ref.b48(who.q[0]), ref.b48(who.q[1]), sig, hashlib.sha256(msg).digest())


def _pass(csp, b, seq, device=None, seed_memo=True):
    if device is not None:
        csp.set_option("pass_stage_min_bytes", 1 if device else 1 << 40)
    return fabgpu.preverify_block2(csp, b["block"], block_seq=seq, seed_memo=seed_memo)


@pytest.mark.parametrize("device", [False, True], ids=["host_route", "device_route"])
def test_seeding_keyed_form(blk, device):
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        for sg in blk["signers"]:
            csp.key_import_p384(sg.q)
        out = _pass(csp, blk, 41, device)
        assert out["tuple_status"].tolist() == blk["want"]
        st = csp.p384_pass_stats()
        assert (st["keyed_launches"], st["fresh_launches"], st["submitted"], st["memo_seeded"]) == (1, 0, 24, 24)
        assert out["memo_seeded"] == 24                       # (an all-P-384 block: nothing else to remember)
        assert [_ask(csp, tu) for tu in blk["tuples"]] == [(w, 41) for w in blk["want"]]
        assert fabgpu.memo_stats_p384(csp) == dict(entries=24, hits=24, misses=0, evicted=0)
        assert fabgpu.memo_has_block(csp, 41) == 24
        # the outputs keep their layout: not hashed, no 32-byte key, no digest for these tuples
        assert not out["tuple_hashed"].any() and not out["tuple_qxy"].any() and not out["tuple_digest"].any()
        # near the entries: another digest, another key, other signature bytes, the other framing
        _, who, msg, sig = blk["tuples"][0]
        x, y, dg = ref.b48(who.q[0]), ref.b48(who.q[1]), hashlib.sha256(msg).digest()
        assert fabgpu.memo_lookup_p384(csp, x, y, sig, hashlib.sha256(msg + b"x").digest()) is None
        assert fabgpu.memo_lookup_p384(csp, y, x, sig, dg) is None
        assert fabgpu.memo_lookup_p384(csp, x, y, sig + b"\0", dg) is None
        assert fabgpu.memo_lookup_p384(csp, x, y, sig + dg[:1], dg[1:]) is None
    finally:
        csp.close()


def test_seeding_fresh_form(blk):
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        for sg in blk["signers"][:2]:                        # one signer is not imported: the batch takes the fresh-key kernel
            csp.key_import_p384(sg.q)
        out = _pass(csp, blk, 42)
        st = csp.p384_pass_stats()
        assert (st["keyed_launches"], st["fresh_launches"], st["submitted"], st["memo_seeded"]) == (0, 1, 24, 24)
        assert out["tuple_status"].tolist() == blk["want"] and out["memo_seeded"] == 24
        assert [_ask(csp, tu) for tu in blk["tuples"]] == [(w, 42) for w in blk["want"]]
    finally:
        csp.close()


@pytest.fixture(scope="module")
def mixed():
    """4 transactions signed by P-256 identities and 4 signed by P-384 identities"""
    rnd = random.Random(44384)
    s = pb.signers(3, 44384)
    fx = blockgen.fixture_signers()
    sign256 = blockgen.make_signer(11)
    p = [P256Signer(fx[k][0], fx[k][1], sign256) for k in (4, 0, 1)]
    envs, tuples = [], []
    for t in range(8):
        who = p if t % 2 == 0 else s
        env, tu = pb.endorser_tx(rnd, who[0], [who[1], who[2]])
        envs.append(env)
        tuples += tu
    is384 = [isinstance(tu[1], pb.Signer) for tu in tuples]
    assert is384.count(True) == 12 and is384.count(False) == 12
    return dict(block=bb.block(9, envs), tuples=tuples, is384=is384, signers=s)


def _ask256(csp, out, i, sig):
    return fabgpu.memo_lookup(csp, bytes(out["tuple_qxy"][i][:32]), bytes(out["tuple_qxy"][i][32:]), sig, bytes(out["tuple_digest"][i]))


def test_mixed_block_against_the_option_off(mixed):
    rows256 = [i for i, v in enumerate(mixed["is384"]) if not v]
    rows384 = [i for i, v in enumerate(mixed["is384"]) if v]
    runs = {}
    for p384 in (0, 1):
        csp = fabgpu.GPUCSP(device=0, p384=p384)
        try:
            out = _pass(csp, mixed, 5)
            a256 = [_ask256(csp, out, i, mixed["tuples"][i][3]) for i in rows256]
            a384 = [_ask(csp, mixed["tuples"][i]) for i in rows384]
            runs[p384] = dict(out=out, a256=a256, a384=a384, stats=fabgpu.memo_stats(csp), stats384=fabgpu.memo_stats_p384(csp),
                              has=fabgpu.memo_has_block(csp, 5))
            if p384:                                         # lifetime: one eviction drops both tables' entries of the block, summed
                assert fabgpu.memo_evict_block(csp, 5) == out["memo_seeded"] == runs[1]["stats"]["entries"] + 12
                assert [_ask256(csp, out, i, mixed["tuples"][i][3]) for i in rows256] == [None] * 12
                assert [_ask(csp, mixed["tuples"][i]) for i in rows384] == [None] * 12
                assert fabgpu.memo_has_block(csp, 5) == 0 and fabgpu.memo_stats_p384(csp)["evicted"] == 12
        finally:
            csp.close()
    off, on = runs[0], runs[1]
    # the P-256 tuples: the off-run's answers from fabgpu_csp_memo_lookup, the off-run's counters, the off-run's rows of every output
    assert on["a256"] == off["a256"] == [0] * 12 and on["stats"] == off["stats"] and off["stats"]["hits"] == 12
    for k in ("tuple_tx", "tuple_kind", "tuple_spans"):
        assert np.array_equal(on["out"][k], off["out"][k]), k
    for k in ("tuple_status", "tuple_digest", "tuple_hashed", "tuple_qxy"):
        assert np.array_equal(on["out"][k][rows256], off["out"][k][rows256]), k
    assert on["out"]["tuple_hashed"][rows256].all() and not on["out"]["tuple_hashed"][rows384].any()
    # the P-384 tuples: only the new entry knows them, and only with the option on
    assert on["a384"] == [(0, 5)] * 12 and off["a384"] == [None] * 12
    assert on["stats384"] == dict(entries=12, hits=12, misses=0, evicted=0) and off["stats384"] == dict(entries=0, hits=0, misses=0, evicted=0)
    assert on["out"]["memo_seeded"] == off["out"]["memo_seeded"] + 12 and on["has"] == off["has"] + 12
    assert on["out"]["tx_flags"].tolist() == [0] * 8 and off["out"]["tx_flags"].tolist() == [0, pb.TX_NEEDS_SW] * 4


def test_tuples_the_stage_does_not_decide_get_no_entry():
    rnd = random.Random(45384)
    s = pb.signers(3, 45384)
    high_s = lambda m, sig: (lambda r, t: ref.der_sig(r, ref.N - t))(*pb.parse_der_sig(sig))
    envs, tuples = [], []
    for kw in (dict(creator_sig=high_s), dict(end_sig=lambda j, m, sig: b"" if j == 1 else sig), dict()):
        env, tu = pb.endorser_tx(rnd, s[0], [s[1], s[2]], **kw)
        envs.append(env)
        tuples += tu
    want = [pb.tuple_status(who.q, msg, sig) for _, who, msg, sig in tuples]
    assert want == [2, 0, 0, 0, 0, pb.TUPLE_ST_EMPTY_SIG, 0, 0, 0]
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        out = fabgpu.preverify_block2(csp, bb.block(3, envs), block_seq=6, seed_memo=True)
        assert out["tuple_status"].tolist() == want
        assert out["memo_seeded"] == 7 == csp.p384_pass_stats()["memo_seeded"] == csp.p384_pass_stats()["submitted"]
        got = [_ask(csp, tu) if tu[3] else None for tu in tuples]      # (an empty signature is no question a lookup takes)
        assert got == [(0, 6) if w == 0 else None for w in want]
        _, who, msg, _ = tuples[5]
        assert fabgpu.memo_lookup_p384(csp, ref.b48(who.q[0]), ref.b48(who.q[1]), b"", hashlib.sha256(msg).digest()) is None
    finally:
        csp.close()


def test_capacity_pushes_the_older_record_out_whole(blk, blk_b):
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        fabgpu.memo_set_capacity_p384(csp, 24)
        _pass(csp, blk, 1)
        assert [_ask(csp, tu) for tu in blk["tuples"]] == [(w, 1) for w in blk["want"]]
        _pass(csp, blk_b, 2)
        assert [_ask(csp, tu) for tu in blk["tuples"]] == [None] * 24
        assert [_ask(csp, tu) for tu in blk_b["tuples"]] == [(w, 2) for w in blk_b["want"]]
        assert fabgpu.memo_stats_p384(csp) == dict(entries=24, hits=48, misses=24, evicted=24)
        assert fabgpu.memo_has_block(csp, 1) == 0 and fabgpu.memo_has_block(csp, 2) == 24
        assert fabgpu.memo_evict_block(csp, 1) == 0 and fabgpu.memo_evict_block(csp, 2) == 24
        assert [_ask(csp, tu) for tu in blk_b["tuples"]] == [None] * 24
    finally:
        csp.close()


def test_option_off_nothing_is_seeded_and_the_pass_answers_as_before(blk):
    outs = []
    for kw in (dict(), dict(p384=0)):                        # a provider that never heard of the option, and one with it off
        csp = fabgpu.GPUCSP(device=0, **kw)
        try:
            outs.append(_pass(csp, blk, 9))
            assert [_ask(csp, tu) for tu in blk["tuples"]] == [None] * 24
            assert fabgpu.memo_stats_p384(csp) == dict(entries=0, hits=0, misses=0, evicted=0)
            assert csp.p384_pass_stats() == dict.fromkeys(fabgpu.P384_PASS_STATS, 0) and fabgpu.memo_has_block(csp, 9) == 0
        finally:
            csp.close()
    for k in ARRAYS:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    assert outs[0]["memo_seeded"] == outs[1]["memo_seeded"] == 0
    assert outs[1]["tuple_status"].tolist() == [pb.TUPLE_ST_NEEDS_SW] * 24 and outs[1]["tx_flags"].tolist() == [pb.TX_NEEDS_SW] * 8


def test_option_on_without_the_seed_flag_adds_no_entries(blk):
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        out = _pass(csp, blk, 10, seed_memo=False)
        assert out["tuple_status"].tolist() == blk["want"] and out["memo_seeded"] == 0
        st = csp.p384_pass_stats()
        assert st["submitted"] == 24 and st["memo_seeded"] == 0
        assert [_ask(csp, tu) for tu in blk["tuples"]] == [None] * 24
        assert fabgpu.memo_stats_p384(csp) == dict(entries=0, hits=0, misses=24, evicted=0) and fabgpu.memo_has_block(csp, 10) == 0
    finally:
        csp.close()


def test_audit_of_hits_agrees_without_corruption(blk):
    csp = fabgpu.GPUCSP(device=0, p384=1, audit_permille=1000)
    try:
        _pass(csp, blk, 11)
        base = csp.audit_stats()
        assert csp.p384_verdict_audits() == 0 and base["direct_audits"] == 21       # (the pass audited its own "valid" rows)
        assert [_ask(csp, tu) for tu in blk["tuples"]] == [(w, 11) for w in blk["want"]]
        st = csp.audit_stats()
        assert csp.p384_verdict_audits() == 24 and st["mismatches"] == 0 and st["verdict_audits"] == base["verdict_audits"] == 0
        assert csp.poisoned() is None
    finally:
        csp.close()


def test_audit_catches_a_corrupted_entry_and_poisons(blk):
    csp = fabgpu.GPUCSP(device=0, p384=1, audit_permille=1000)
    try:
        _pass(csp, blk, 12)
        bad = blk["want"].index(1)                           # (all 24 tuples were submitted: entry i is tuple i)
        good = blk["want"].index(0)
        assert fabgpu.p384_memo_corrupt(csp, 12, good) == 1 and fabgpu.p384_memo_corrupt(csp, 13, bad) == 1
        assert _ask(csp, blk["tuples"][good]) == (0, 12) and csp.poisoned() is None
        assert fabgpu.p384_memo_corrupt(csp, 12, bad) == 0   # a stored reject now reads "valid"
        assert _ask(csp, blk["tuples"][bad]) is None         # the audit recomputes it: a miss, and the provider is retired
        assert "P-384 verdict memo" in csp.poisoned()
        assert csp.audit_stats()["mismatches"] == 1
        assert [_ask(csp, tu) for tu in blk["tuples"]] == [None] * 24
        with pytest.raises(fabgpu.PoisonedError):
            _pass(csp, blk, 13)
    finally:
        csp.close()


def test_a_poisoned_provider_misses_and_a_corrupt_entry_is_handed_out_without_audit(blk):
    """Poison() by hand makes every later lookup miss; and with auditing off the hook's corruption is what comes back - the audit test
    above fails for the right reason if the sampler does not run"""
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        _pass(csp, blk, 14)
        bad = blk["want"].index(1)
        assert fabgpu.p384_memo_corrupt(csp, 14, bad) == 0
        assert _ask(csp, blk["tuples"][bad]) == (0, 14) and csp.p384_verdict_audits() == 0
        csp.poison("test")
        assert [_ask(csp, tu) for tu in blk["tuples"]] == [None] * 24
    finally:
        csp.close()
