"""The two C entries of the block pass - fabgpu_csp_block_preverify and fabgpu_csp_block_preverify2 - run one body: with no flags they
give one answer, on the device route and on the host route, and they keep their differences at FABGPU_ETOOBIG (the first entry reports
the tuples COUNTED so far, 0 included; the second says how many fit while nothing is counted)."""
import ctypes
import hashlib

import numpy as np
import pytest

import bccsp_sw_oracle as po
import blockbuilder as bb
import blockgen
import fabgpu

ETOOBIG = -5
N_TX, N_TUPLES = 3, 9            # 3 transactions x (creator + 2 endorsements); bb.block carries no orderer signatures


def _block():
    """-> (block, per-tuple oracle statuses in walk order, per-transaction flags): endorsement 1 of transaction 1 is re-encoded high-S"""
    fx = blockgen.fixture_signers()
    rng, sign = np.random.default_rng(77), blockgen.make_signer(78)

    def craft(t, j, der):
        if (t, j) != (1, 1):
            return der
        r, s = po.unmarshal_ecdsa_signature(der)
        return po.marshal_ecdsa_signature(r, po.N - s)
    envs = [blockgen.endorser_tx(t, rng, fx[4 + t % 2], [fx[t % 4], fx[(t + 1) % 4]], sign, craft, ext_bytes=200) for t in range(N_TX)]
    blk = bb.block(5, envs)
    tuples, arena = fabgpu.block_tuples(blk)
    key = {ident: blockgen._pubkey(d32) for ident, d32 in fx}
    status, flags = [], [fabgpu.TX_ALL_SIGNATURES_VALID] * N_TX
    for tp in tuples:
        cut = lambda sp: arena[sp[0]:sp[0] + sp[1]]
        q, msg, sig = key[cut(tp["identity"])], cut(tp["prefix"]) + cut(tp["suffix"]), cut(tp["sig"])
        r, s = po.unmarshal_ecdsa_signature(sig)
        st = po.status_raw(int.from_bytes(q[:32], "big"), int.from_bytes(q[32:], "big"), hashlib.sha256(msg).digest(), r, s)
        assert (st == 0) == (po.identity_verify((int.from_bytes(q[:32], "big"), int.from_bytes(q[32:], "big")), msg, sig) is None)
        status.append(st)
        if st != 0:
            flags[tp["tx"]] = fabgpu.TX_BAD_ENDORSEMENT if tp["kind"] == fabgpu.TUPLE_ENDORSEMENT else fabgpu.TX_BAD_CREATOR_SIGNATURE
    assert len(tuples) == N_TUPLES and status == [0, 0, 0, 0, 0, po.ST_HIGH_S, 0, 0, 0] and flags == [0, fabgpu.TX_BAD_ENDORSEMENT, 0]
    return np.frombuffer(blk, dtype=np.uint8).copy(), np.array(status, np.uint8), np.array(flags, np.uint8)


BLOCK = None


def _case():
    global BLOCK
    if BLOCK is None:
        BLOCK = _block()          # built once: the oracle's answers are shared by the tests below
    return BLOCK


FIELDS = ["tx_flags", "tx_type", "tuple_tx", "tuple_kind", "tuple_status"]


def _arrays(cap_tx, cap_tu):
    return dict(tx_flags=np.full(cap_tx, 0xEE, np.uint8), tx_type=np.full(cap_tx, 0xEE, np.uint8), tuple_tx=np.full(cap_tu, 0xEEEEEEEE, np.uint32),
                tuple_kind=np.full(cap_tu, 0xEE, np.uint8), tuple_status=np.full(cap_tu, 0xEE, np.uint8))


def _entry1(csp, buf, cap_tx=16, cap_tu=64, only=FIELDS):
    a = _arrays(cap_tx, cap_tu)
    n_tx, n_tu = ctypes.c_uint32(0xAAAA), ctypes.c_uint32(0xBBBB)
    p = {k: (a[k].ctypes.data_as(fabgpu._u32p) if k == "tuple_tx" else fabgpu._p8(a[k])) if k in only else None for k in FIELDS}
    rc = csp._L.fabgpu_csp_block_preverify(csp._h, fabgpu._p8(buf), buf.size, ctypes.byref(n_tx), p["tx_flags"], p["tx_type"], cap_tx, ctypes.byref(n_tu),
                                           p["tuple_tx"], p["tuple_kind"], p["tuple_status"], cap_tu)
    return rc, n_tx.value, n_tu.value, a


def _entry2(csp, buf, cap_tx=16, cap_tu=64):
    a = _arrays(cap_tx, cap_tu)
    ps = fabgpu._BlockPass()
    ps.block, ps.len, ps.block_seq, ps.flags, ps.cap_tx, ps.cap_tuples = buf.ctypes.data, buf.size, 0, 0, cap_tx, cap_tu
    for k in FIELDS:
        setattr(ps, k, a[k].ctypes.data)
    rc = csp._L.fabgpu_csp_block_preverify2(csp._h, ctypes.byref(ps))
    return rc, ps.n_tx, ps.n_tuples, a


def _answers(n_tx, n_tu, a):
    return {k: (a[k][:n_tx] if k.startswith("tx_") else a[k][:n_tu]).tolist() for k in FIELDS}


@pytest.fixture(params=[0, -1], ids=["device_walk", "host_walk"])
def csp(request):
    c = fabgpu.GPUCSP(device=0)
    c.set_option("pass_device_walk", request.param)
    c.device_walk = request.param >= 0
    yield c
    c.close()


@pytest.mark.gpu
def test_both_entries_give_one_answer_and_it_is_the_oracles(csp):
    buf, status, flags = _case()
    rc1, n_tx1, n_tu1, a1 = _entry1(csp, buf)
    rc2, n_tx2, n_tu2, a2 = _entry2(csp, buf)
    assert (rc1, n_tx1, n_tu1) == (0, N_TX, N_TUPLES) == (rc2, n_tx2, n_tu2)
    one, two = _answers(n_tx1, n_tu1, a1), _answers(n_tx2, n_tu2, a2)
    assert one == two
    assert one["tx_flags"] == flags.tolist() and one["tuple_status"] == status.tolist()
    assert one["tuple_tx"] == [0, 0, 0, 1, 1, 1, 2, 2, 2] and one["tuple_kind"] == [0, 1, 1] * 3 and one["tx_type"] == [3, 3, 3]
    routes = fabgpu.pass_routes(csp)
    assert (routes["device_walks"], routes["host_walks"]) == ((2, 0) if csp.device_walk else (0, 2)), routes


@pytest.mark.gpu
def test_too_small_arrays_launch_nothing_and_the_retry_finds_its_upload(csp):
    buf, status, flags = _case()
    before, passes = fabgpu.pass_routes(csp), csp.passes_per_device()
    rc1, n_tx1, n_tu1, _ = _entry1(csp, buf, cap_tx=1)
    rc2, n_tx2, n_tu2, _ = _entry2(csp, buf, cap_tx=1)
    assert (rc1, n_tx1) == (ETOOBIG, N_TX) == (rc2, n_tx2)
    # the device route says so from the outline, before anything is counted: the first entry reports the 0 tuples counted, the second
    # that 64 fit; the host route has walked the block by then
    assert (n_tu1, n_tu2) == ((0, 64) if csp.device_walk else (N_TUPLES, N_TUPLES))
    after = fabgpu.pass_routes(csp)
    if not csp.device_walk:      # (a provider with the device walk switched off counts the decline of each attempt, launched or not)
        assert after["host_walks"] == before["host_walks"] + 2 and after["last_decline"] == "pass_device_walk is off"
        after = dict(after, host_walks=before["host_walks"], last_decline=before["last_decline"])
    assert after == before and csp.passes_per_device() == passes
    rc1, n_tx1, n_tu1, a1 = _entry1(csp, buf)                       # the retry with room
    assert (rc1, n_tx1, n_tu1) == (0, N_TX, N_TUPLES)
    assert _answers(n_tx1, n_tu1, a1)["tx_flags"] == flags.tolist() and _answers(n_tx1, n_tu1, a1)["tuple_status"] == status.tolist()
    assert csp._L.fabgpu_csp_block_pass_abandon(csp._h) == 0         # ... took the parked upload along
    rc2, n_tx2, n_tu2, a2 = _entry2(csp, buf)
    assert rc2 == 0 and _answers(n_tx2, n_tu2, a2) == _answers(n_tx1, n_tu1, a1)
    assert sum(csp.passes_per_device()) == sum(passes) + 2


@pytest.mark.gpu
def test_a_status_array_alone_makes_the_first_entry_mind_the_tuple_room(csp):
    buf, status, flags = _case()
    rc, n_tx, n_tu, _ = _entry1(csp, buf, cap_tu=1, only=["tx_flags", "tuple_status"])
    assert (rc, n_tx, n_tu) == (ETOOBIG, N_TX, N_TUPLES)
    assert csp._L.fabgpu_csp_block_pass_abandon(csp._h) == 1         # no retry comes: the kept upload is dropped
    rc, n_tx, n_tu, a = _entry1(csp, buf, cap_tu=1, only=["tx_flags"])   # flags alone: room for tuples does not matter
    assert (rc, n_tx, n_tu) == (0, N_TX, N_TUPLES) and a["tx_flags"][:N_TX].tolist() == flags.tolist()
