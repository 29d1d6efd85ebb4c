"""One batch through each of the ten ECDSA P-256 verify kernels of kernels.hip, chosen by context flags and key registration alone,
through the digest call and through the fused hash+verify call; status bytes and verdict bits bit for bit against the CPU oracle,
the digests a fused run returns against hashlib.

  flags                                   digest call                          fused call
  ONE_LANE_ONLY                           p256_verify_kernel                   sha256_p256_verify_kernel
  PAIR_TABLE_GLOBAL                       p256_verify_pair_kernel              sha256_p256_verify_pair_kernel
  PAIR_TABLE_LDS                          p256_verify_pair_lds_kernel          sha256_p256_verify_pair_kernel
  PAIR_TABLE_LDS | PAIR_SOLO              p256_verify_pair_lds_solo_kernel     sha256_p256_verify_pair_kernel
  NO_WIDE | ONE_LANE_ONLY, keys by id     p256_verify_keyed_kernel             sha256_p256_verify_keyed_kernel
  NO_WIDE, keys by id                     p256_verify_keyed_pair_kernel        sha256_p256_verify_keyed_pair_kernel

n = 257 rows: with one lane per signature one full 256-row tile plus one lane, with two lanes per signature two full 128-row tiles plus
one pair - both shapes reach the tail lanes that compute on row n - 1 and the partial last ballot word.  Rows: the in-range vectors of
tests/golden/edge_kats.json (in keyed runs those whose key can be registered), padded with seeded valid signatures of a small key pool;
keyed runs name one key id that is not registered."""
import hashlib
import json
import os

import numpy as np
import pytest

import bccsp_sw_oracle as po
import coracle
import fabgpu

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 257
BAD_ID_ROW = 200          # a padding row (a valid signature) whose key id is out of range in keyed runs
FORMS = {
    "one-lane": (fabgpu.FLAG_ONE_LANE_ONLY, False),
    "pair-table-global": (fabgpu.FLAG_PAIR_TABLE_GLOBAL, False),
    "pair-table-lds": (fabgpu.FLAG_PAIR_TABLE_LDS, False),
    "pair-table-lds-solo": (fabgpu.FLAG_PAIR_TABLE_LDS | fabgpu.FLAG_PAIR_SOLO, False),
    "keyed-one-lane": (fabgpu.FLAG_NO_WIDE | fabgpu.FLAG_ONE_LANE_ONLY, True),
    "keyed-pair": (fabgpu.FLAG_NO_WIDE, True),
}


def _h32(x):
    return bytes.fromhex(x.rjust(64, "0"))


def _arr(items):
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(-1, 32).copy()


def _dataset(vs, seed):
    """N rows: the vectors vs, then valid signatures by a pool of four keys.  Given digests (e) for the digest call; messages whose
    SHA-256 the padding rows signed for the fused call (the edge rows keep their keys and signatures under a digest they were not made for)."""
    m = len(vs)
    assert 0 < m < N - 128          # the padding reaches into every tile
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 200, size=N)
    lens[:3] = (0, 55, 64)          # empty, one block with the padding exactly fitting, one block plus a padding block
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    arena = rng.integers(0, 256, size=int(off[-1]) + 1, dtype=np.uint8)
    dig = _arr([hashlib.sha256(arena[off[i]:off[i + 1]].tobytes()).digest() for i in range(N)])
    pad_e = coracle.make_pool_batch(N - m, seed=seed, nkeys=4)
    pad_m = coracle.make_pool_batch(N - m, seed=seed, nkeys=4, digests=dig[m:])
    assert (pad_e["pool_qx"] == pad_m["pool_qx"]).all()
    d = dict(arena=arena, off=off, dig=dig)
    d["qx"] = np.concatenate([_arr([_h32(v["qx"]) for v in vs]), pad_e["qx"]])
    d["qy"] = np.concatenate([_arr([_h32(v["qy"]) for v in vs]), pad_e["qy"]])
    assert (d["qx"][m:] == pad_m["qx"]).all() and (d["qy"][m:] == pad_m["qy"]).all()
    edge_r, edge_s = _arr([_h32(v["r"]) for v in vs]), _arr([_h32(v["s"]) for v in vs])
    d["e"] = np.concatenate([_arr([fabgpu.hash_to_int(bytes.fromhex(v["e"])) for v in vs]), pad_e["e"]])   # hashToInt on the host, as the Go provider does
    d["r"], d["s"] = np.concatenate([edge_r, pad_e["r"]]), np.concatenate([edge_s, pad_e["s"]])
    d["r_msg"], d["s_msg"] = np.concatenate([edge_r, pad_m["r"]]), np.concatenate([edge_s, pad_m["s"]])
    d["want"] = coracle.verify_batch(d["qx"], d["qy"], d["e"], d["r"], d["s"])
    d["want_msg"] = coracle.verify_batch(d["qx"], d["qy"], dig, d["r_msg"], d["s_msg"])
    assert list(d["want"][:m]) == [v["status"] for v in vs]
    assert (d["want"][m:] == 0).all() and (d["want_msg"][m:] == 0).all() and (d["want_msg"][:m] != 0).all()
    for w in (d["want"], d["want_msg"]):
        w.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def data():
    vs = [v for v in json.load(open(os.path.join(G, "edge_kats.json")))["vectors"] if 0 <= int(v["r"], 16) < 1 << 256 and 0 <= int(v["s"], 16) < 1 << 256]
    keyed = [v for v in vs if po.on_curve(int(v["qx"], 16), int(v["qy"], 16))]
    assert len(vs) > 100 and 60 < len(keyed) < len(vs)
    return {False: _dataset(vs, 20261017), True: _dataset(keyed, 20261018)}


@pytest.fixture(scope="module", params=list(FORMS))
def form(request, data):
    """(context, rows, key ids or None, expected status of the digest call, of the fused call)"""
    flags, keyed = FORMS[request.param]
    d = data[keyed]
    c = fabgpu.Context(device=0, flags=flags)
    ids, want, want_msg = None, d["want"], d["want_msg"]
    if keyed:
        reg = {}
        for qx, qy in zip(d["qx"], d["qy"]):
            k = (qx.tobytes(), qy.tobytes())
            if k not in reg:
                reg[k] = c.key_register(*k)
        ids = np.array([reg[(qx.tobytes(), qy.tobytes())] for qx, qy in zip(d["qx"], d["qy"])], dtype=np.uint32)
        ids[BAD_ID_ROW] = len(reg) + 1000
        want, want_msg = want.copy(), want_msg.copy()
        assert want[BAD_ID_ROW] == 0 and want_msg[BAD_ID_ROW] == 0
        want[BAD_ID_ROW] = want_msg[BAD_ID_ROW] = 4        # "use bccsp/sw", never a verdict
    yield c, d, ids, want, want_msg
    c.close()


def _same(bits, st, want):
    assert st.dtype == np.uint8 and (st == want).all(), np.nonzero(st != want)[0][:20]
    assert bits.shape == (N,) and (bits == (want == 0)).all()


def test_digest_call(form):
    c, d, ids, want, _ = form
    if ids is None:
        bits, st = c.p256_verify_batch(d["qx"], d["qy"], d["e"], d["r"], d["s"])
    else:
        bits, st = c.p256_verify_batch_keyed(ids, d["e"], d["r"], d["s"])
    _same(bits, st, want)


def test_fused_call(form):
    c, d, ids, _, want_msg = form
    if ids is None:
        bits, st, dig = c.identity_verify_batch(d["arena"], d["off"], d["r_msg"], d["s_msg"], qx=d["qx"], qy=d["qy"], want_digests=True)
    else:
        bits, st, dig = c.identity_verify_batch(d["arena"], d["off"], d["r_msg"], d["s_msg"], key_id=ids, want_digests=True)
    _same(bits, st, want_msg)
    assert (dig == d["dig"]).all()
