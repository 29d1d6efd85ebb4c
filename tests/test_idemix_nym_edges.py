"""The pseudonym-signature commitment on adversarial vectors (tests/nym_vectors.py), in every lane geometry: on the CPU through the host
compilation of bn_nym29.h (one lane and two lanes per signature), on the MI355X through gputest_nym_commitment (one, two and four lanes;
the four-lane form, bn_quad29.h, has no host build) and through the product entry point under its five kernel configurations.  Every
comparison is exact equality with big integers.

The `exc` flag of glv_mult29 - a collision inside the interleaved one-lane loop - is NOT reached by any of these vectors
(nym_vectors.one_lane_collision checks that none does): the host test with the identity "endomorphism" in
tests/test_idemix_oracle.py::test_glv_decomposition_and_double_scalar_loop remains its only exerciser."""
import ctypes
import os
import random

import numpy as np
import pytest

import idemix_oracle as io
import nym_vectors as nv
from idemix_common import ROOT, NymBatch, be32, env  # noqa: F401  (env: the five kernel configurations, a fixture)

CAP = {0: 64, 1: 32, 2: 16}
_memo = {}


@pytest.fixture(scope="module")
def vectors():
    return nv.build()


@pytest.fixture(scope="module")
def hosttest():
    L = ctypes.CDLL(os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_hosttest.so"))
    L.hosttest_bn_issuer_new.restype = ctypes.c_void_p
    L.hosttest_bn_issuer_new.argtypes = [ctypes.c_char_p] * 4
    L.hosttest_bn_issuer_free.argtypes = [ctypes.c_void_p]
    L.hosttest_bn_nym_commitment.argtypes = [ctypes.c_void_p] + [ctypes.c_char_p] * 7
    L.hosttest_bn_nym_commitment_split.argtypes = [ctypes.c_void_p] + [ctypes.c_char_p] * 7
    return L


@pytest.fixture(scope="module")
def dev():
    return ctypes.CDLL(os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_gputest.so"))


def decomposition_inputs(n_random, seed):
    rng = random.Random(seed)
    ks = [c for _, c in nv.glv_edge_cs()] + [c for _, c, _ in nv.booth_edge_cs()] + [nv.R, nv.R + 1, (1 << 255), (1 << 256) - 1]
    return ks + [rng.randrange(1 << 256) for _ in range(n_random)]


# ---- CPU half -------------------------------------------------------------------------------------------------------------------------------
def test_generator_self_check(vectors):
    _, V = vectors
    print(nv.report())
    count = {cls: len(V[cls]) for cls in nv.CLASSES}
    assert all(count.values()), count
    names = [n for n, _ in nv.glv_edge_cs()]
    for sign in ("k1>0,k2<0", "k1>0,k2>0"):
        assert len([n for n in names if n.startswith(sign)]) >= 8, sign
    assert len([n for n in names if n.startswith("|k1| rank")]) == 8 and len([n for n in names if n.startswith("|k2| rank")]) == 8
    # what cannot exist is named, with the reason - and is exactly what the bounds of the module's docstring rule out
    dead = {"glv_edges k1<0,k2<0", "glv_edges k1<0,k2>0"} | {"booth_edges %s on k%d" % (p, h) for p in ("top_window_26_only", "carry_into_window_26")
                                                              for h in (1, 2)}
    assert set(nv.UNREACHABLE) == dead, sorted(set(nv.UNREACHABLE) ^ dead)
    booth = nv.booth_edge_cs()
    for p, (mag, holds) in nv.BOOTH_PATTERNS.items():
        for h in (1, 2):
            got = [e for e in booth if e[0].startswith("%s on k%d " % (p, h))]
            if "booth_edges %s on k%d" % (p, h) in dead:
                assert not got
                continue
            # a k1 of one low digit goes with k2 == 0 alone (f2 of the decomposition falls under the rounding of its quotients otherwise)
            assert len(got) >= (1 if p.startswith("single_low") and h == 1 else 4), (p, h, len(got))
            for _, c, (k1, k2) in got:
                assert nv.glv_decompose(c) == (k1, k2) and holds(nv.booth_digits(abs(k1 if h == 1 else k2)))
    for cls in nv.EXCEPTIONAL_CLASSES:
        for v in V[cls]:
            assert nv.check_vector(v) == [], (cls, v.name)
    for cls in nv.CLASSES + ["ordinary", "short"]:
        for v in V[cls]:
            assert not nv.one_lane_collision(v.c), (cls, v.name)
            k1, k2 = nv.glv_decompose(v.c)
            assert (k1 + k2 * nv.LAM - v.c) % nv.R == 0 and k1 >= 0 and max(k1, abs(k2)) < 1 << 129
    assert {v.status for v in V["last_add"]} == {0, 6} and {v.status for v in V["infinities"]} == {0, 6}
    for cls in nv.CLASSES:
        for split in (0, 1, 2):
            assert nv.placements(cls, CAP[split])


def test_python_decomposition_against_the_host_compilation(hosttest):
    m1b, m2b = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    for k in decomposition_inputs(20000, 41):
        fl = hosttest.hosttest_bn_glv_decompose(be32(k), m1b, m2b)
        k1, k2 = nv.glv_decompose(k)
        assert (int.from_bytes(m1b.raw, "big"), int.from_bytes(m2b.raw, "big"), fl) == (abs(k1), abs(k2), (k1 < 0) | (k2 < 0) << 1), hex(k)


@pytest.mark.parametrize("cls", nv.CLASSES + ["ordinary", "short"])
def test_host_compilation_on_every_vector(hosttest, vectors, cls):
    issuers, V = vectors
    ox, oy = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    for name in sorted({v.issuer for v in V[cls]}):
        iss = issuers[name]
        h = ctypes.c_void_p(hosttest.hosttest_bn_issuer_new(be32(iss.hsk[0]), be32(iss.hsk[1]), be32(iss.hrand[0]), be32(iss.hrand[1])))
        try:
            for v in (v for v in V[cls] if v.issuer == name):
                for fn in (hosttest.hosttest_bn_nym_commitment, hosttest.hosttest_bn_nym_commitment_split):
                    st = fn(h, be32(v.nym[0]), be32(v.nym[1]), be32(v.c), be32(v.s_sk), be32(v.s_rnym), ox, oy)
                    assert st == v.status, (cls, v.name, fn.__name__, st, v.status)
                    if v.status == 0:
                        assert (int.from_bytes(ox.raw, "big"), int.from_bytes(oy.raw, "big")) == v.t, (cls, v.name, fn.__name__)
        finally:
            hosttest.hosttest_bn_issuer_free(h)


def test_the_oracle_accepts_signatures_with_chosen_s_values():
    rows = nv.signed_comb_edges()
    ipk = nv.build()[0][nv.FIXTURE_ISSUER].ipk
    want = [io.nym_verify(sig, nym, ipk, msg) for nym, sig, msg, _, _ in rows]
    assert want == [0, 1] * (len(rows) // 2)
    zeros = [(which, v) for _, _, _, which, v in rows[::2] if v == 0]
    assert zeros == [("s_sk", 0), ("s_rnym", 0)]           # the rows an s_inf = 1 record of the side stream has to carry


# ---- GPU half -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_decomposition_on_device(dev):
    ks = decomposition_inputs(65536, 43)
    n = len(ks)
    inp = np.frombuffer(b"".join(be32(k) for k in ks), dtype=np.uint8).copy()
    out = np.zeros(68 * n, dtype=np.uint8)
    rc = dev.gputest_bn_glv_decompose(ctypes.c_uint32(n), inp.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    raw = out.tobytes()
    for i, k in enumerate(ks):
        row = raw[68 * i:68 * i + 68]
        k1, k2 = nv.glv_decompose(k)
        got = (int.from_bytes(row[:32], "big"), int.from_bytes(row[32:64], "big"), int.from_bytes(row[64:], "little"))
        assert got == (abs(k1), abs(k2), (k1 < 0) | (k2 < 0) << 1), hex(k)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 1, 2], ids=["one-lane", "two-lanes", "four-lanes"])
@pytest.mark.parametrize("cls", nv.CLASSES)
def test_commitment_on_device(dev, vectors, cls, split):
    issuers, _ = vectors
    for w, wave in enumerate(nv.placements(cls, CAP[split])):
        iss = issuers[wave[0].issuer]
        m = len(wave)
        rows = b"".join(be32(v.nym[0]) + be32(v.nym[1]) + be32(v.c) + be32(v.s_sk) + be32(v.s_rnym) for v in wave)
        out = ctypes.create_string_buffer(64 * m)
        st = (ctypes.c_uint32 * m)()
        rc = dev.gputest_nym_commitment(split, m, be32(iss.hsk[0]) + be32(iss.hsk[1]), be32(iss.hrand[0]) + be32(iss.hrand[1]), rows, out, st)
        assert rc == 0, rc
        for i, v in enumerate(wave):
            assert st[i] == v.status, (cls, split, w, i, v.cls, v.name, st[i], v.status)
            if v.status == 0:
                got = (int.from_bytes(out.raw[64 * i:64 * i + 32], "big"), int.from_bytes(out.raw[64 * i + 32:64 * i + 64], "big"))
                assert got == v.t, (cls, split, w, i, v.cls, v.name)


@pytest.mark.gpu
@pytest.mark.parametrize("side_after", [False, True], ids=["side-stream", "side-launch-late"])
def test_signatures_with_edge_s_values_through_the_product(env, side_after):
    """valid signatures whose s_sk or s_rnym is a comb_edges value (0 among them: the fixed-base term at infinity, s_inf = 1 in the side
    stream's record), each beside a twin with one message bit flipped"""
    ctx, issuers = env
    ipk = issuers[0][0]
    assert bytes(ipk.hash) == bytes(nv.build()[0][nv.FIXTURE_ISSUER].ipk.hash)
    if "exp" not in _memo:      # the oracle's verdicts, once for the ten runs
        _memo["exp"] = [io.nym_verify(sig, nym, ipk, msg) for nym, sig, msg, _, _ in nv.signed_comb_edges()]
    b = NymBatch()
    for (nym, sig, msg, _, _), want in zip(nv.signed_comb_edges(), _memo["exp"]):
        b.add(0, ipk, nym, sig, msg, expect=want)
    arena, off, iid, cols, expect = b.arrays()
    assert list(expect) == [0, 1] * (len(expect) // 2) and len(expect) <= 16384
    ctx.test_nym_side_after(side_after)
    try:
        ok, st = ctx.idemix_nym_verify_batch(arena, off, *cols, issuer_id=iid)
    finally:
        ctx.test_nym_side_after(False)
    assert np.array_equal(st, expect), [(int(i), int(st[i])) for i in np.nonzero(st != expect)[0][:8]]
    assert np.array_equal(ok, expect == 0)

