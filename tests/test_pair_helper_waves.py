"""The helper-wave form of the LDS-table pair kernel (p256_verify_pair_lds_kernel: main waves run the u2*Q chain, helper waves on the
same SIMDs compute s^-1, u1, u2 and u1*G and hand u2 and S over through LDS) against the CPU oracle and, bit for bit, against its
one-wave-per-SIMD form (FABGPU_FLAG_PAIR_SOLO): verdict bits and status bytes, in every case where the handoff could go wrong -
partial last tiles, the recoding-edge scalars, u1 = 0, the range and curve gates, and wavefronts that mix gated and valid lanes."""
import numpy as np
import pytest

import bccsp_sw_oracle as po
import coracle
import fabgpu
import scalar_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def forms():
    """(helper, solo): both forced onto the LDS table, so that batches of any size take it."""
    helper = fabgpu.Context(device=0, flags=fabgpu.FLAG_PAIR_TABLE_LDS)
    solo = fabgpu.Context(device=0, flags=fabgpu.FLAG_PAIR_TABLE_LDS | fabgpu.FLAG_PAIR_SOLO)
    yield helper, solo
    helper.close()
    solo.close()


@pytest.fixture(scope="module")
def default_forms():
    """(product default, solo by size): above 16 384 tuples the default is the helper-wave form."""
    auto = fabgpu.Context(device=0)
    solo = fabgpu.Context(device=0, flags=fabgpu.FLAG_PAIR_SOLO)
    yield auto, solo
    auto.close()
    solo.close()


def _be(x):
    return int(x).to_bytes(32, "big")


def _cols(rows):
    return [np.frombuffer(b"".join(row[c] for row in rows), dtype=np.uint8).reshape(-1, 32).copy() for c in range(5)]


def _check(pair, cols, expect=None):
    a, b = pair
    bits_a, st_a = a.p256_verify_batch(*cols)
    bits_b, st_b = b.p256_verify_batch(*cols)
    want = coracle.verify_batch(*cols)
    assert (st_a == want).all(), np.nonzero(st_a != want)[0][:20]
    assert (bits_a == (want == 0)).all()
    assert (st_a == st_b).all() and (bits_a == bits_b).all()
    if expect is not None:
        assert (want == np.asarray(expect, dtype=np.uint8)).all()
    return want


def _sign(d, e, k):
    """(r, s) for private key d, digest value e (any 256-bit value: ECDSA reduces it mod n) and nonce k, low-S."""
    r = po.pt_mul(k, (po.GX, po.GY))[0] % po.N
    s = (e + r * d) * pow(k, -1, po.N) % po.N
    if not po.is_low_s(s):
        s = po.N - s
    return r, s


def _valid_row(rng, d=None, e=None):
    while True:
        dd = d if d is not None else int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) + 1
        ee = e if e is not None else int.from_bytes(bytes(rng.integers(0, 256, size=32, dtype=np.uint8)), "big")
        k = int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) + 3
        r, s = _sign(dd, ee, k)
        if r and s:
            Q = po.pt_mul(dd, (po.GX, po.GY))
            return [_be(Q[0]), _be(Q[1]), _be(ee), _be(r), _be(s)]


def test_bench_shaped_block(default_forms):
    n = 30000
    b = fabgpu.synth_batch(n, seed=20260921, invalid_permille=10)
    cols = [b[k] for k in ("qx", "qy", "e", "r", "s")]
    want = _check(default_forms, cols)
    assert ((want == 0) == (b["kind"] == 0)).all()


@pytest.mark.parametrize("n", [16385, 16511, 32767, 32768])
def test_partial_last_tiles(default_forms, n):
    b = fabgpu.synth_batch(n, seed=n, invalid_permille=30)
    _check(default_forms, [b[k] for k in ("qx", "qy", "e", "r", "s")])


@pytest.mark.parametrize("n", [1, 33, 127, 129, 257])
def test_small_batches_on_the_lds_table(forms, n):
    b = fabgpu.synth_batch(n, seed=7 * n, invalid_permille=100)
    _check(forms, [b[k] for k in ("qx", "qy", "e", "r", "s")])


def test_recoding_edge_scalars(forms):
    """Valid signatures whose u2 = r / s is n - 2 (the scalar whose product the main wave takes from the table) and the other
    recoding edges, each beside a signature of the same key with another s."""
    rng = np.random.default_rng(11)
    targets = scalar_sets.edge_u2_targets()
    assert len(targets) == 30
    rows, expect = [], []
    for u2 in targets:
        for _ in range(200):
            k = int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) + 1
            r = po.pt_mul(k, (po.GX, po.GY))[0] % po.N
            s = r * pow(u2, -1, po.N) % po.N
            if r == 0 or not po.is_low_s(s):
                continue
            e = int.from_bytes(bytes(rng.integers(0, 256, size=32, dtype=np.uint8)), "big")
            d = (s * k - e) * pow(r, -1, po.N) % po.N
            if d == 0:
                continue
            Q = po.pt_mul(d, (po.GX, po.GY))
            rows.append([_be(Q[0]), _be(Q[1]), _be(e), _be(r), _be(s)])
            rows.append([_be(Q[0]), _be(Q[1]), _be(e), _be(r), _be((s + 1) % po.N or 1)])
            expect += [0, None]
            break
        else:
            raise AssertionError("no low-S signature for u2 = %x" % u2)
    want = _check(forms, _cols(rows))
    for i, x in enumerate(expect):
        if x is not None:
            assert want[i] == x, hex(targets[i // 2])


def test_u1_zero_and_digests_at_or_above_n(forms):
    """e = 0 and e = n give u1 = 0: S stays at infinity and the verdict rests on T alone; e >= n is reduced."""
    rng = np.random.default_rng(12)
    rows = []
    for e in (0, po.N, 0, po.N, po.N + 1, po.N + 5, (1 << 256) - 1, po.P, po.N - 1):
        rows.append(_valid_row(rng, e=e))
    bad = [list(r) for r in rows]
    for r in bad:
        r[2] = _be((int.from_bytes(r[2], "big") + 1) % (1 << 256))
    want = _check(forms, _cols(rows + bad))
    assert (want[:len(rows)] == 0).all() and (want[len(rows):] != 0).all()


def test_range_and_curve_gates(forms):
    rng = np.random.default_rng(13)
    base = _valid_row(rng)
    qx, qy = int.from_bytes(base[0], "big"), int.from_bytes(base[1], "big")
    cases = []
    for r in (0, po.N, po.N + 1, (1 << 256) - 1, po.P):
        cases.append([base[0], base[1], base[2], _be(r), base[4]])
    for s in (0, po.N, po.N - 1, po.HALF_N, po.HALF_N + 1, (1 << 256) - 1):
        cases.append([base[0], base[1], base[2], base[3], _be(s)])
    cases.append([base[0], _be((qy + 1) % po.P), base[2], base[3], base[4]])      # off the curve
    cases.append([_be(qx + po.P) if qx + po.P < (1 << 256) else _be(po.P), base[1], base[2], base[3], base[4]])   # x out of the field
    cases.append([base[0], _be(po.P + qy) if po.P + qy < (1 << 256) else _be(po.P), base[2], base[3], base[4]])  # y out of the field
    cases.append([_be(0), _be(0), base[2], base[3], base[4]])
    cases.append([_be(0), _be(0), base[2], _be(0), base[4]])                      # range and curve gates together
    cases.append(base)
    _check(forms, _cols(cases))


def test_mixed_wavefronts(forms):
    """Every wave's 32 signatures mix valid lanes with range-gated, off-curve and wrong-math ones, across several tiles."""
    rng = np.random.default_rng(14)
    n = 700
    b = fabgpu.synth_batch(n, seed=99, invalid_permille=0)
    cols = [b[k].copy() for k in ("qx", "qy", "e", "r", "s")]
    for i in range(n):
        m = i % 7
        if m == 1:
            cols[3][i] = np.frombuffer(_be(0), np.uint8)
        elif m == 2:
            cols[4][i] = np.frombuffer(_be(po.N), np.uint8)
        elif m == 3:
            cols[1][i, 31] ^= 1
        elif m == 4:
            cols[2][i, 0] ^= 0x80
        elif m == 5 and rng.random() < 0.5:
            cols[4][i] = np.frombuffer(_be(po.N - int.from_bytes(cols[4][i].tobytes(), "big")), np.uint8)   # high S
    want = _check(forms, cols)
    assert (want != 0).any() and (want == 0).any()
