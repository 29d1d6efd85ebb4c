"""The LDS-table pair kernels with the all-odd recoding of u2 over a table of odd multiples (63 windows: the default) against the Booth
form they replace (FABGPU_FLAG_PAIR_BOOTH4: 65 windows over j*Q), in the helper-wave and the one-wave form, and all four against the
CPU oracle: verdict words and status bytes bit for bit.  Rows: a valid low-S signature for every u2 of tests/pair_odd_targets.py
(u2 = n - 2 and u2 = 2, the one scalar whose product is computed apart, among them), each beside a twin with s + 1; rows that fail each
gate; synthetic rows around them, so that gated and valid lanes share wavefronts."""
import ctypes

import numpy as np
import pytest

import bccsp_sw_oracle as po
import coracle
import fabgpu
import pair_odd_targets as pt

pytestmark = pytest.mark.gpu

LDS = fabgpu.FLAG_PAIR_TABLE_LDS


@pytest.fixture(scope="module")
def forms():
    """{helper, solo} x {default, PAIR_BOOTH4}, all forced onto the LDS table so that batches of any size take it."""
    f = {"helper": fabgpu.Context(device=0, flags=LDS),
         "helper-booth4": fabgpu.Context(device=0, flags=LDS | fabgpu.FLAG_PAIR_BOOTH4),
         "solo": fabgpu.Context(device=0, flags=LDS | fabgpu.FLAG_PAIR_SOLO),
         "solo-booth4": fabgpu.Context(device=0, flags=LDS | fabgpu.FLAG_PAIR_SOLO | fabgpu.FLAG_PAIR_BOOTH4)}
    yield f
    for c in f.values():
        c.close()


def _be(x):
    return int(x).to_bytes(32, "big")


def _cols(rows):
    return [np.frombuffer(b"".join(row[c] for row in rows), dtype=np.uint8).reshape(-1, 32).copy() for c in range(5)]


def _verify_words(ctx, cols):
    """(verdict words as the kernel left them, status bytes) through the host-pointer C ABI."""
    n = cols[0].shape[0]
    words = np.zeros((n + 63) // 64, dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    p8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    rc = ctx._L.fabgpu_p256_verify_batch(ctx._h, n, *(p8(c) for c in cols), words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), p8(st))
    assert rc == 0
    return words, st


def _check(contexts, cols):
    want = coracle.verify_batch(*cols)
    n = len(want)
    first = None
    for name, ctx in contexts.items():
        words, st = _verify_words(ctx, cols)
        assert (st == want).all(), (name, np.nonzero(st != want)[0][:20])
        assert (fabgpu.unpack_bits(words, n) == (want == 0)).all(), name
        if first is None:
            first = (words, st)
        assert (words == first[0]).all() and (st == first[1]).all(), name
    return want


@pytest.fixture(scope="module")
def pool():
    """(rows, expected status or None per row, index of the first gate row).  Edge rows: for every target u2 a valid low-S signature
    with r / s = u2, and its twin with s + 1.  Gate rows: r = 0, s = 0, r >= n, Q off the curve, a coordinate >= p."""
    rng = np.random.default_rng(20261021)
    rows, expect = [], []
    for u2 in pt.device_u2():
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
    first_gate = len(rows)
    base = rows[0]
    qx, qy = int.from_bytes(base[0], "big"), int.from_bytes(base[1], "big")
    gates = [[base[0], base[1], base[2], _be(0), base[4]],                                  # r = 0
             [base[0], base[1], base[2], base[3], _be(0)],                                  # s = 0
             [base[0], base[1], base[2], _be(po.N), base[4]],                               # r = n
             [base[0], base[1], base[2], _be((1 << 256) - 1), base[4]],                     # r > n
             [base[0], _be((qy + 1) % po.P), base[2], base[3], base[4]],                    # Q off the curve
             [_be(qx + po.P) if qx + po.P < (1 << 256) else _be(po.P), base[1], base[2], base[3], base[4]],   # x >= p
             [base[0], _be(qy + po.P) if qy + po.P < (1 << 256) else _be(po.P), base[2], base[3], base[4]],   # y >= p
             [_be(0), _be(0), base[2], _be(0), _be(0)]]                                     # every gate at once
    rows += gates
    expect += [None] * len(gates)
    return rows, expect, first_gate


def _batch(pool, n, stride):
    """n synthetic rows (10 % invalid) with the pool's rows written over every stride-th of them, as many as fit; gate rows first among
    them when not all fit, so that every size has gated lanes beside valid ones.  Returns (columns, {row index: expected status})."""
    rows, expect, first_gate = pool
    b = fabgpu.synth_batch(n, seed=31 * n + 7, invalid_permille=100)
    cols = [b[k].copy() for k in ("qx", "qy", "e", "r", "s")]
    order = list(range(len(rows)))
    slots = list(range(0, n, stride))
    if len(slots) < len(order):
        order = order[:2] + order[first_gate:] + order[2:first_gate]              # u2 = 1 and its twin, the gates, then the other edges
    placed = {}
    for slot, j in zip(slots, order):
        for c in range(5):
            cols[c][slot] = np.frombuffer(rows[j][c], dtype=np.uint8)
        if expect[j] is not None:
            placed[slot] = expect[j]
    return cols, placed


@pytest.mark.parametrize("n", [1, 33, 127, 129, 257])
def test_small_batches(forms, pool, n):
    cols, placed = _batch(pool, n, 2)
    want = _check(forms, cols)
    for i, x in placed.items():
        assert want[i] == x


def test_every_target_and_every_gate_in_mixed_wavefronts(forms, pool):
    rows, expect, first_gate = pool
    assert len(rows) <= len(range(0, 700, 3))                                     # every pool row fits at stride 3
    cols, placed = _batch(pool, 700, 3)
    assert len(placed) == sum(x is not None for x in expect)                      # no target left out
    want = _check(forms, cols)
    for i, x in placed.items():
        assert want[i] == x, i
    gate_slots = [3 * j for j in range(first_gate, len(rows))]
    assert (want[gate_slots] != 0).all() and len(set(want[gate_slots])) >= 2      # range and curve statuses both occur
    # a wavefront of the pair kernel serves 32 rows: those that hold the gate rows hold valid rows too
    for w in {i // 32 for i in gate_slots}:
        assert (want[w * 32:(w + 1) * 32] == 0).any(), w


def test_size_selected_path_is_the_new_form(forms, pool):
    """16 385 rows on a context without flags: the batch size alone selects the LDS table, helper waves and the all-odd recoding."""
    cols, placed = _batch(pool, 16385, 61)
    auto = fabgpu.Context(device=0)
    try:
        want = _check({"default": auto, "helper-booth4": forms["helper-booth4"]}, cols)
    finally:
        auto.close()
    assert len(placed) == sum(x is not None for x in pool[1])
    for i, x in placed.items():
        assert want[i] == x, i
