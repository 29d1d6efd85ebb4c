"""The LDS-table pair kernels with the table of odd multiples built by co-Z additions (the default) against the build by general
additions they replace (FABGPU_FLAG_PAIR_TABLE_ADD), in the helper-wave and the one-wave form, and all four against the CPU oracle:
verdict words and status bytes bit for bit.  Rows: valid low-S signatures whose u2 puts each of the eight table entries into the top
window with both signs of the fold (scalars of tests/scalar_sets.py), u2 = 2 and u2 = n - 2 (the doubling of entry 0), u1 = 0, a Q off
the curve and a Q out of the field - spread over synthetic rows (1 % tampered), so that gated and valid lanes share wavefronts."""
import ctypes
import random

import numpy as np
import pytest

import bccsp_sw_oracle as po
import coracle
import fabgpu
import scalar_sets

pytestmark = pytest.mark.gpu

LDS = fabgpu.FLAG_PAIR_TABLE_LDS
G = (po.GX, po.GY)


@pytest.fixture(scope="module")
def forms():
    f = {"helper": fabgpu.Context(device=0, flags=LDS),
         "helper-add": fabgpu.Context(device=0, flags=LDS | fabgpu.FLAG_PAIR_TABLE_ADD),
         "solo": fabgpu.Context(device=0, flags=LDS | fabgpu.FLAG_PAIR_SOLO),
         "solo-add": fabgpu.Context(device=0, flags=LDS | fabgpu.FLAG_PAIR_SOLO | fabgpu.FLAG_PAIR_TABLE_ADD)}
    yield f
    for c in f.values():
        c.close()


def _be(x):
    return int(x).to_bytes(32, "big")


def top_entry_and_sign(u2):
    """What p256_odd4.h makes of u2: k = u2 or n - u2, whichever is odd; the top window reads entry k >> 253."""
    even = u2 % 2 == 0
    k = po.N - u2 if even else u2
    return k >> 253, even


def _row_for_u2(rng, u2):
    """A valid low-S signature whose u2 = r / s is the given scalar."""
    for _ in range(400):
        k = rng.randrange(1, po.N)
        r = po.pt_mul(k, G)[0] % po.N
        s = r * pow(u2, -1, po.N) % po.N
        if r == 0 or not po.is_low_s(s):
            continue
        e = rng.randrange(1 << 256)
        d = (s * k - e) * pow(r, -1, po.N) % po.N
        if d == 0:
            continue
        Q = po.pt_mul(d, G)
        return [_be(Q[0]), _be(Q[1]), _be(e), _be(r), _be(s)]
    raise AssertionError("no low-S signature for u2 = %x" % u2)


def _row_for_e(rng, e):
    """A valid low-S signature over the digest e (e = 0 or n: u1 = 0)."""
    while True:
        d, k = rng.randrange(1, po.N), rng.randrange(1, po.N)
        r = po.pt_mul(k, G)[0] % po.N
        s = pow(k, -1, po.N) * (e + r * d) % po.N
        if r == 0 or s == 0:
            continue
        if not po.is_low_s(s):
            s = po.N - s
        Q = po.pt_mul(d, G)
        return [_be(Q[0]), _be(Q[1]), _be(e), _be(r), _be(s)]


@pytest.fixture(scope="module")
def special_rows():
    """(row, expected status): computed once, shared by every size."""
    rng = random.Random(20261021)
    pool = scalar_sets.edge_u2_targets() + scalar_sets.adversarial_u2s(rng)
    by_top = {}
    for u2 in pool:
        by_top.setdefault(top_entry_and_sign(u2), u2)
    assert sorted(by_top) == [(t, s) for t in range(8) for s in (False, True)], sorted(by_top)   # every entry on top, both signs
    rows = [(_row_for_u2(rng, by_top[key]), 0) for key in sorted(by_top)]
    rows += [(_row_for_u2(rng, 2), 0), (_row_for_u2(rng, po.N - 2), 0)]                       # PAIR_DBL of entry 0, both signs
    rows += [(_row_for_e(rng, 0), 0), (_row_for_e(rng, po.N), 0)]                              # u1 = 0: the comb adds nothing
    base = rows[0][0]
    qx, qy = int.from_bytes(base[0], "big"), int.from_bytes(base[1], "big")
    rows.append(([base[0], _be((qy + 1) % po.P), base[2], base[3], base[4]], 4))               # Q off the curve
    rows.append(([_be(qx + po.P) if qx + po.P < (1 << 256) else _be(po.P), base[1], base[2], base[3], base[4]], 4))   # x >= p
    rows.append(([base[0], _be((1 << 256) - 1), base[2], base[3], base[4]], 4))                # y >= p
    return rows


def _verify_words(ctx, cols):
    """(verdict words as the kernel left them, status bytes) through the host-pointer C ABI."""
    n = cols[0].shape[0]
    words = np.zeros((n + 63) // 64, dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    p8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    rc = ctx._L.fabgpu_p256_verify_batch(ctx._h, n, *(p8(c) for c in cols), words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), p8(st))
    assert rc == 0
    return words, st


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 257])
def test_coz_table_against_the_table_by_additions_and_the_oracle(forms, special_rows, n):
    """A single pair, a partial wavefront, a full tile, a tile plus one, two tiles plus one.  A batch with room for them holds every
    special row (gated ones between valid ones); a smaller batch runs once per special row."""
    b = fabgpu.synth_batch(n, seed=10000 + n, invalid_permille=10)
    names = ("qx", "qy", "e", "r", "s")
    if n >= len(special_rows):
        placements = [[(i * n // len(special_rows), sp) for i, sp in enumerate(special_rows)]]
    else:
        placements = [[(j % n, sp)] for j, sp in enumerate(special_rows)]
    for placed in placements:
        cols = [b[k].copy() for k in names]
        for pos, (row, _) in placed:
            for c in range(5):
                cols[c][pos] = np.frombuffer(row[c], dtype=np.uint8)
        want = coracle.verify_batch(*cols)
        for pos, (_, st) in placed:
            assert want[pos] == st, (pos, want[pos], st)
        got = {m: _verify_words(c, cols) for m, c in forms.items()}
        for m, (words, st) in got.items():
            print(n, m, "mismatches against the oracle", int((st != want).sum()))
        for m, (words, st) in got.items():
            assert (st == want).all(), (m, np.nonzero(st != want)[0][:20])
            assert (fabgpu.unpack_bits(words, n) == (want == 0)).all(), m
            assert (st == got["helper-add"][1]).all() and (words == got["helper-add"][0]).all(), m
