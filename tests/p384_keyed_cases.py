"""Tuples for the registered-key P-384 tests (test_p384_keyed_host.py, test_p384_keyed_gpu.py) and what p384_ref.py says about them.

Everything here is Python integers over p384_ref.py; nothing is shared with csrc/.  A row is (qx, qy, e, r, s); its expected status is
p384_ref.status of exactly that row.  The expensive parts are computed once per process (functools.lru_cache) and never changed.
"""
import functools
import json
import os
import random

import p384_ref as R

P, N = R.P, R.N
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WINDOWS, DIGITS, ENTRY_WORDS = 48, 256, 24


def want(rows):
    return [R.status(*t) for t in rows]


@functools.lru_cache(maxsize=None)
def keys():
    """five key pairs (d, Q)"""
    rng = random.Random(384008)
    out = []
    for _ in range(5):
        d = rng.randrange(1, N)
        out.append((d, R.mul(d, R.G)))
    return tuple(out)


def kat_rows():
    return [tuple(int(v[k], 16) for k in ("qx", "qy")) + (R.hash_to_int(bytes.fromhex(v["digest"])), int(v["r"], 16), int(v["s"], 16))
            for v in json.load(open(os.path.join(GOLD, "p384_kats.json")))["vectors"]]


def _signed(rng, d, q, e):
    while True:
        sg = R.sign(d, e, rng.randrange(1, N))
        if sg:
            return (q[0], q[1], e, sg[0], R.low_s(sg[1]))


@functools.lru_cache(maxsize=None)
def mixed257():
    """257 rows over the five keys, each key with valid, bit-flipped and gate-refused rows; (rows, statuses)"""
    rng = random.Random(384257)
    rows = []
    for i in range(257):
        d, q = keys()[i % 5]
        kind = (i // 5) % 3
        t = list(_signed(rng, d, q, rng.randrange(2**384 if rng.random() < 0.5 else 2**256)))
        if kind == 1:
            t[2 + rng.randrange(3)] ^= 1 << rng.randrange(380)
        elif kind == 2:
            which = (i // 15) % 5
            if which == 0:
                t[4] = N - t[4]                  # high s
            elif which == 1:
                t[3] = 0
            elif which == 2:
                t[4] = 0
            elif which == 3:
                t[3] = N + rng.randrange(2**384 - N)
            else:
                t[4] = N
        rows.append(tuple(t))
    st = want(rows)
    assert st.count(0) >= 80 and st.count(1) >= 40 and st.count(2) >= 20 and st.count(3) >= 20
    return tuple(rows), tuple(st)


@functools.lru_cache(maxsize=None)
def exceptional():
    """Rows that steer the 48-window sum into pt_add's exceptional cases whatever order the windows are taken in; (rows, statuses).

    u1 = u2 = k = d * 2^(8 w): one nonzero window each, the same one, the same digit.  With Q = G the two table entries are the same
    point: the second addition is P + P.  r = x(2 k G) mod n, s = r / k, e = r (u1 = e / s = k, u2 = r / s = k): status 0; only
    (w, d) whose s is low are kept.  With Q = -G the same rows sum to infinity: status 1.
    Then u1 = 0 (e = 0 and e = n), u2 below 2^8 and below 2^64 (every upper window zero), e >= n in 48 bytes, and x(R) in [n, p):
    the second acceptance branch."""
    rng = random.Random(384999)
    negG = R.neg(R.G)
    rows, fixed = [], []
    for w in (0, 23, 47):
        kept = 0
        for d in (1, 255):
            k = d << (8 * w)
            r = R.mul(2 * k, R.G)[0] % N
            s = r * pow(k, -1, N) % N
            if s > R.HALF_N or r == 0:
                continue
            kept += 1
            rows.append((R.G[0], R.G[1], r, r, s)); fixed.append(0)
            rows.append((negG[0], negG[1], r, r, s)); fixed.append(1)
        assert kept >= 1, "no (w, d) with a low s for window %d" % w
    d, q = keys()[0]
    dinv = pow(d, -1, N)
    for e in (0, N):                                             # u1 = 0: the sum is u2 Q alone
        while True:
            kk = rng.randrange(1, N)
            r = R.mul(kk, R.G)[0] % N
            s = r * pow(kk * dinv % N, -1, N) % N
            if 0 < s <= R.HALF_N:
                break
        rows.append((q[0], q[1], e, r, s)); fixed.append(0)
        rows.append((q[0], q[1], e, r, (s - 1) or 1)); fixed.append(1)
    for bound in (2**8, 2**64):                                  # u2 small: R = kk G = u1 G + u2 Q, u1 = kk - u2 d
        while True:
            u2 = rng.randrange(1, bound)
            kk = rng.randrange(1, N)
            r = R.mul(kk, R.G)[0] % N
            s = r * pow(u2, -1, N) % N
            if r and 0 < s <= R.HALF_N:
                break
        e = (kk - u2 * d) * s % N
        rows.append((q[0], q[1], e, r, s)); fixed.append(0)
        rows.append((q[0], q[1], e ^ 1, r, s)); fixed.append(1)
    while True:                                                  # e >= n in 48 bytes: reduced once
        e = N + rng.randrange(2**384 - N)
        t = _signed(rng, d, q, e)
        if t:
            break
    rows.append(t); fixed.append(0)
    rows.append(t[:2] + (e - N,) + t[3:]); fixed.append(0)
    k = 1                                                        # x(R) = n + k < p: r = x - n verifies, r + 1 does not
    while R.lift_x(N + k) is None:
        k += 1
    Rp, r = R.lift_x(N + k), k
    s = rng.randrange(1, R.HALF_N)
    e = rng.randrange(2**384)
    wv = pow(s, -1, N)
    u1, u2 = e * wv % N, r * wv % N
    q2 = R.mul(pow(u2, -1, N), R.add(Rp, R.neg(R.mul(u1, R.G))))
    assert R.on_curve(*q2) and r + N < P
    rows.append((q2[0], q2[1], e, r, s)); fixed.append(0)
    rows.append((q2[0], q2[1], e, r + 1, s)); fixed.append(1)
    st = want(rows)
    assert st == fixed, (st, fixed)
    return tuple(rows), tuple(st)


def comb_table(q):
    """T[w][d] = d * 2^(8 w) * q as Python integers: a list of 48 lists of 256 affine points (entry 0: None)"""
    out = []
    base = q
    for _ in range(WINDOWS):
        row, acc = [None], None
        for _d in range(1, DIGITS):
            acc = R.add(acc, base)
            row.append(acc)
        out.append(row)
        base = R.add(acc, base)
    return out


def mont_words(v):
    """the canonical Montgomery form of v mod p as twelve little-endian 32-bit words"""
    m = v * 2**384 % P
    return [(m >> (32 * i)) & 0xFFFFFFFF for i in range(12)]


def comb_words(q):
    """the table of csrc/p384_tables.h CombTab384 for q, as a flat list of 48 * 256 * 24 words"""
    out = []
    for row in comb_table(q):
        for pt in row:
            out.extend([0] * ENTRY_WORDS if pt is None else mont_words(pt[0]) + mont_words(pt[1]))
    return out
