"""Rows for the 16-bit comb tables of registered P-384 keys (csrc/p384_tables16.h): signatures whose scalars u1 = e / s and u2 = r / s
are CHOSEN, so that the 24-window sum of verify_core_keyed meets what its 16-bit digits can meet - an accumulator equal to the entry
(the doubling branch), opposite to it (infinity), zero digits, digits with one zero byte (the entries the builders copy), all-ones digits.
Shared by test_p384_tables16_host.py and test_p384_tables16_gpu.py; statuses come from Python integers (p384_ref.py)."""
import functools
import random

import p384_keyed_cases as K
import p384_ref as R

N, G = R.N, R.G
DIGITS16 = (1, 2, 0x00FF, 0x0100, 0x0101, 0x7FFF, 0x8000, 0xFF00, 0xFFFF)


def windows16(digits):
    """{window: 16-bit digit} -> the scalar"""
    return sum(d << (16 * w) for w, d in digits.items())


@functools.lru_cache(maxsize=None)
def keys():
    """name -> (d, Q): the generator, its opposite and two of the keyed cases' random keys"""
    out = {"G": 1, "-G": N - 1, "K1": K.keys()[0][0], "K2": K.keys()[1][0]}
    return {k: (d, R.mul(d, G)) for k, d in out.items()}


def row_for(key, u1, u2, want_valid=True):
    """(qx, qy, e, r, s) with e / s = u1 and r / s = u2 under `key`, s low.  want_valid: r = x(u1 G + u2 Q) mod n, or None when that
    cannot be had (the sum is at infinity, or s comes out high); otherwise r is arbitrary and the row is an arithmetic reject."""
    q = keys()[key][1]
    if want_valid:
        pt = R.add(R.mul(u1, G), R.mul(u2, q))
        if pt is None:
            return None
        r = pt[0] % N
    else:
        r = (u1 * 0x9E3779B97F4A7C15 + u2 + 12345) % N or 1
    s = r * pow(u2, -1, N) % N
    if r == 0 or s == 0 or s > R.HALF_N:
        if want_valid:
            return None
        r = N - r                                  # (s -> n - s: the same u2, a low s)
        s = r * pow(u2, -1, N) % N
    return (q[0], q[1], u1 * s % N, r, s)


def _first(key, make):
    """the first of make(0), make(1), ... that gives a valid row with a low s"""
    for t in range(64):
        u1, u2 = make(t)
        row = row_for(key, u1 % N, u2 % N)
        if row:
            return row
    raise AssertionError("no low-s row in 64 tries")


@functools.lru_cache(maxsize=None)
def steering(generic=("K1", "K2")):
    """[(name, key, row)]; generic: the keys of the rows that steer by their digits alone"""
    rng = random.Random(38416)
    full = lambda: windows16({w: rng.randrange(1, 65536) for w in range(24)}) % N
    out = []
    # Q = G, the same digit in the same single window of u1 and u2: the accumulator d B meets the entry d B - pt_add doubles
    for w in (0, 11, 23):
        out.append(("doubling in window %d" % w, "G", _first("G", lambda t, w=w: (windows16({w: 0x1234 + t}),) * 2)))
    # ... with Q = -G the two entries are opposite: the sum is at infinity, whatever r says
    for w in (0, 11, 23):
        u = windows16({w: 0x4321})
        out.append(("infinity in window %d" % w, "-G", row_for("-G", u, u, want_valid=False)))
    # Q = G and u1 = u2 with every digit set: the same entry twice per window, on an accumulator that is never that entry
    out.append(("full digits, Q = G, u1 = u2", "G", _first("G", lambda t: (windows16({w: 0x0101 * (w + 1) + t for w in range(24)}),) * 2)))
    for key in generic:
        # zero 16-bit digits: entry 1 is loaded and the sum dropped
        out.append(("u1 has zero digits", key, _first(key, lambda t: (windows16({0: 7 + t, 5: 0xBEEF, 23: 0x00FF}), full()))))
        out.append(("u2 has zero digits", key, _first(key, lambda t: (full(), windows16({1: 9 + t, 12: 0xFFFF, 22: 0x8000})))))
        out.append(("u1 is one digit", key, _first(key, lambda t: (windows16({11: 0x8000 + t}), full()))))
        # digits with one zero byte: the entries both builders COPY from the 8-bit table
        out.append(("low bytes zero", key, _first(key, lambda t: (windows16({w: (1 + (w + t) % 255) << 8 for w in range(24)}),
                                                                  windows16({w: (255 - (w + t) % 255) << 8 for w in range(23)})))))
        out.append(("high bytes zero", key, _first(key, lambda t: (windows16({w: 1 + (w + t) % 255 for w in range(24)}),
                                                                   windows16({w: 255 - (w + t) % 255 for w in range(24)})))))
        # all-ones digits (the last entry of every window); the top window stays below n
        out.append(("all-ones digits", key, _first(key, lambda t: (windows16({**{w: 0xFFFF for w in range(23)}, 23: 0x7FFF - t}),
                                                                   windows16({**{w: 0xFFFF for w in range(23)}, 23: 0x3FFF - t})))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def steering_expected(generic=("K1", "K2")):
    st = tuple(R.status(*row) for _n, _k, row in steering(generic))
    assert st.count(1) == 3 and st.count(0) == len(st) - 3
    return st


@functools.lru_cache(maxsize=None)
def signed(n, seed, key_names=("K1", "K2")):
    """n rows signed by the named keys in turn; every fourth one has a bit flipped in e, r or s in turn: ([(key, row)], statuses)"""
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        key = key_names[i % len(key_names)]
        d, q = keys()[key]
        t = list(K._signed(rng, d, q, rng.randrange(2**384)))
        if i % 4 == 3:
            t[2 + (i // 4) % 3] ^= 1 << rng.randrange(380)
        rows.append((key, tuple(t)))
    return tuple(rows), tuple(R.status(*row) for _k, row in rows)
