"""Cases for the eight-lanes-per-signature form of the registered-key P-384 verification (test_p384_wide_host.py, test_p384_wide_gpu.py)
and what p384_ref.py says about them.

Everything here is Python integers over p384_ref.py; nothing is shared with csrc/.  The form cuts u1 G + u2 Q into eight partial sums -
lane j takes the 8-bit windows 6 j .. 6 j + 5 of both scalars - and joins them in a tree (lanes j ^ 1, j ^ 2, j ^ 4).  Any pair (u1, u2)
is reachable through the raw entry: pick s, r = u2 s mod n, e = u1 s mod n.  Such a row answers 1 unless it arranges x(R) = r: then
s = r / u2, kept only when it is low.  A case is (name, key, e, r, s, id kind); its expected status is p384_ref.status of exactly that
row, behind the rule for an id that names no live key.  Computed once per process (functools.lru_cache) and never changed.
"""
import functools
import random

import p384_ref as R

N, G = R.N, R.G
LANES, PER_LANE = 8, 6
LIVE, WRONG_GEN, ABOVE_HWM, RETIRED = "live", "wrong generation", "slot at the high-water mark", "retired"


@functools.lru_cache(maxsize=None)
def keys():
    """name -> (d, Q): the generator, +-2^48 G, +-2^96 G, +-2^192 G (partial sums of different lanes that are equal or opposite), one
    random key, and one more that the device test registers and retires"""
    rng = random.Random(3848)
    out = {"G": 1, "A": 2**48, "-A": N - 2**48, "B": 2**96, "-B": N - 2**96, "C": 2**192, "-C": N - 2**192, "-G": N - 1,
           "K": rng.randrange(1, N), "gone": rng.randrange(1, N)}
    return {k: (d, R.mul(d, G)) for k, d in out.items()}


def windows(digits):
    """{window: digit} -> the scalar"""
    return sum(d << (8 * w) for w, d in digits.items())


def lane_of(w):
    return w // PER_LANE


def _row(key, u1, u2, s):
    q = keys()[key][1]
    return (q[0], q[1], u1 * s % N, u2 * s % N, s)


def _hit(key, u1, u2):
    """the row whose r is x(u1 G + u2 Q) mod n, or None (the sum is at infinity, r is zero or s comes out high)"""
    q = keys()[key][1]
    pt = R.add(R.mul(u1, G), R.mul(u2, q))
    if pt is None or u2 == 0:
        return None
    r = pt[0] % N
    s = r * pow(u2, -1, N) % N
    if r == 0 or s == 0 or s > R.HALF_N:
        return None
    return (q[0], q[1], u1 * s % N, r, s)


def _flip_e(row, bit):
    return row[:2] + (row[2] ^ (1 << bit),) + row[3:]


@functools.lru_cache(maxsize=None)
def crafted():
    """[(name, key, (qx, qy, e, r, s), id kind)]"""
    rng = random.Random(384806)
    out = []

    def add(name, key, row, kind=LIVE):
        out.append((name, key, row, kind))

    def hit_with_twin(name, key, make):
        """make() -> (u1, u2), drawn again until the arranged row has a low s; the row, and its twin with one bit of e flipped"""
        for _ in range(64):
            row = _hit(key, *make())
            if row is not None:
                add(name + ": x(R) = r", key, row)
                add(name + ": one bit of e flipped", key, _flip_e(row, rng.randrange(256)))
                return
        raise AssertionError("no low s for " + name)

    def digits(ws):
        return windows({w: rng.randrange(1, 255) for w in ws})

    every = range(LANES * PER_LANE)
    # lane idle: all twelve digits of one lane zero; all lanes idle but one; u1 = 0 and u2 in a single window
    for j in range(LANES):
        rest = [w for w in every if lane_of(w) != j]
        hit_with_twin("lane %d idle" % j, "K", lambda: (digits(rest), digits(rest)))
        add("lane %d idle, any s" % j, "K", _row("K", digits(rest), digits(rest), rng.randrange(1, R.HALF_N)))
        mine = [w for w in every if lane_of(w) == j]
        hit_with_twin("only lane %d" % j, "K", lambda: (digits(mine), digits(mine)))
    for w in (0, 17, 47):
        hit_with_twin("u1 = 0, u2 in window %d" % w, "K", lambda: (0, digits([w])))
    # tree doubling: equal partial sums meet at level 1 (lanes 0 / 1), 2 (0 / 2), 3 (0 / 4)
    for key, sh, lvl in (("A", 48, 1), ("B", 96, 2), ("C", 192, 3)):
        def dbl():
            d = rng.randrange(1, 256)
            return d << sh, d
        hit_with_twin("doubling at level %d" % lvl, key, dbl)
        add("doubling at level %d, any s" % lvl, key, _row(key, 1 << sh, 1, rng.randrange(1, R.HALF_N)))
    # ... and at level 2 from two lanes that are not lane 0: lane 1 holds 2^48 A = 2^96 G, lane 2 holds 2^96 G
    hit_with_twin("doubling at level 2, lanes 1 / 2", "A", lambda: (lambda d: (d << 96, d << 48))(rng.randrange(1, 256)))
    # tree cancellation: opposite partial sums give infinity inside the tree, joined with live sums afterwards
    # (the node where the two meet covers lanes 0 .. 2^level - 1, which are otherwise idle; at level 3 that node is the root)
    for key, sh, lvl in (("-A", 48, 1), ("-B", 96, 2), ("-C", 192, 3)):
        def cancel():
            d = rng.randrange(1, 256)
            live = [w for w in every if lane_of(w) >= 2**lvl]
            return (d << sh) + digits(live[:PER_LANE * 2]), d + digits(live[-PER_LANE:])
        if lvl < 3:
            hit_with_twin("infinity at level %d, live sums behind it" % lvl, key, cancel)
        d = rng.randrange(1, 256)
        add("infinity at the root from level %d" % lvl, key, _row(key, d << sh, d, rng.randrange(1, R.HALF_N)))
    ds = [rng.randrange(1, 256) for _ in range(4)]                   # all eight lanes cancel pairwise: infinity at the root
    add("eight lanes cancel pairwise", "-A", _row("-A", sum(d << (96 * i + 48) for i, d in enumerate(ds)), sum(d << (96 * i) for i, d in enumerate(ds)),
                                                   rng.randrange(1, R.HALF_N)))
    # in-lane doubling and cancellation: Q = +-G with equal digits in one window
    for w in (0, 23, 47):
        hit_with_twin("in-lane doubling, window %d" % w, "G", lambda: (lambda k: (k, k))(rng.randrange(1, 256) << (8 * w)))
        k = rng.randrange(1, 256) << (8 * w)
        add("in-lane cancellation, window %d" % w, "-G", _row("-G", k, k, rng.randrange(1, R.HALF_N)))
    # real signatures under those same keys, each beside a twin with one bit of e flipped
    signed = []
    for key in ("G", "A", "-A", "B", "-C", "K"):
        d, q = keys()[key]
        while True:
            e = rng.randrange(2**384)
            sg = R.sign(d, e, rng.randrange(1, 2**40))      # (a short nonce: the reference multiplies bit by bit; u1 and u2 are full size)
            if sg:
                break
        row = (q[0], q[1], e, sg[0], R.low_s(sg[1]))
        signed.append((key, row))
        add("signature under " + key, key, row)
        add("signature under " + key + ", one bit of e flipped", key, _flip_e(row, rng.randrange(384)))
    # gate rows: r or s equal to 0, equal to n, above n
    key, row = signed[-1]
    for what, r, s in (("r = 0", 0, row[4]), ("s = 0", row[3], 0), ("r = n", N, row[4]), ("s = n", row[3], N),
                       ("r > n", N + 1 + rng.randrange(2**384 - N - 1), row[4]), ("s > n", row[3], N + 1 + rng.randrange(2**384 - N - 1)),
                       ("s high", row[3], N - row[4])):
        add("gate: " + what, key, row[:3] + (r, s))
    # ids that name no live key: the row is a valid one under the key it once named - and a gate row, whose status goes first
    for kind in (WRONG_GEN, ABOVE_HWM):
        add("stale id (%s)" % kind, key, row, kind)
    d, q = keys()["gone"]
    sg = None
    while not sg:
        e = rng.randrange(2**256)
        sg = R.sign(d, e, rng.randrange(1, 2**40))      # (a short nonce: the reference multiplies bit by bit; u1 and u2 are full size)
    gone = (q[0], q[1], e, sg[0], R.low_s(sg[1]))
    add("stale id (retired)", "gone", gone, RETIRED)
    add("stale id (retired), s high", "gone", gone[:4] + (N - gone[4],), RETIRED)
    add("stale id (wrong generation), r = 0", key, row[:3] + (0, row[4]), WRONG_GEN)
    return tuple(out)


def expected(row, kind=LIVE):
    """p384_ref.status, behind the id rule: a row whose id names no live key answers 4 unless the gate refuses it first"""
    st = R.status(*row)
    return st if kind == LIVE or st in (R.ST_HIGH_S, R.ST_RANGE) else R.ST_OFF_CURVE


@functools.lru_cache(maxsize=None)
def crafted_expected():
    return tuple(expected(row, kind) for _n, _k, row, kind in crafted())


@functools.lru_cache(maxsize=None)
def random256():
    """256 seeded signatures over four of the keys, every second one tampered (a bit of e, r or s); ([(key, row)], statuses)"""
    rng = random.Random(384256)
    names = ("K", "G", "A", "-B")
    out = []
    for i in range(256):
        d, q = keys()[names[i % 4]]
        sg = None
        while not sg:
            e = rng.randrange(2**384 if i % 3 else 2**256)
            sg = R.sign(d, e, rng.randrange(1, 2**40))      # (a short nonce: the reference multiplies bit by bit; u1 and u2 are full size)
        t = [q[0], q[1], e, sg[0], R.low_s(sg[1])]
        if i & 1:
            t[2 + rng.randrange(3)] ^= 1 << rng.randrange(380)
        out.append((names[i % 4], tuple(t)))
    st = tuple(R.status(*row) for _k, row in out)
    assert st.count(0) == 128 and st.count(1) >= 64
    return tuple(out), st


def case_line(row, key_ok=True):
    """one line of csrc/hosttest_p384_wide.cpp's input"""
    return "%x %x %x %x %x %d\n" % (row + (1 if key_ok else 0,))


def write_cases(path):
    """the crafted list and the 256 signatures as a case file (`make sanitize-p384-wide P384_WIDE_CASES=...`)"""
    with open(path, "w") as f:
        for _n, _k, row, kind in crafted():
            f.write(case_line(row, kind == LIVE))
        for _k, row in random256()[0]:
            f.write(case_line(row))


if __name__ == "__main__":
    import sys
    write_cases(sys.argv[1])
