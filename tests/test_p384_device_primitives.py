"""The P-384 field, scalar, inversion, digit and point code (csrc/p384.h, p384_dev.h, p384_tables.h, p384_tables16.h, p384_wide.h), one
primitive at a time, against Python integers - with the rare branches forced.

Why: on the device every P-384 primitive is otherwise reached only through whole verifications, which feed it random-looking operands.
Two things stay unseen that way.  (1) mont_mul ends with sel384(r, t[12] != 0 || br == 0, d, r); the `br == 0` half decides only when
the sum before the subtraction lies in [m, 2^384), a window of about 2^128 values for p and 2^190 for n that random operands never hit
(mod_add has the same select, with probability about 2^-256).  (2) under __HIP_DEVICE_COMPILE__ mont_mul is one out-of-line function,
and pt_add calls it (through pt_dbl) from inside its only divergent branch, the P + P case: a call under a partial exec mask.

The reference is Python integers and the affine group law of tests/p384_ref.py - never the host C bodies.  Every comparison is
equality of integers.  Two halves, like tests/test_device_primitives.py:
  * the CPU half (not marked gpu) holds an integer model of the CIOS loop, pre(a, b, m) = (a b + q m) / 2^384, from which the operand
    classes below are SOLVED FOR; it checks that the comparators flag what they must, asserts the precondition and the census of every
    generator (no case is dropped after the device has answered), and sends the crafted classes through the hooks of
    libfabgpu_hosttest.so - which closes hole (1) for the host compilation that the audit relies on;
  * the GPU half runs the hooks "P-384 primitives on many wavefronts" of csrc/gputest.hip: one launch per (op, modulus, form) with all
    classes concatenated, and one parametrised case per op and class.

Operand classes
  pre_subtraction_window  t in [m + 1, 2^384): m + 1, m + 2, 2^384 - 1, 2^384 - 2, the midpoint, the value that differs from m in one
                      word only - the highest word of m that is not all ones (the top word of both moduli is 0xffffffff, so nothing
                      in the window differs from m there) - and 200 random ones.  a random in [2^300, m), b = t 2^384 / a mod m,
                      kept only if pre(a, b, m) == t.  pre is congruent to t and below a b / 2^384 + m, so it is t or t - m; with
                      a >= 2^300 and b of full size a b / 2^384 exceeds t - m < 2^384 - m and pre == t: every pair is kept, and
                      the generator asserts kept == generated.  Built for the raw product, for the square (where t 2^384 is a
                      quadratic residue: both moduli are 3 mod 4), for the plain product and square (the Montgomery forms of the
                      operands are the solved pair) and for to_mont (a = t / 2^384, second factor 2^768 mod m).  from_mont cannot
                      have it: pre(a, 1, m) = (a + q m) / 2^384 <= (m - 1 + (2^384 - 1) m) / 2^384 < m.  The census says all this.
  carry_word          t = 2^384, 2^384 + 1 .. 2^384 + 3 and random t >= 2^384 (word 12 set, the low words zero or near zero), found by
                      drawing a until pre(a, b, m) == t; and products whose result is 0, 1 and m - 1.
  add_sub_edges       a + b in {m - 1, m, m + 1, 2^384 - 1, 2^384, 2^384 + 1, 2m - 2}, a - b in {0, 1, -1, -(m - 1)}, from random a.
  limb_ends           the _limb_patterns of tests/test_p384_host.py, all against all (45 of the 2 916 pairs for p and 51 for n land in
                      the window as well: counted and asserted in the CPU half).
  random              2^15 pairs.
  wide_values         for add384, sub384, lt384, eq384, is_zero, fn_reduce_once, range_status, the identity and the 32-byte form:
                      values of the whole of [0, 2^384) - m, m +- 1, 2^384 - 1, the half order, the half order + 1, p - n +- 1, limb
                      ends - all against all; one_bit_apart: a and a with one bit flipped, for every bit.
  inverse             0, 1, 2, m - 1, m - 2, (m + 1) / 2, 2^k and 2^-k for k stepping by 13, 2 048 random values; the launch starts
                      with wavefronts in which zeros sit beside live inputs and ends in a partial wavefront.
  points              from a pool of multiples of G with random Z: random_z (8 192), p_plus_p, p_plus_minus_p, infinity on the left,
                      on the right and on both sides, G and -G, small coordinates (affine x small; X or Y small as the Montgomery
                      words the device holds, through a chosen Z: a square root for X as p = 3 mod 4, a cube root for Y as p = 2
                      mod 3), and divergent_doubling: whole wavefronts with no, one (at several lanes), every other, all lanes
                      P + P, and P + P, P + (-P) and infinity mixed; the launch ends in a partial wavefront.
  x_equals_r          both acceptance branches (x = n + k < p by lift_x, r = k and r = k + 1), r in {p - n - 1, p - n, p - n + 1},
                      infinity.  A point with X == r Z^2 only for another representative cannot exist among canonical inputs: the
                      census asserts every input word value is below p.
"""
import ctypes
import os
import random

import numpy as np
import pytest

import p384_ref as R
from test_p384_host import _limb_patterns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, N = R.P, R.N
W = 1 << 384
M32 = (1 << 32) - 1
RINV_P = pow(W, -1, P)
MODULI = {"p": P, "n": N}
FID = {"p": 1, "n": 0}
NRANDOM = 1 << 15
WAVE = 64
gpu = pytest.mark.gpu


# ---- the integer model of the CIOS loop -------------------------------------------------------------------------------------------------
def pre(a, b, m):
    """The sum before the final subtraction: (a b + q m) / 2^384 with q = -a b / m mod 2^384."""
    q = (-a * b * pow(m, -1, W)) % W
    assert (a * b + q * m) % W == 0
    return (a * b + q * m) >> 384


def cios(a, b, m):
    """The same sum word by word, as p384.h forms it: (t after every outer step)."""
    n0 = (-pow(m, -1, 1 << 32)) & M32
    t, steps = 0, []
    for i in range(12):
        t += a * ((b >> (32 * i)) & M32)
        t = (t + ((t * n0) & M32) * m) >> 32
        steps.append(t)
    return steps


def one_word_above(m):
    """The value of the window that differs from m in one word only: the highest word of m that is not all ones, set to all ones."""
    k = max(i for i in range(12) if (m >> (32 * i)) & M32 != M32)
    return m | (M32 << (32 * k))


def window_targets(m, rng, nrandom=200):
    t = [m + 1, m + 2, W - 1, W - 2, (m + W) // 2, one_word_above(m)] + [rng.randrange(m + 1, W) for _ in range(nrandom)]
    assert all(m < v < W for v in t) and len(set(t[:6])) == 6
    return t


def window_pairs(m, rng):
    """([(a, b, t)] with pre(a, b, m) == t, how many were generated)"""
    kept, generated = [], 0
    for t in window_targets(m, rng):
        a = rng.randrange(1 << 300, m)
        b = t * W * pow(a, -1, m) % m
        generated += 1
        if pre(a, b, m) == t:
            kept.append((a, b, t))
    assert len(kept) == generated, (len(kept), generated)
    return kept, generated


def window_squares(m, rng):
    """([(a, t)] with pre(a, a, m) == t, how many targets had a root at all)"""
    assert m % 4 == 3
    kept, residues = [], 0
    for t in window_targets(m, rng):
        c = t * W % m
        r = pow(c, (m + 1) // 4, m)
        if r * r % m != c:
            continue
        residues += 1
        kept += [(a, t) for a in (r, m - r) if a >= 1 << 300 and pre(a, a, m) == t]
    assert residues > 0 and len(kept) >= residues, (len(kept), residues)
    return kept, residues


def window_to_mont(m, rng):
    """[(a, t)] with pre(a, 2^768 mod m, m) == t: to_mont(a) passes through the window"""
    r2 = W * W % m
    kept = [(a, t) for a, t in ((t * pow(W, -1, m) % m, t) for t in window_targets(m, rng)) if pre(a, r2, m) == t]
    assert kept
    return kept


def window_from_mont(m, rng):
    """from_mont multiplies by 1: pre(a, 1, m) < m for every a < m, so nothing can be kept - the census reports the zero."""
    kept = [(a, t) for a, t in ((t * W % m, t) for t in window_targets(m, rng)) if pre(a, 1, m) == t]
    assert not kept and pre(m - 1, 1, m) < m
    return kept


def carry_pairs(m, rng):
    """{what: [(a, b)]}: the sum before the subtraction is exactly t >= 2^384, and products whose result is 0, 1, m - 1"""
    targets = [W, W + 1, W + 2, W + 3] + [rng.randrange(W, W + (m >> 1)) for _ in range(64)]
    carry = []
    for t in targets:
        for _ in range(400):
            a = rng.randrange(1 << 300, m)
            b = t * W * pow(a, -1, m) % m
            if pre(a, b, m) == t:
                carry.append((a, b))
                break
    assert len(carry) == len(targets), (len(carry), len(targets))
    results = [(0, 0), (0, m - 1), (m - 1, 0)]
    for _ in range(8):
        a = rng.randrange(1, m)
        results += [(a, 0), (0, a), (a, W * pow(a, -1, m) % m), (a, (m - W * pow(a, -1, m)) % m)]
    assert {a * b * pow(W, -1, m) % m for a, b in results} == {0, 1, m - 1}
    return carry + results


def add_sub_edges(m, rng, each=16):
    out = []
    for s in (m - 1, m, m + 1, W - 1, W, W + 1, 2 * m - 2):
        lo, hi = max(0, s - (m - 1)), min(m - 1, s)
        for _ in range(each):
            a = rng.randrange(lo, hi + 1)
            out.append((a, s - a))
    for d in (0, 1, -1, -(m - 1)):
        lo, hi = max(0, d), min(m - 1, m - 1 + d)
        for _ in range(each):
            a = rng.randrange(lo, hi + 1)
            out.append((a, a - d))
    assert {a + b for a, b in out} >= {m - 1, m, m + 1, W - 1, W, W + 1, 2 * m - 2} and {a - b for a, b in out} >= {0, 1, -1, 1 - m}
    return out


def wide_specials():
    s = {0, 1, 2, P - 1, P, P + 1, N - 1, N, N + 1, W - 1, W - 2, R.HALF_N, R.HALF_N + 1, R.HALF_N - 1, P - N, P - N - 1, P - N + 1, 1 << 383,
         (1 << 256) - 1, 1 << 256, int("ffffffff00000000" * 6, 16), int("00000000ffffffff" * 6, 16)}
    for k in range(1, 12):
        s |= {1 << (32 * k), (1 << (32 * k)) - 1}
    assert all(0 <= v < W for v in s)
    return sorted(s)


def inverse_vectors(m, rng):
    """{class: [a]} in launch order: four wavefronts with zeros beside live inputs, one of zeros only, the structured values, the random
    ones; the last wavefront is partial."""
    v = {"wave_zero_beside_live": [], "wave_all_zero": [0] * WAVE}
    for w in range(4):
        v["wave_zero_beside_live"] += [rng.randrange(1, m) if i % (w + 2) else 0 for i in range(WAVE)]
    st = [0, 1, 2, m - 1, m - 2, (m + 1) // 2]
    for k in range(0, 384, 13):
        st += [(1 << k) % m, pow(1 << k, -1, m)]
    v["structured"] = st
    v["random_partial_last_wave"] = [rng.randrange(1, m) for _ in range(2048)]
    total = sum(len(x) for x in v.values())
    assert total % WAVE != 0 and all(0 <= a < m for x in v.values() for a in x)
    for w in range(4):
        lanes = v["wave_zero_beside_live"][WAVE * w:WAVE * (w + 1)]
        assert 0 < lanes.count(0) < WAVE
    return v


# ---- the field and scalar ops -----------------------------------------------------------------------------------------------------------
FIELD_OPS = {"mont_mul": 0, "mod_add": 1, "mod_sub": 2, "to_mont": 3, "from_mont": 4, "mul": 5, "sqr": 6, "inv": 7, "reduce_once": 8, "add384": 9,
             "sub384": 10, "lt384": 11, "eq384": 12, "is_zero": 13, "range_status": 14, "ident": 15}
CONTRACT_OPS = ("mont_mul", "mod_add", "mod_sub", "to_mont", "from_mont", "mul", "sqr", "inv")          # operands in [0, m), both moduli
WIDE_OPS = ("reduce_once", "add384", "sub384", "lt384", "eq384", "is_zero", "range_status", "ident")     # operands in [0, 2^384)
UNARY = ("to_mont", "from_mont", "sqr", "inv", "reduce_once", "is_zero", "ident")


def range_status(r, s):
    """The gate of p384.h as integers: r or s zero: 3; s above the half order: 2; r not below n: 3; else 0."""
    if r == 0 or s == 0:
        return 3
    if s > R.HALF_N:
        return 2
    return 3 if r >= N else 0


def field_want(m, op, a, b):
    """(the 48-byte output, the flag word) of gputest_p384_field_op as integers"""
    ri = pow(W, -1, m)
    if op in ("lt384", "eq384", "is_zero", "range_status"):
        return a, {"lt384": int(a < b), "eq384": int(a == b), "is_zero": int(a == 0), "range_status": range_status(a, b)}[op]
    if op == "add384":
        return (a + b) % W, (a + b) >> 384
    if op == "sub384":
        return (a - b) % W, int(a < b)
    if op == "inv":
        return (pow(a, -1, m) if a else 0), 0
    return {"mont_mul": a * b * ri % m, "mod_add": (a + b) % m, "mod_sub": (a - b) % m, "to_mont": a * W % m, "from_mont": a * ri % m, "mul": a * b % m,
            "sqr": a * a % m, "reduce_once": a - N if a >= N else a, "ident": a}[op], 0


def field_errors(m, op, a, b, out, flag):
    """What is wrong with one answer: 'value' (wrong modulo m, or wrong outright for the ops that do not reduce), 'canonical' (right
    modulo m and not the representative of [0, m)), 'flag'."""
    want, wflag = field_want(m, op, a, b)
    errs = []
    if out != want:
        errs.append("canonical" if op in CONTRACT_OPS + ("reduce_once",) and (out - want) % m == 0 else "value")
    if flag != wflag:
        errs.append("flag")
    return errs


_vec_cache = {}


def field_vectors(mname, op, form=0):
    """{class: [(a, b)]} for one launch of gputest_p384_field_op, in launch order.  Operands of the contract ops lie in [0, m): asserted."""
    key = (mname, op, form)
    if key in _vec_cache:
        return _vec_cache[key]
    m = MODULI[mname]
    rng = random.Random("p384/%s/%s/%d" % key)
    ri = pow(W, -1, m)
    sp = _limb_patterns(m)
    v = {}
    if op == "mont_mul":
        v["pre_subtraction_window"] = [(a, b) for a, b, _ in window_pairs(m, rng)[0]]
        v["pre_subtraction_window_square"] = [(a, a) for a, _ in window_squares(m, rng)[0]]
        v["carry_word"] = carry_pairs(m, rng)
    elif op == "mul":            # the Montgomery forms of the operands are the solved pair: the inner product passes through the window
        v["pre_subtraction_window"] = [(a * ri % m, b * ri % m) for a, b, _ in window_pairs(m, rng)[0]]
        v["carry_word"] = [(a * ri % m, b * ri % m) for a, b in carry_pairs(m, rng)]
    elif op == "sqr":
        v["pre_subtraction_window"] = [(a * ri % m, 0) for a, _ in window_squares(m, rng)[0]]
    elif op == "to_mont":
        v["pre_subtraction_window"] = [(a, 0) for a, _ in window_to_mont(m, rng)]
    elif op == "from_mont":
        window_from_mont(m, rng)
    elif op in ("mod_add", "mod_sub"):
        v["add_sub_edges"] = add_sub_edges(m, rng)
    if op == "inv":
        v = {c: [(a, 0) for a in xs] for c, xs in inverse_vectors(m, rng).items()}
    elif op in CONTRACT_OPS:
        v["limb_ends"] = [(a, 0) for a in sp] if op in UNARY else [(a, b) for a in sp for b in sp]
        v["random"] = [(rng.randrange(m), 0 if op in UNARY else rng.randrange(m)) for _ in range(NRANDOM)]
    else:
        top = 1 << 256 if form else W                       # form 1: a is a 32-byte row
        ws = [x for x in wide_specials() if x < top]
        v["wide_values"] = [(a, b) for a in ws for b in wide_specials()]
        v["one_bit_apart"] = [(a, a ^ (1 << k)) for k in range(384) for a in (rng.randrange(top),)]
        v["random"] = [(rng.randrange(top), rng.randrange(W)) for _ in range(NRANDOM)]
        assert all(0 <= a < top and 0 <= b < W for xs in v.values() for a, b in xs)
    if op in CONTRACT_OPS:
        assert all(0 <= a < m and 0 <= b < m for xs in v.values() for a, b in xs)
    assert all(len(xs) > 0 for xs in v.values())
    _vec_cache[key] = v
    return v


def census(vecs):
    return {c: len(xs) for c, xs in vecs.items()}


_EDGES = ["limb_ends", "random"]
FIELD_CLASSES = {"mont_mul": ["pre_subtraction_window", "pre_subtraction_window_square", "carry_word"] + _EDGES,
                 "mul": ["pre_subtraction_window", "carry_word"] + _EDGES, "sqr": ["pre_subtraction_window"] + _EDGES,
                 "to_mont": ["pre_subtraction_window"] + _EDGES, "from_mont": _EDGES, "mod_add": ["add_sub_edges"] + _EDGES,
                 "mod_sub": ["add_sub_edges"] + _EDGES, "inv": ["wave_zero_beside_live", "wave_all_zero", "structured", "random_partial_last_wave"]}
FIELD_CLASSES.update({op: ["wide_values", "one_bit_apart", "random"] for op in WIDE_OPS})          # what field_vectors() makes: asserted below
FIELD_CASES = [(mn, op, 0, c) for op in CONTRACT_OPS for mn in ("p", "n") for c in FIELD_CLASSES[op]] + \
              [("n", op, 0, c) for op in WIDE_OPS for c in FIELD_CLASSES[op]] + \
              [("n", op, 1, c) for op in ("ident", "reduce_once") for c in FIELD_CLASSES[op]]
FIELD_IDS = ["%s-%s-%s-%s" % (op, mn, "e32" if form else "be48", c) for mn, op, form, c in FIELD_CASES]


# ---- digits -------------------------------------------------------------------------------------------------------------------------------
def digit_vectors():
    rng = random.Random("p384/digits")
    return {"wide_values": wide_specials(), "random": [rng.randrange(W) for _ in range(4096)]}


def digits_want(a):
    """take_top_nibble x 96, wide_digit(0 .. 47), take_low_byte x 48 (CombPtr384::take), take_low_half x 24 (CombPtr384x16::take)"""
    return [(a >> (380 - 4 * k)) & 15 for k in range(96)] + [(a >> (8 * w)) & 255 for w in range(48)] * 2 + [(a >> (16 * k)) & 0xffff for k in range(24)]


# ---- points -------------------------------------------------------------------------------------------------------------------------------
INF = (1, 1, 0)                 # pt_infinity(): X = Y = one, Z = 0 (plain integers here; the Montgomery form is taken when a row is packed)
_pool = []


def pool():
    """256 multiples of G: k0 G + i k1 G"""
    if not _pool:
        rng = random.Random("p384/pool")
        pt, step = R.mul(rng.randrange(1, N), R.G), R.mul(rng.randrange(1, N), R.G)
        for _ in range(256):
            _pool.append(pt)
            pt = R.add(pt, step)
        assert len({p[0] for p in _pool}) == 256 and all(R.on_curve(*p) for p in _pool)
    return _pool


def jac(pt, z):
    """an affine point as plain Jacobian integers with the given Z (None: infinity)"""
    if pt is None:
        return INF
    assert 0 < z < P
    return (pt[0] * z * z % P, pt[1] * z * z * z % P, z)


def affine(X, Y, Z):
    if Z % P == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def z_for_small_x(pt, xm):
    """Z with X = x Z^2 equal to the Montgomery word value xm (X plain = xm / 2^384), or None when that needs a non-residue"""
    z = R.sqrt_mod_p(xm * RINV_P * pow(pt[0], -1, P) % P)
    return z if z else None


def z_for_small_y(pt, ym):
    """Z with Y = y Z^3 equal to the Montgomery word value ym: p = 2 mod 3, every element has one cube root, c^((2p - 1) / 3)"""
    assert P % 3 == 2
    c = ym * RINV_P * pow(pt[1], -1, P) % P
    z = pow(c, (2 * P - 1) // 3, P)
    assert z * z * z % P == c
    return z


def small_coordinate_points(rng):
    """[(affine point, Z)]: affine x small; X or Y small as Montgomery words"""
    out, k = [], 0
    while len(out) < 8:
        k += 1
        pt = R.lift_x(k)
        if pt:
            out += [(pt, 1), (pt, rng.randrange(1, P))]
    for pt in pool()[:12]:
        xm = 1
        while z_for_small_x(pt, xm) is None:
            xm += 1
        out.append((pt, z_for_small_x(pt, xm)))
        out.append((pt, z_for_small_y(pt, 1 + len(out))))
        out.append((pt, z_for_small_y(pt, 1 << 32)))
    for pt, z in out[8:]:
        X, Y, _ = jac(pt, z)
        assert X * W % P <= 1 << 32 or Y * W % P <= 1 << 32
    return out


def _pp(rng, kind, mixed):
    """one row (first triple, second triple, what the sum must be) of the given kind; mixed: the second Z is one"""
    pl = pool()
    p = pl[rng.randrange(256)]
    z1 = rng.randrange(1, P)
    z2 = 1 if mixed else rng.randrange(1, P)
    if kind == "generic":
        q = pl[rng.randrange(256)]
        while q[0] == p[0]:
            q = pl[rng.randrange(256)]
        return (jac(p, z1), jac(q, z2), R.add(p, q))
    if kind == "p_plus_p":
        return (jac(p, z1), jac(p, z2), R.add(p, p))
    if kind == "p_plus_minus_p":
        return (jac(p, z1), jac(R.neg(p), z2), None)
    if kind == "infinity_left":
        return (INF, jac(p, z2), p)
    if kind == "infinity_right":
        return (jac(p, z1), INF, p)
    assert kind == "infinity_both"
    return (INF, (rng.randrange(P), rng.randrange(P), 0), None)


def divergent_waves(rng, mixed):
    """Whole wavefronts around the one divergent branch of pt_add: [row], in wavefront order"""
    kinds = ["infinity_left", "p_plus_p", "p_plus_minus_p", "generic"] + ([] if mixed else ["infinity_right", "infinity_both"])
    waves = [["generic"] * WAVE]
    for lane in (0, 1, 31, 32, 63):
        waves.append(["p_plus_p" if i == lane else "generic" for i in range(WAVE)])
    waves.append(["p_plus_p" if i % 2 == 0 else "generic" for i in range(WAVE)])
    waves.append(["p_plus_p" if i % 2 == 1 else "generic" for i in range(WAVE)])
    waves.append(["p_plus_p"] * WAVE)
    waves.append([kinds[(i + i // len(kinds)) % len(kinds)] for i in range(WAVE)])
    assert all(len(w) == WAVE for w in waves) and [w.count("p_plus_p") for w in waves[:9]] == [0, 1, 1, 1, 1, 1, 32, 32, 64]
    assert set(waves[9]) == set(kinds)
    return [_pp(rng, k, mixed) for w in waves for k in w]


POINT_OPS = {"dbl": 0, "add": 1, "madd": 2}
_ADD = ["divergent_doubling", "random_z", "p_plus_p", "p_plus_minus_p", "infinity_left", "infinity_right", "infinity_both", "g_and_minus_g",
        "small_coordinates", "partial_last_wave"]
POINT_CLASSES = {"dbl": ["random_z", "infinity", "g_and_minus_g", "small_coordinates", "partial_last_wave"], "add": _ADD,
                 "madd": [c for c in _ADD if c not in ("infinity_right", "infinity_both")]}          # what point_vectors() makes: asserted below


def point_vectors(op):
    """{class: [(first triple, second triple, the affine result)]} in launch order: divergent_doubling starts the launch (whole
    wavefronts), partial_last_wave ends it."""
    key = ("point", op)
    if key in _vec_cache:
        return _vec_cache[key]
    rng = random.Random("p384/point/" + op)
    pl = pool()
    mixed = op == "madd"
    v = {}
    if op == "dbl":
        def d(pt, z):
            return (jac(pt, z), jac(R.G, 1), R.add(pt, pt))
        v["random_z"] = [d(pl[rng.randrange(256)], rng.randrange(1, P)) for _ in range(8192)]
        v["infinity"] = [(INF, INF, None), ((rng.randrange(P), rng.randrange(P), 0), INF, None)]
        v["g_and_minus_g"] = [d(R.G, 1), d(R.neg(R.G), 1), d(R.G, rng.randrange(1, P)), d(R.neg(R.G), rng.randrange(1, P))]
        v["small_coordinates"] = [d(pt, z) for pt, z in small_coordinate_points(rng)]
        v["partial_last_wave"] = [d(pl[i], rng.randrange(1, P)) if i % 3 else (INF, INF, None) for i in range(37)]
    else:
        v["divergent_doubling"] = divergent_waves(rng, mixed)
        v["random_z"] = [_pp(rng, "generic", mixed) for _ in range(8192)]
        for kind in ("p_plus_p", "p_plus_minus_p", "infinity_left") + (() if mixed else ("infinity_right", "infinity_both")):
            v[kind] = [_pp(rng, kind, mixed) for _ in range(64)]
        g, ng = R.G, R.neg(R.G)
        zs = (lambda: 1) if mixed else (lambda: rng.randrange(1, P))
        v["g_and_minus_g"] = [(jac(a, rng.randrange(1, P)), jac(b, zs()), R.add(a, b)) for a in (g, ng, pl[0]) for b in (g, ng)] + \
                             [(jac(a, 1), jac(b, 1), R.add(a, b)) for a in (g, ng) for b in (g, ng)]
        sc = small_coordinate_points(rng)
        v["small_coordinates"] = [(jac(pt, z), jac(q, zs()), R.add(pt, q)) for (pt, z), q in zip(sc, pl)] + \
                                 [(jac(pt, z), jac(pt, zs()), R.add(pt, pt)) for pt, z in sc] + \
                                 [(jac(pt, z), jac(R.neg(pt), zs()), None) for pt, z in sc]
        if not mixed:
            v["small_coordinates"] += [(jac(q, zs()), jac(pt, z), R.add(pt, q)) for (pt, z), q in zip(sc, pl)]
        kinds = ["generic", "p_plus_p", "p_plus_minus_p", "infinity_left"]
        v["partial_last_wave"] = [_pp(rng, kinds[i % 4], mixed) for i in range(37)]
    rows = [r for xs in v.values() for r in xs]
    assert len(rows) % WAVE != 0
    for a, b, want in rows:                                  # the contract: canonical words; the mixed form's second Z is one
        assert all(0 <= c < P for c in a + b) and (not mixed or b[2] == 1)
        if op != "dbl":
            assert R.add(affine(*a), affine(*b)) == want
    _vec_cache[key] = v
    return v


def point_errors(want, raw, montgomery):
    """What is wrong with one answer X Y Z (raw: the integers as the hook gave them; montgomery: the device's words, x 2^384): 'range'
    (a coordinate not below p), 'infinity' (Z3 zero or not where it must not be), 'affine' (another point)."""
    errs = ["range"] if any(not 0 <= c < P for c in raw) else []
    X, Y, Z = ((c * RINV_P % P) if montgomery else c % P for c in raw)
    if (Z == 0) != (want is None):
        errs.append("infinity")
    elif want is not None and affine(X, Y, Z) != want:
        errs.append("affine")
    return errs


ON_CURVE_CLASSES = ["on_curve", "negated_y", "y_off", "x_off", "origin"]


def on_curve_vectors():
    rng = random.Random("p384/on_curve")
    pl = pool()
    v = {"on_curve": [(x, y, 1) for x, y in pl] + [(R.GX, R.GY, 1)], "negated_y": [(x, P - y, 1) for x, y in pl[:64]],
         "y_off": [(x, (y + 1 + rng.randrange(3)) % P, 0) for x, y in pl], "x_off": [((x + 1) % P, y, 0) for x, y in pl], "origin": [(0, 0, 0), (0, 1, 0), (1, 0, 0)]}
    for xs in v.values():
        assert all(0 <= x < P and 0 <= y < P and R.on_curve(x, y) == bool(w) for x, y, w in xs)
    return v


def x_equals_r_vectors():
    """{class: [(Jacobian triple, r, accept)]}; accept by the integer definition: not infinity and x mod n == r.  r in [0, n), canonical words."""
    rng = random.Random("p384/x_equals_r")
    pl = pool()

    def row(pt, r, z=None):
        t = jac(pt, z or rng.randrange(1, P))
        return (t, r, int(pt is not None and pt[0] % N == r))
    v = {"first_branch": [], "second_branch": [], "r_edges": [], "infinity": []}
    for pt in pl[:128]:
        v["first_branch"] += [row(pt, pt[0] % N), row(pt, (pt[0] + 1) % N), row(pt, pt[0] % N, 1)]
    found, k = [], 0
    while len(found) < 4:
        if R.lift_x(N + k):
            found.append(k)
        k += 1
    for k in found:
        pt = R.lift_x(N + k)
        assert N + k < P
        v["second_branch"] += [row(pt, k), row(pt, k + 1), row(R.neg(pt), k), row(pt, k, 1)]
    for r in (P - N - 1, P - N, P - N + 1):
        v["r_edges"].append(row(pl[0], r))
        for x in (r, r + N):
            pt = R.lift_x(x) if x < P else None
            if pt:
                v["r_edges"] += [row(pt, r), row(pt, (r + 1) % N)]
    v["infinity"] = [(INF, 1, 0), ((0, 0, 0), 0, 0), ((0, 0, 0), 5, 0), ((rng.randrange(P), rng.randrange(P), 0), rng.randrange(1, N), 0)]
    assert [w for _, _, w in v["second_branch"]].count(1) == 12 and any(w for _, _, w in v["r_edges"])
    for xs in v.values():
        assert xs and all(0 <= r < N and all(0 <= c < P for c in t) for t, r, _ in xs)       # canonical: one representative per coordinate
    return v


# ---- the libraries ------------------------------------------------------------------------------------------------------------------------
def b48(v):
    return int(v).to_bytes(48, "big")


def be_rows(xs, width=48):
    return np.frombuffer(b"".join(int(x).to_bytes(width, "big") for x in xs), dtype=np.uint8).reshape(-1, width).copy()


def ints_of(arr, width=48):
    raw = arr.tobytes()
    return [int.from_bytes(raw[i:i + width], "big") for i in range(0, len(raw), width)]


def words_of(v):
    return [(v >> (32 * i)) & M32 for i in range(12)]


def int_of_words(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def flatten(vecs):
    flat, spans = [], {}
    for cls, vs in vecs.items():
        spans[cls] = (len(flat), len(flat) + len(vs))
        flat += vs
    return flat, spans


@pytest.fixture(scope="module")
def H():
    p = os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_hosttest.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(p)


@pytest.fixture(scope="module")
def dev():
    return ctypes.CDLL(os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_gputest.so"))


def _h(fn, *args, n=48):
    out = ctypes.create_string_buffer(n)
    fn(*args, out)
    return out.raw


# =========================================================================================================================================
# CPU half
# =========================================================================================================================================
@pytest.mark.parametrize("mname", ["p", "n"])
def test_cios_model_and_where_random_operands_land(mname):
    m = MODULI[mname]
    rng = random.Random("p384/model/" + mname)
    below, window, above = 0, 0, 0
    for k, (a, b) in enumerate([(rng.randrange(m), rng.randrange(m)) for _ in range(2000)] + [(m - 1, m - 1), (0, 0), (1, 1), (m - 1, 1)]):
        steps = cios(a, b, m)
        assert steps[-1] == pre(a, b, m) and all(t < 2 * m for t in steps)          # the bound the header claims: word 12 is 0 or 1
        t = steps[-1]
        assert (t - m if t >= m else t) == a * b * pow(W, -1, m) % m
        if k < 2000:
            below, window, above = below + (t < m), window + (m <= t < W), above + (t >= W)
    print("p384 census %s: 2 000 random products: %d below m, %d in [m, 2^384), %d with word 12 set" % (mname, below, window, above))
    assert window == 0 and above > 0                    # why the class has to be solved for


@pytest.mark.parametrize("mname", ["p", "n"])
def test_generators_reach_what_they_claim(mname):
    m = MODULI[mname]
    rng = random.Random("p384/gen/" + mname)
    kept, generated = window_pairs(m, rng)
    assert len(kept) == generated == 206 and all(m < pre(a, b, m) == t < W and a >= 1 << 300 for a, b, t in kept)
    assert {m + 1, m + 2, W - 1, W - 2, (m + W) // 2, one_word_above(m)} <= {t for _, _, t in kept}
    om = one_word_above(m)
    assert m < om < W and sum(1 for x, y in zip(words_of(om), words_of(m)) if x != y) == 1
    sq, residues = window_squares(m, rng)
    assert all(m < pre(a, a, m) == t < W for a, t in sq)
    tm = window_to_mont(m, rng)
    assert all(m < pre(a, W * W % m, m) < W for a, _ in tm)
    fm = window_from_mont(m, rng)
    print("p384 census %s pre_subtraction_window: mul kept %d of %d generated; square %d operands over %d residue targets; to_mont %d; from_mont %d "
          "(cannot: pre(a, 1, m) < m)" % (mname, len(kept), generated, len(sq), residues, len(tm), len(fm)))
    le = sum(1 for a, b in field_vectors(mname, "mont_mul")["limb_ends"] if m <= pre(a, b, m) < W)
    print("p384 census %s limb_ends: %d of %d pairs land in [m, 2^384)" % (mname, le, len(field_vectors(mname, "mont_mul")["limb_ends"])))
    assert le == {"p": 45, "n": 51}[mname]
    cp = carry_pairs(m, rng)
    assert sum(1 for a, b in cp if pre(a, b, m) >= W) >= 68 and {W, W + 1} <= {pre(a, b, m) for a, b in cp}
    for a in (1, 2):                                      # a small first factor does not reach the window: a b / 2^384 < 1, the sum is t - m
        assert pre(a, (m + 1) * W * pow(a, -1, m) % m, m) == 1
    ed = add_sub_edges(m, rng)
    assert any(a + b >= W for a, b in ed) and any(m <= a + b < W for a, b in ed) and any(a + b < m for a, b in ed)
    for op in CONTRACT_OPS + WIDE_OPS:
        c = census(field_vectors(mname, op))
        print("p384 census %s %s: %s" % (mname, op, c))
        assert list(c) == FIELD_CLASSES[op] and all(k > 0 for k in c.values())
        if op == "inv":
            continue
        assert c["random"] == NRANDOM
    for op in ("mont_mul", "mul", "sqr", "to_mont"):
        assert field_vectors(mname, op)["pre_subtraction_window"]
    assert "pre_subtraction_window" not in field_vectors(mname, "from_mont")
    assert census(field_vectors(mname, "mont_mul"))["pre_subtraction_window"] == 206
    assert census(field_vectors("n", "ident", 1))["wide_values"] > 0 and all(a < 1 << 256 for xs in field_vectors("n", "ident", 1).values() for a, _ in xs)


def test_field_comparator_flags_what_it_must():
    for m in (P, N):
        a = m - 5
        b = W * pow(a, -1, m) % m                         # a b / 2^384 = 1
        want, _ = field_want(m, "mont_mul", a, b)
        assert want == 1 and field_errors(m, "mont_mul", a, b, want, 0) == []
        for k in range(12):
            assert field_errors(m, "mont_mul", a, b, want ^ (1 << (32 * k)), 0) == ["value"]          # a word off by one
        assert want + m < W and field_errors(m, "mont_mul", a, b, want + m, 0) == ["canonical"]       # right modulo m, not canonical
        assert field_errors(m, "mod_add", 1, m - 1, m, 0) == ["canonical"] and field_errors(m, "mod_add", 1, m - 1, 0, 0) == []
        assert field_errors(m, "mod_sub", 0, 1, W - 1, 0) == ["value"]
        assert field_errors(m, "mont_mul", a, b, want, 1) == ["flag"]
    assert field_errors(N, "reduce_once", N + 3, 0, N + 3, 0) == ["canonical"] and field_errors(N, "reduce_once", N + 3, 0, 3, 0) == []
    assert field_errors(N, "add384", W - 1, 1, 0, 0) == ["flag"] and field_errors(N, "add384", W - 1, 1, 0, 1) == []
    assert field_errors(N, "sub384", 0, 1, W - 1, 0) == ["flag"] and field_errors(N, "lt384", 3, 3, 3, 1) == ["flag"]
    assert [range_status(r, s) for r, s in ((0, 1), (1, 0), (1, R.HALF_N), (1, R.HALF_N + 1), (N, 1), (N, N), (N - 1, 1), (W - 1, W - 1))] == [3, 3, 0, 2, 3, 2, 0, 2]
    for r, s in ((1, 1), (N - 1, R.HALF_N), (N, 5), (7, R.HALF_N + 1), (0, 9)):       # the precedence of the reference's status
        st = R.status(R.GX, R.GY, 1, r, s)
        assert range_status(r, s) == (st if st in (R.ST_HIGH_S, R.ST_RANGE) else 0)


def test_point_generators_and_comparator():
    rng = random.Random("p384/point/cmp")
    for op in POINT_OPS:
        v = point_vectors(op)
        print("p384 census point %s: %s" % (op, census(v)))
        assert list(v) == POINT_CLASSES[op] and all(len(xs) > 0 for xs in v.values()) and len(v["random_z"]) == 8192
        if op != "dbl":
            assert list(v)[0] == "divergent_doubling" and len(v["divergent_doubling"]) == 10 * WAVE
    pt = pool()[3]
    want = R.add(pt, pt)
    z = rng.randrange(1, P)
    good = [c * W % P for c in jac(want, z)]
    assert point_errors(want, good, True) == [] and point_errors(want, list(jac(want, z)), False) == []
    for k in range(3):
        for wd in range(12):
            bad = list(good)
            bad[k] ^= 1 << (32 * wd)
            assert point_errors(want, bad, True) in (["affine"], ["range", "affine"], ["infinity"], ["range", "infinity"])
    xm = 1
    while z_for_small_x(want, xm) is None:
        xm += 1
    small = [c * W % P for c in jac(want, z_for_small_x(want, xm))]
    assert small[0] == xm and point_errors(want, small, True) == []
    assert point_errors(want, [small[0] + P] + small[1:], True) == ["range"]          # right, with one coordinate not below p
    assert point_errors(want, [good[0], good[1], 0], True) == ["infinity"] and point_errors(None, good, True) == ["infinity"]
    assert point_errors(None, [5, 7, 0], True) == []
    print("p384 census on_curve: %s   x_equals_r: %s" % (census(on_curve_vectors()), census(x_equals_r_vectors())))
    assert len(digits_want(W - 1)) == 216 and digits_want(1 << 380)[:2] == [1, 0] and digits_want(0xabcd)[96:98] == [0xcd, 0xab]


@pytest.mark.parametrize("mname", ["p", "n"])
def test_host_compilation_on_the_crafted_field_classes(H, mname):
    """mont_mul, to_mont (a product by 2^768 mod m), mod_add and mod_sub of the host compilation, raw, on every class but `random` cut to
    2 048 pairs; the plain-integer hooks on the classes solved for their inner product."""
    m, f = MODULI[mname], FID[mname]
    r2 = W * W % m
    seen, failed = {}, {}
    for op, call in (("mont_mul", lambda a, b: _h(H.hosttest_p384_mont_mul, f, b48(a), b48(b))),
                     ("to_mont", lambda a, b: _h(H.hosttest_p384_mont_mul, f, b48(a), b48(r2))),
                     ("from_mont", lambda a, b: _h(H.hosttest_p384_mont_mul, f, b48(a), b48(1))),
                     ("mod_add", lambda a, b: _h(H.hosttest_p384_mod_addsub, f, 0, b48(a), b48(b))),
                     ("mod_sub", lambda a, b: _h(H.hosttest_p384_mod_addsub, f, 1, b48(a), b48(b)))):
        for cls, xs in field_vectors(mname, op).items():
            xs = xs[:2048] if cls == "random" else xs
            bad = [(a, b, e) for a, b, e in ((a, b, field_errors(m, op, a, b, int.from_bytes(call(a, b), "big"), 0)) for a, b in xs) if e]
            seen[(op, cls)] = len(xs)
            if bad:
                failed[(op, cls)] = (len(bad), bad[0])
    plain = {"mul": (H.hosttest_p384_fp_op, 0) if f else (H.hosttest_p384_fn_op, 0), "sqr": (H.hosttest_p384_fp_op, 1) if f else None,
             "inv": (H.hosttest_p384_fp_op, 5) if f else (H.hosttest_p384_fn_op, 1)}
    for op, hook in plain.items():
        if hook is None:
            continue
        for cls, xs in field_vectors(mname, op).items():
            xs = xs[:512] if op == "inv" else xs[:2048] if cls == "random" else xs
            bad = [(a, b, e) for a, b, e in ((a, b, field_errors(m, op, a, b, int.from_bytes(_h(hook[0], hook[1], b48(a), b48(a if op == "sqr" else b)), "big"), 0))
                                             for a, b in xs) if e]
            seen[(op, cls)] = len(xs)
            if bad:
                failed[(op, cls)] = (len(bad), bad[0])
    print("p384 census host %s: %s" % (mname, seen))
    # every class is run before the verdict, so that a failure names all that notice
    assert not failed, "classes that fail: %s; first of each: %s" % (sorted(failed), failed)
    assert seen[("mont_mul", "pre_subtraction_window")] == 206 and seen[("mod_add", "add_sub_edges")] == 176


def test_host_compilation_on_the_wide_range_ops(H):
    for cls, xs in field_vectors("n", "reduce_once").items():
        for a, _ in xs[:2048]:
            assert int.from_bytes(_h(H.hosttest_p384_fn_op, 2, b48(a), b48(0)), "big") == field_want(N, "reduce_once", a, 0)[0], cls


def _host_point(H, op, a, b):
    raw = _h(H.hosttest_p384_pt_op, POINT_OPS[op], b"".join(map(b48, a)), b"".join(map(b48, b)), n=144)
    return [int.from_bytes(raw[48 * k:48 * k + 48], "big") for k in range(3)]


@pytest.mark.parametrize("op", list(POINT_OPS))
def test_host_compilation_on_the_crafted_point_classes(H, op):
    for cls, rows in point_vectors(op).items():
        bad = [(i, e) for i, e in ((i, point_errors(want, _host_point(H, op, a, b), False)) for i, (a, b, want) in enumerate(rows[:640])) if e]
        assert not bad, (op, cls, len(bad), bad[:3])


def test_host_compilation_on_the_acceptance_classes(H):
    for cls, rows in x_equals_r_vectors().items():
        for t, r, want in rows:
            assert H.hosttest_p384_x_equals_r(b"".join(map(b48, t)), b48(r)) == want, (cls, t, r)


def test_the_gpu_test_library_exports_the_p384_hooks_and_the_product_does_not():
    import subprocess

    import fabgpu
    fabgpu.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_gputest.so")], capture_output=True,
                        text=True, check=True).stdout
    assert {"gputest_p384_field_op", "gputest_p384_digits", "gputest_p384_point_op"} <= {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    nm = subprocess.run(["nm", "-D", "--defined-only", fabgpu.lib_path()], capture_output=True, text=True, check=True).stdout
    assert not [ln for ln in nm.splitlines() if "gputest" in ln]


# =========================================================================================================================================
# GPU half
# =========================================================================================================================================
_run_cache = {}


def field_run(dev, mname, op, form):
    """One launch per (modulus, op, form) with every class concatenated; cached for the cases that read it."""
    key = (mname, op, form)
    if key not in _run_cache:
        flat, spans = flatten(field_vectors(mname, op, form))
        n = len(flat)
        a, b = be_rows([x for x, _ in flat], 32 if form else 48), be_rows([y for _, y in flat])
        out = np.zeros((n, 48), dtype=np.uint8)
        flag = np.full(n, 0xdeadbeef, dtype=np.uint32)
        rc = dev.gputest_p384_field_op(FID[mname], FIELD_OPS[op], form, ctypes.c_uint32(n), _ptr(a), _ptr(b), _ptr(out), _ptr(flag))
        assert rc == 0, rc
        _run_cache[key] = (flat, spans, ints_of(out), flag.tolist())
    return _run_cache[key]


@gpu
@pytest.mark.parametrize("mname,op,form,cls", FIELD_CASES, ids=FIELD_IDS)
def test_p384_field_and_scalar_ops_on_device(dev, mname, op, form, cls):
    """Every op of gputest_p384_field_op: the raw Montgomery product, mod_add / mod_sub, the conversions, the plain product, square and
    inverse, fn_reduce_once, the 384-bit add / subtract / compare helpers, the gate - and the row loads and the store around them."""
    flat, spans, out, flag = field_run(dev, mname, op, form)
    lo, hi = spans[cls]
    assert hi > lo
    print("vectors %s %s %s: %d" % (mname, op, cls, hi - lo))
    bad = [(i - lo, e, flat[i]) for i, e in ((i, field_errors(MODULI[mname], op, flat[i][0], flat[i][1], out[i], flag[i])) for i in range(lo, hi)) if e]
    assert not bad, (len(bad), bad[:3])


@gpu
@pytest.mark.parametrize("cls", ["wide_values", "random"])
def test_p384_digit_accessors_on_device(dev, cls):
    """take_top_nibble (p384.h), wide_digit (p384_wide.h), take_low_byte (p384_tables.h) and take_low_half (p384_tables16.h)"""
    if "digits" not in _run_cache:
        flat, spans = flatten(digit_vectors())
        a = be_rows(flat)
        out = np.zeros((len(flat), 216), dtype=np.uint32)
        assert dev.gputest_p384_digits(ctypes.c_uint32(len(flat)), _ptr(a), _ptr(out)) == 0
        _run_cache["digits"] = (flat, spans, out.tolist())
    flat, spans, out = _run_cache["digits"]
    lo, hi = spans[cls]
    assert hi > lo
    bad = [(i - lo, flat[i]) for i in range(lo, hi) if out[i] != digits_want(flat[i])]
    assert not bad, (len(bad), bad[:3])


def pack_points(rows):
    """[(first triple, second slot as three integers already in the form the hook reads)] -> (n, 72) words"""
    return np.array([[w for c in t for w in words_of(c)] for t in rows], dtype=np.uint32)


def point_call(dev, op, rows):
    inp = pack_points(rows)
    n = len(rows)
    out = np.zeros((n, 36), dtype=np.uint32)
    flag = np.full(n, 0xdeadbeef, dtype=np.uint32)
    rc = dev.gputest_p384_point_op(op, ctypes.c_uint32(n), _ptr(inp), _ptr(out), _ptr(flag))
    assert rc == 0, rc
    return [[int_of_words(r[12 * k:12 * k + 12]) for k in range(3)] for r in out.tolist()], flag.tolist()


def mont_p(t):
    return tuple(c * W % P for c in t)


POINT_CASES = [(op, c) for op in POINT_OPS for c in POINT_CLASSES[op]]


@gpu
@pytest.mark.parametrize("op,cls", POINT_CASES, ids=["%s-%s" % c for c in POINT_CASES])
def test_p384_point_ops_on_device(dev, op, cls):
    """pt_dbl, pt_add<false> and pt_add<true> on chosen representatives: Z3 != 0 and the affine sum of the reference, Z3 == 0 for
    P + (-P) and infinity, the reference's doubling for P + P - also where one lane of a wavefront takes that branch alone - and every
    output coordinate in [0, p)."""
    key = ("point", op)
    if key not in _run_cache:
        flat, spans = flatten(point_vectors(op))
        out, flag = point_call(dev, POINT_OPS[op], [mont_p(a) + mont_p(b) for a, b, _ in flat])
        assert set(flag) == {0}
        _run_cache[key] = (flat, spans, out)
    flat, spans, out = _run_cache[key]
    lo, hi = spans[cls]
    assert hi > lo
    print("vectors %s %s: %d" % (op, cls, hi - lo))
    bad = [(i - lo, e) for i, e in ((i, point_errors(flat[i][2], out[i], True)) for i in range(lo, hi)) if e]
    assert not bad, (len(bad), bad[:3])


@gpu
@pytest.mark.parametrize("cls", ON_CURVE_CLASSES)
def test_p384_on_curve_on_device(dev, cls):
    if "on_curve" not in _run_cache:
        flat, spans = flatten(on_curve_vectors())
        out, flag = point_call(dev, 3, [mont_p((x, y, 1)) + mont_p(R.G + (1,)) for x, y, _ in flat])
        assert all(tuple(o) == mont_p((x, y, 1)) for o, (x, y, _) in zip(out, flat))
        _run_cache["on_curve"] = (flat, spans, flag)
    flat, spans, flag = _run_cache["on_curve"]
    lo, hi = spans[cls]
    assert hi > lo and [flag[i] for i in range(lo, hi)] == [w for _, _, w in flat[lo:hi]]


@gpu
@pytest.mark.parametrize("cls", ["first_branch", "second_branch", "r_edges", "infinity"])
def test_p384_x_equals_r_on_device(dev, cls):
    if "x_equals_r" not in _run_cache:
        flat, spans = flatten(x_equals_r_vectors())
        _, flag = point_call(dev, 4, [mont_p(t) + (r, 0, 0) for t, r, _ in flat])          # r travels as plain words
        _run_cache["x_equals_r"] = (flat, spans, flag)
    flat, spans, flag = _run_cache["x_equals_r"]
    lo, hi = spans[cls]
    bad = [(i - lo, flat[i][1]) for i in range(lo, hi) if flag[i] != flat[i][2]]
    assert hi > lo and not bad, bad[:3]
