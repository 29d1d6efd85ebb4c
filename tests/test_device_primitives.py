"""The DEVICE compilation of the field, scalar, inversion and point code, one primitive at a time, against Python integers.

Wherever the headers branch on __HIP_DEVICE_COMPILE__ the kernels run code no host test executes: the generated asm products of
fe29_gcn.h / bn29_gcn.h, the 36 one-lane programs of one29_gcn.h, the v_mad_u64_u32 mac of fp256.h, and the wave-wide ballots that end
modinv and pair_modinv.  The hooks of gputest.hip ("primitives on many wavefronts") run exactly that code over grids of wavefronts;
this file compares every answer with big-integer arithmetic and the affine group law of oracle/bccsp_sw_oracle.py - never with the
gcn_dsl interpreter and never with the host C bodies.  All comparisons are exact.

Two halves.  The CPU half (not marked gpu) tests the generators and the comparators themselves - a comparator must flag a limb off by
one, a value off by p, and a right value with a digit one step outside its contract - and sends the same 32-byte vectors through the
host hooks of libfabgpu_hosttest.so where an entry point with the same meaning exists.  The GPU half runs one launch per (op, input
form) with all input classes concatenated (at least 2^16 items each) and reports one case per op and input class.

No case is dropped after the device has answered: an input class that needs a precondition (L(a) L(b) within the field's bound,
|a| < 16 p for the zero test, u2 != 0, ...) enforces it in its generator, and the enforcing code and the surviving count are asserted.

Bounds that the headers leave to the reader are derived here, not measured:
  * top limb of a product: the result lies in [T/R, T/R + p) (fe29.h, bn29.h: "some representative in (T/R, T/R + p)"), its low
    eight digits sum to less than 2^231 + 2^203 in magnitude, hence |v[8]| <= ((|T| / R + p) >> 232) + 1;
  * fe_weak_norm: for |limb| < 2^31 - 2^28 the carry (a + 2^28) >> 29 lies in [-3, 3], so digits 1..7 lie in [-2^28 - 3, 2^28 + 2],
    digit 0 in [-2^28, 2^28 - 1], and the value is unchanged as an integer.

Division-step survey (the `slow_search` class, a fixed budget of candidates per modulus: 2 000 seeded random values plus 2^k, 2^-k,
m - 2^k, 2^k +- 1 and -2^-k for every k).  The largest count depends on the seed of the random part; with the seeds the GPU launches
use it is SURVEY_MAX_STEPS below, which test_inversion_generator_arranges_the_wavefronts recomputes and asserts: batch counts 16, 17
and 18 (17 and 18 only for the BN prime).  Nothing above 540 steps turned up under any seed tried - inversion_vectors() asserts it -
so batches 19 and 20 of the loops stay unreached by these tests.
"""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import bccsp_sw_oracle as po
import idemix_oracle as io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-mod_amd", "csrc"))
import gen_pair_gcn as gp  # noqa: E402

R = 1 << 261                      # the Montgomery radix of both 29-bit-limb fields
B28 = 1 << 28
M29 = (1 << 29) - 1
W256 = 1 << 256
NRANDOM = 1 << 16
G = (po.GX, po.GY)


class Field:
    def __init__(self, name, fid, p, max_l, contracts):
        self.name, self.fid, self.p, self.max_l = name, fid, p, max_l
        self.ri = pow(R, -1, p)
        self.contracts = contracts        # {name: (lo, hi, top lo, top hi)} taken from gen_pair_gcn, not retyped


def _contracts(*states):
    c = {"AFFINE": gp.AFFINE}
    for sname, st in states:
        for k, v in st.items():
            c["%s.%s" % (sname, k)] = v
    return c


P256F = Field("p256", 0, po.P, 14, _contracts(("STATE_P256", gp.STATE_P256), ("STATE_ONE", gp.STATE_ONE)))
BNF = Field("bn", 1, io.P, 12, _contracts(("STATE_BN", gp.STATE_BN)))
FIELDS = {"p256": P256F, "bn": BNF}


# ---- digits ---------------------------------------------------------------------------------------------------------------------------
def bal(x):
    """Balanced digits of any integer: digits 0..7 in [-2^28, 2^28), the rest in digit 8."""
    d = []
    for _ in range(8):
        t = x & M29
        if t >> 28:
            t -= 1 << 29
        d.append(t)
        x = (x - t) >> 29
    d.append(x)
    return d


def uns(x):
    """Unsigned digits: digits 0..7 in [0, 2^29), the rest in digit 8."""
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def value(limbs):
    return sum(int(v) << (29 * i) for i, v in enumerate(limbs))


def limb_l(limbs):
    """Limb magnitude in units of 2^28 (fe29.h "L"), over all nine limbs."""
    return max(1, max(-(-abs(int(v)) // B28) for v in limbs))


def special_values(m):
    """The special 256-bit values around modulus m that the issue lists."""
    s = [0, 1, 2, m - 1, m - 2, m, m + 1, W256 - 1, 1 << 255, (1 << 224) + 1, (1 << 224) - 1, (1 << 192) + 1, (1 << 192) - 1,
         (1 << 96) + 1, (1 << 96) - 1, int("1fffffff" * 8, 16), int("10000000" * 8, 16)]
    for k in range(1, 9):
        s += [1 << (29 * k), (1 << (29 * k)) - 1]
    for k in range(1, 8):
        s += [(1 << (32 * k)) + 1, (1 << (32 * k)) - 1]
    out = []
    for v in s:
        if 0 <= v < W256 and v not in out:
            out.append(v)
    return out


# ---- comparators ------------------------------------------------------------------------------------------------------------------------
def product_errors(F, T, limbs, canon=None, zero=None):
    """What is wrong with `limbs` as the Montgomery product of an operand product T (an integer): [] when
    value(limbs) * R == T (mod p) with the representative inside [T/R, T/R + p), digits 0..7 inside [-2^28, 2^28] and the top limb inside
    the derived bound.  canon / zero, when given, must be T / R^2 mod p as an integer of [0, p) and the zero flag of that residue."""
    errs = []
    v = value(limbs)
    if (v * R - T) % F.p:
        errs.append("value")
    elif not (T <= v * R < T + F.p * R):
        errs.append("representative")
    for i in range(8):
        if not -B28 <= int(limbs[i]) <= B28:
            errs.append("digit%d" % i)
    if abs(int(limbs[8])) > (((abs(T) // R) + F.p) >> 232) + 1:
        errs.append("digit8")
    want = T * F.ri * F.ri % F.p
    if canon is not None and canon != want:
        errs.append("canon")
    if zero is not None and bool(zero) != (want == 0):
        errs.append("zero")
    return errs


def contract_errors(limbs, c):
    """Digits of `limbs` outside the contract c = (lo, hi, top lo, top hi)."""
    errs = ["digit%d" % i for i in range(8) if not c[0] <= int(limbs[i]) <= c[1]]
    if not c[2] <= int(limbs[8]) <= c[3]:
        errs.append("digit8")
    return errs


WEAK_NORM_IN = (1 << 31) - (1 << 28) - 1          # fe29.h: "input limbs may be anything below 2^31 - 2^28 in magnitude"


def weak_norm_errors(a, out):
    errs = []
    if value(out) != value(a):
        errs.append("value")
    if not -B28 <= int(out[0]) <= B28 - 1:
        errs.append("digit0")
    errs += ["digit%d" % i for i in range(1, 8) if not -B28 - 3 <= int(out[i]) <= B28 + 2]
    return errs


# ---- vectors of the field ops -----------------------------------------------------------------------------------------------------------
FIELD_OPS = {"mul": 0, "sqr": 1, "addsub_mul": 2, "dbl_mul": 3, "weak_norm": 4, "ident": 5}


def op_product(op, va, vb):
    """The integer the op's product multiplies out to (T); None for the ops that are not products."""
    return {"mul": va * vb, "sqr": va * va, "addsub_mul": (va + vb) * (va - vb), "dbl_mul": 2 * va * vb}.get(op)


def op_operand_ls(op, a, b):
    """(L of the first factor, L of the second) as the op forms them from limbs a, b."""
    if op == "mul":
        return limb_l(a), limb_l(b)
    if op == "sqr":
        return limb_l(a), limb_l(a)
    if op == "addsub_mul":
        return limb_l([x + y for x, y in zip(a, b)]), limb_l([x - y for x, y in zip(a, b)])
    return limb_l([2 * x for x in a]), limb_l(b)


def value_vectors(F, rng):
    """Form 0 (32-byte integers, converted on the device): {class: [(x, y)]}."""
    sp = special_values(F.p)
    return {"special_values": [(x, y) for x in sp for y in sp],
            "random": [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(NRANDOM)]}


def _rand_in(rng, c):
    return [rng.randrange(c[0], c[1] + 1) for _ in range(8)] + [rng.randrange(c[2], c[3] + 1)]


def _norm(rng):
    return [rng.randrange(-B28, B28 + 1) for _ in range(8)] + [rng.randrange(-(1 << 24), (1 << 24) + 1)]


def _lazy(rng, k, extreme):
    """A sum / difference of k normalised elements; extreme: every digit of every term at an end of its range."""
    if extreme:
        return [rng.choice((-1, 1)) * k * B28 for _ in range(8)] + [rng.choice((-1, 1)) * k * (1 << 24)]
    acc = [0] * 9
    for _ in range(k):
        s = rng.choice((-1, 1))
        acc = [x + s * y for x, y in zip(acc, _norm(rng))]
    return acc


def sqrt_mod_2k(c, k):
    """A square root of c = 1 (mod 8) modulo 2^k, by Hensel lifting: x^2 = c (mod 2^i) makes x or x + 2^(i-1) a root modulo 2^(i+1)."""
    assert c % 8 == 1 and k >= 3
    x = 1
    for i in range(3, k):
        if (x * x - c) >> i & 1:
            x += 1 << (i - 1)
    assert (x * x - c) % (1 << k) == 0
    return x


def quotient_of(F, op, a, b):
    """q = -T / p mod 2^261 of the product the op forms from limbs a, b: the nine Montgomery quotient digits, low column first."""
    return op_product(op, value(a), value(b)) * ((-pow(F.p, -1, R)) % R) % R


def quotient_cells(F, op):
    """The (column, digit) cells among {0..8} x {0, 2^29 - 1} that the op's product can have at all.  q = T * (-1/p) mod 2^261:
    any q for mul and for (a + b)(a - b) (factors of equal parity: both odd, or T = 0 mod 4);  q even for (2a) b, so digit 0 is never
    2^29 - 1;  for a square q = a^2 * (-1/p) is 0, 4 or -1/p modulo 8, so digit 0 = 2^29 - 1 (7 mod 8) needs p = 1 (mod 8)."""
    cells = {(k, v) for k in range(9) for v in (0, M29)}
    if op == "dbl_mul" or (op == "sqr" and F.p % 8 != 1):
        cells.discard((0, M29))
    return cells


def quotient_pairs(F, op, rng, per_cell=24):
    """Operands, solved for per op, whose product has Montgomery quotient digit `col` equal to 0 or to 2^29 - 1, for every cell of
    quotient_cells(F, op).  Each pair is checked here against the product the op really forms."""
    ninv = (-pow(F.p, -1, R)) % R
    out = []
    for col, forced in sorted(quotient_cells(F, op)):
        for _ in range(per_cell):
            q = rng.getrandbits(261)
            q = (q & ~(M29 << (29 * col))) | (forced << (29 * col))
            if op == "mul":                       # a odd:  b = q / (a * -1/p)
                a = rng.getrandbits(256) | 1
                b = q * pow(a * ninv, -1, R) % R
            elif op == "dbl_mul":                 # T = 2 a b, q even:  b = (q / 2) / (a * -1/p) mod 2^260
                q &= ~1
                a = rng.getrandbits(256) | 1
                b = (q >> 1) * pow(a * ninv, -1, R >> 1) % (R >> 1)
            elif op == "addsub_mul":              # T = f1 f2 with f1 = a + b, f2 = a - b of equal parity
                if (col, forced) == (0, 0):       # q = 0 (mod 4): both factors even, f1 = 2 g1, f2 = 2 g2, g2 = (q / 4) / (g1 * -1/p) mod 2^259
                    g1 = rng.getrandbits(255) | 1
                    f1, f2 = 2 * g1, 2 * ((q >> 2) * pow(g1 * ninv, -1, R >> 2) % (R >> 2))
                else:                             # q odd: both factors odd
                    q |= 1
                    f1 = rng.getrandbits(256) | 1
                    f2 = q * pow(f1 * ninv, -1, R) % R
                a, b = (f1 + f2) // 2, (f1 - f2) // 2
            elif (col, forced) == (0, 0):         # a^2 = 0 (mod 2^29): a a multiple of 2^15
                a = b = rng.getrandbits(241) << 15
            else:                                 # a^2 = q / (-1/p) (mod 2^261): a root exists when that is 1 (mod 8), i.e. q = -1/p (mod 8)
                q = (q & ~7) | (ninv & 7)
                a = b = sqrt_mod_2k(q * pow(ninv, -1, R) % R, 261)
            la, lb = bal(a), bal(b)
            assert quotient_of(F, op, la, lb) >> (29 * col) & M29 == forced, (op, col, forced)
            out.append((la, lb))
    return out


def euler(F, c):
    return pow(c % F.p, (F.p - 1) // 2, F.p) if c % F.p else 0


def target_reps(F, op):
    """Which of the representatives 0, 1, p - 1 and (before canonicalisation) p the op's exact Montgomery result can be.  All four for
    the products of two free factors.  A square a^2 / R is 0 for a = 0 and p for a = p;  it is p - 1 only if -R is a square modulo p,
    and 1 only if R - j p is a perfect square for some 0 <= j <= 32 (the result is at least a^2 / R, so 1 needs a^2 <= R)."""
    if op != "sqr":
        return {0, 1, F.p - 1, F.p}
    reps = {0, F.p}
    if euler(F, -R) == 1:
        reps.add(F.p - 1)
    if any(_isqrt_exact(R - j * F.p) for j in range(33)):
        reps.add(1)
    return reps


def target_residues(F, op):
    """The residues among 0, 1, -1 that the op's result can be congruent to: for a square, t only where R t is a square modulo p."""
    return {0, 1, F.p - 1} if op != "sqr" else {0} | {t for t in (1, F.p - 1) if euler(F, R * t) == 1}


def _isqrt_exact(x):
    import math
    return x >= 0 and math.isqrt(x) ** 2 == x


def product_value(F, T):
    """The exact representative Montgomery reduction leaves for the operand product T."""
    return (T + (-T * pow(F.p, -1, R)) % R * F.p) // R


def target_pairs(F, op, rng):
    """Operands, solved for per op, whose result lands on 0, 1, p - 1 and, before canonicalisation, on p itself - as the exact
    representative where target_reps() says the op can reach it, and as the residue class (1 or -1 plus a multiple of p) besides.
    A small first factor (T / R < 1) makes the representative the target itself and not the target plus p."""
    p = F.p
    assert p % 4 == 3                                              # square roots below are c^((p + 1) / 4)
    out = []
    if op == "sqr":
        for k in range(-12, 13):                                   # a = k p: T = k^2 p^2, the result a multiple of p (0 for k = 0, p for k = +-1)
            out.append((bal(k * p), bal(k * p)))
        for t in (1, p - 1):
            c = R * t % p
            if euler(F, c) == 1:
                r = pow(c, (p + 1) // 4, p)
                assert r * r % p == c
                for k in range(-12, 13):                           # every representative +-r + k p of the two roots
                    out += [(bal(r + k * p), bal(r + k * p)), (bal(k * p - r), bal(k * p - r))]
        return out
    for f1 in list(range(1, 16)) + [rng.randrange(1, p) for _ in range(64)]:
        for t in (0, 1, p - 1, p):
            div = 2 * f1 if op == "dbl_mul" else f1                # the first factor the op forms
            f2 = p if t == p else R * t * pow(div, -1, p) % p      # T = div * p: q = R - div, the result is p itself
            if op == "addsub_mul":
                if (f1 + f2) & 1:                                  # a + b and a - b have the same parity: the other representative of f2
                    if t == p:
                        continue                                   # ... p itself is left to the odd f1
                    f2 += p
                out.append((bal((f1 + f2) // 2), bal((f1 - f2) // 2)))
            else:
                out.append((bal(f1), bal(f2)))
    return out


def target_hits(F, op, pairs):
    """(exact representatives among 0, 1, p - 1, p; residues among 0, 1, -1) that the results of `pairs` land on."""
    reps, res = set(), set()
    for a, b in pairs:
        v = product_value(F, op_product(op, value(a), value(b)))
        if v in (0, 1, F.p - 1, F.p):
            reps.add(v)
        if v % F.p in (0, 1, F.p - 1):
            res.add(v % F.p)
    return reps, res


def limb_vectors(F, op, rng):
    """Form 1 (raw limbs) for a product op: {class: [(a, b)]}.  Every pair satisfies L(first factor) * L(second factor) <= F.max_l as
    the op forms its factors: pairs that would not are never emitted, and limb_vector_census() asserts what survives."""
    out = {"limb_ends": [], "lazy": [], "quotient": [], "result_targets": [], "random_limbs": []}    # quotient, result_targets: built per op
    norm_c = (-B28, B28, -(1 << 24), 1 << 24)
    cs = list(F.contracts.items()) + [("normalised", norm_c)]
    for na, ca in cs:
        for nb, cb in cs:
            pats = []
            for ea in (0, 1):
                for eb in (0, 1):
                    pats.append(([ca[ea]] * 8 + [ca[2 + ea]], [cb[eb]] * 8 + [cb[2 + eb]]))                          # all-low / all-high
                    pats.append(([ca[(ea + i) & 1] for i in range(8)] + [ca[2 + ea]], [cb[(eb + i) & 1] for i in range(8)] + [cb[2 + eb]]))  # alternating
            for pos in range(9):                                                                                   # one digit at an end, the rest random
                for end in (0, 1):
                    a, b = _rand_in(rng, ca), _rand_in(rng, cb)
                    a[pos] = ca[end] if pos < 8 else ca[2 + end]
                    b[8 - pos] = cb[end] if pos > 0 else cb[2 + end]
                    pats.append((a, b))
            out["limb_ends"] += pats
    # lazy operands: the [L x L] shapes the point formulas use (ec29.h, p256_verify29.h pt_dbl29: [8x1] [6x1] [3x3] [3x2] [2x2];
    # bn_nym29.h: [4x1] [3x3] [3x2]) and the bound itself
    shapes = [(8, 1), (6, 1), (3, 3), (3, 2), (2, 2), (4, 1), (F.max_l, 1), (F.max_l // 2, 2), (F.max_l // 2, 1), (F.max_l // 3, 3)]
    for la, lb in shapes:
        for extreme in (False, True):
            for _ in range(40):
                out["lazy"].append((_lazy(rng, la, extreme), _lazy(rng, lb, extreme)))
                out["lazy"].append((_lazy(rng, lb, extreme), _lazy(rng, la, extreme)))
    out["quotient"] = quotient_pairs(F, op, rng)
    out["result_targets"] = target_pairs(F, op, rng)
    out["random_limbs"] = [(_norm(rng), _norm(rng)) for _ in range(NRANDOM)]
    # the precondition, enforced before anything is launched
    kept = {}
    for cls, vs in out.items():
        if op == "sqr" and cls not in ("quotient", "result_targets"):
            vs = [(a, a) for a, _ in vs] + [(b, b) for _, b in vs if cls != "random_limbs"]
        kept[cls] = [(a, b) for a, b in vs if _fits(F, op, a, b)]
    return kept


def _fits(F, op, a, b):
    """L(first factor) * L(second factor) within the field's bound, and every limb of the operands AND of the sums, differences and
    doublings the op forms from them representable in an int32 (fe_add / fe_sub / fe_dbl do not wrap: FE29_ASSERT_LIMB)."""
    la, lb = op_operand_ls(op, a, b)
    formed = {"addsub_mul": [x + y for x, y in zip(a, b)] + [x - y for x, y in zip(a, b)], "dbl_mul": [2 * x for x in a]}.get(op, [])
    return la * lb <= F.max_l and all(abs(int(x)) < (1 << 31) for x in list(a) + list(b) + formed)


def zero_vectors(F, rng):
    """Form 1, op ident: k p for every k with |k p| < 16 p, canonical and lazy digit forms, and the neighbours k p +- 1.
    {class: [a]}; every a has |value| < 16 p and L(a) <= F.max_l (it is multiplied by 1)."""
    out = {"zero_multiples": [], "zero_neighbours": []}
    for k in range(-15, 16):
        forms = [bal(k * F.p)]
        for k1 in {k // 2, k - 1, 7 if k > 0 else -7}:
            forms.append([x + y for x, y in zip(bal(k1 * F.p), bal((k - k1) * F.p))])                  # lazy: two multiples added limb by limb
        if abs(k) <= F.max_l:
            forms.append([k * x for x in bal(F.p)])                                                   # lazy: k times the digits of p
        if 0 <= k <= 15 and k * F.p < 1 << 261:
            forms.append(uns(k * F.p))
        out["zero_multiples"] += forms
        for f in forms:
            for d in (1, -1):
                g = list(f)
                g[0] += d
                out["zero_neighbours"].append(g)
    for cls in out:
        out[cls] = [a for a in out[cls] if abs(value(a)) < 16 * F.p and limb_l(a) <= F.max_l and all(abs(x) < (1 << 31) for x in a)]    # ... and int32 limbs
    return out


def weak_norm_vectors(rng):
    w = WEAK_NORM_IN
    out = {"limb_ends": [[-w] * 9, [w] * 9, [(-w, w)[i & 1] for i in range(9)], [(w, -w)[i & 1] for i in range(9)]], "random_limbs": []}
    for pos in range(9):
        for end in (-w, w, -B28, B28, B28 - 1, -B28 - 1):
            a = [rng.randrange(-w, w + 1) for _ in range(9)]
            a[pos] = end
            out["limb_ends"].append(a)
    out["random_limbs"] = [[rng.randrange(-w, w + 1) for _ in range(9)] for _ in range(NRANDOM)]
    out["random_limbs"] += [_norm(rng) for _ in range(4096)]          # values below 16 p: the canonical output is checked on these
    return out


# ---- inversion ----------------------------------------------------------------------------------------------------------------------------
MODULI = {"n": (0, po.N), "p": (1, po.P), "bnp": (2, io.P)}
# {(modulus, pair): most division steps the survey of that launch reached}; recomputed and asserted by the CPU half
SURVEY_MAX_STEPS = {("n", 0): 530, ("n", 1): 529, ("p", 0): 530, ("p", 1): 531, ("bnp", 0): 530, ("bnp", 1): 530}


def divstep_count(m, x):
    """Division steps (delta = 1/2 start, modinv30.h) until g = 0."""
    f, g, zeta, n = m, x, -1, 0
    while g:
        if g & 1:
            if zeta < 0:
                f, g, zeta = g, (g - f) >> 1, -zeta - 2
            else:
                g, zeta = (g + f) >> 1, zeta - 1
        else:
            g >>= 1
            zeta -= 1
        n += 1
    return n


def batches(m, x):
    return -(-divstep_count(m, x) // 30)


cls_max_steps = {}          # (modulus, lanes per wavefront) -> most division steps among the surveyed inputs of the last call


def inversion_vectors(m, rng, lanes_per_wave):
    """(inputs, classes {name: [index]}, batch count of every input whose count was computed {index: batches}).  The first part of the
    launch is laid out wavefront by wavefront (lanes_per_wave items each) so that the exit ballot decides: wavefronts whose inputs all finish
    in the fewest batches, one slow input among fast ones, x = 0 beside live inputs, all three batch counts mixed - and the launch
    ends in a partial wavefront."""
    structured = [1, 2, m - 1, m - 2, (m + 1) // 2, (m - 1) // 2]
    for k in range(256):
        v = 1 << k
        if v < m:
            structured += [v, pow(v, -1, m)]
    search = []
    for k in range(1, 256):
        search += [v for v in ((m - (1 << k)) % m, ((1 << k) + 1) % m, ((1 << k) - 1) % m, m - pow(1 << k, -1, m)) if v]
    search += [rng.randrange(1, m) for _ in range(2000)]
    count, steps = {}, {}
    for v in structured + search:
        if v not in count:
            steps[v] = divstep_count(m, v)
            count[v] = -(-steps[v] // 30)
    assert max(count.values()) <= 18, max(steps.values())       # the module docstring says batches 19 and 20 stay unreached: keep it true
    fewest = min(count.values())
    by = {}
    for v, c in count.items():
        by.setdefault(c, []).append(v)
    fast = by[fewest] if len(by[fewest]) >= lanes_per_wave else [v for v in count if count[v] <= 17]
    slow = by[max(by)]
    xs, cls, known = [], {}, {}

    def wave(name, items):
        assert len(items) == lanes_per_wave and len(xs) % lanes_per_wave == 0
        cls.setdefault(name, []).extend(range(len(xs), len(xs) + len(items)))
        for v in items:
            if v:
                known[len(xs)] = count[v]
            xs.append(v)
    for w in range(4):
        wave("wave_all_fast", [fast[(w * lanes_per_wave + i) % len(fast)] for i in range(lanes_per_wave)])
    for w in range(4):
        items = [fast[(w + 3 * i) % len(fast)] for i in range(lanes_per_wave)]
        items[(17 * w + 5) % lanes_per_wave] = slow[w % len(slow)]
        wave("wave_one_slow", items)
    for w in range(4):
        items = [slow[(w + i) % len(slow)] if i % (w + 2) else 0 for i in range(lanes_per_wave)]
        wave("wave_zero_beside_live", items)
    counts = sorted(by)
    for w in range(4):
        wave("wave_mixed_counts", [by[counts[i % len(counts)]][(w + i) % len(by[counts[i % len(counts)]])] for i in range(lanes_per_wave)])
    for name, vs in (("structured", structured), ("slow_search", sorted(count, key=lambda v: -count[v])[:256])):
        cls[name] = list(range(len(xs), len(xs) + len(vs)))
        for v in vs:
            known[len(xs)] = count[v]
            xs.append(v)
    nr = NRANDOM + (-(len(xs) + NRANDOM) % lanes_per_wave) + lanes_per_wave // 2 + 3        # ... so that the last wavefront is partial
    cls["random_partial_last_wave"] = list(range(len(xs), len(xs) + nr))
    xs += [rng.randrange(1, m) for _ in range(nr)]
    cls_max_steps[(m, lanes_per_wave)] = max(steps.values())
    return xs, cls, known


def inversion_census(xs, known, lanes_per_wave):
    """(most distinct batch counts inside one wavefront, whether the last wavefront is partial)"""
    per = {}
    for i, c in known.items():
        per.setdefault(i // lanes_per_wave, set()).add(c)
    return max(len(s) for s in per.values()), len(xs) % lanes_per_wave != 0


# ---- points -------------------------------------------------------------------------------------------------------------------------------
P = po.P
RI = P256F.ri


def mont_rep(v, k=0, unsigned=False):
    """Limbs of the Montgomery form of v mod p, representative v R mod p + k p, balanced or unsigned digits."""
    x = v * R % P + k * P
    return uns(x) if unsigned else bal(x)


def fe_val(limbs):
    return value(limbs) * RI % P


def jac_random(pt, rng):
    z = rng.randrange(1, P)
    return (pt[0] * z * z % P, pt[1] * z * z * z % P, z)


def point_pool(rng, n):
    pts = [po.pt_mul(rng.randrange(1, po.N), G)]
    step = po.pt_mul(rng.randrange(1, po.N), G)
    while len(pts) < n:
        pts.append(po.pt_add(pts[-1], step))
    return pts


def state_limbs(J, rng, lazy=False):
    """X Y Z limbs inside gen_pair_gcn.STATE_ONE; lazy: non-canonical representatives (shifted by multiples of p, unsigned digits)."""
    if not lazy:
        return mont_rep(J[0]) + mont_rep(J[1]) + mont_rep(J[2])
    return mont_rep(J[0], rng.choice((-4, -1, 1, 2))) + mont_rep(J[1], rng.choice((-3, -1, 1)), rng.random() < 0.5) + mont_rep(J[2], rng.choice((0, 1)), True)


def in_state_one(l27):
    S = gp.STATE_ONE
    return not (contract_errors(l27[0:9], S["X"]) or contract_errors(l27[9:18], S["Y"]) or contract_errors(l27[18:27], S["Z"]))


def small_coordinate_points(rng):
    """Jacobian points for the doubling with a small affine x, a small Jacobian X (Z chosen so that x Z^2 is small) and a small
    Jacobian Y (Z a cube root of small / y: p = 4 mod 9, so cube roots of cubic residues are c^(3^-1 mod (p-1)/3))."""
    out = []
    x = 0
    while len(out) < 12:
        x += 1
        rhs = (x * x * x - 3 * x + po.B) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            out += [(x, y, 1), jac_random((x, y), rng), jac_random((x, P - y), rng)]
    pts = point_pool(rng, 24)
    e3 = pow(3, -1, (P - 1) // 3)
    for pt in pts:
        for small in range(1, 200):
            c = small * pow(pt[0], -1, P) % P
            z = pow(c, (P + 1) // 4, P)
            if z * z % P == c:
                out.append((small, pt[1] * z * z * z % P, z))
                break
        for small in range(1, 200):
            c = small * pow(pt[1], -1, P) % P
            z = pow(c, e3, P)
            if z * z * z % P == c:
                out.append((pt[0] * z * z % P, small, z))
                break
    assert len(out) >= 12 + 40 and all(po.on_curve(*affine(*J)) for J in out)
    return out


def affine(X, Y, Z):
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def comb_corner_entries():
    """Affine comb-table entries d * 2^(16 w) * G at window corners (ec29.h CombTab<16>)."""
    return [po.pt_mul(d << (16 * w), G) for w in (0, 1, 7, 15) for d in (1, 2, 255, 256, 32768, 65535)]


def point_vectors(op, rng, nrandom=NRANDOM):
    """{class: [(54 input limbs, ("point", affine or None) | ("exceptional", rr_is_zero))]}; inputs lie inside STATE_ONE (the affine addend of madd
    inside AFFINE): asserted by point_vector_census()."""
    pool = point_pool(rng, 2048)
    out = {}
    zero9 = [0] * 9

    def add_case(J1, J2, lazy=False):
        a1, a2 = affine(*J1), affine(*J2)
        l1, l2 = state_limbs(J1, rng, lazy), state_limbs(J2, rng, lazy)
        if a1[0] == a2[0]:
            return (l1 + l2, ("exceptional", a1[1] == a2[1]))
        return (l1 + l2, ("point", po.pt_add(a1, a2)))

    def madd_case(J1, a2, lazy=False):
        a1 = affine(*J1)
        l = state_limbs(J1, rng, lazy) + mont_rep(a2[0]) + mont_rep(a2[1]) + zero9
        if a1[0] == a2[0]:
            return (l, ("exceptional", a1[1] == a2[1]))
        return (l, ("point", po.pt_add(a1, a2)))

    def dbl_case(J1, lazy=False):
        return (state_limbs(J1, rng, lazy) + zero9 * 3, ("point", po.pt_add(affine(*J1), affine(*J1))))
    pick = lambda: pool[rng.randrange(len(pool))]
    neg = lambda pt: (pt[0], P - pt[1])
    if op == "dbl":
        out["random_z"] = [dbl_case(jac_random(pick(), rng)) for _ in range(nrandom)]
        out["lazy_representatives"] = [dbl_case(jac_random(pick(), rng), True) for _ in range(512)]
        out["small_coordinates"] = [dbl_case(J, lz) for J in small_coordinate_points(rng) for lz in (False, True)]
    elif op == "add":
        out["random_z"] = [add_case(jac_random(pick(), rng), jac_random(pick(), rng)) for _ in range(nrandom)]
        out["lazy_representatives"] = [add_case(jac_random(pick(), rng), jac_random(pick(), rng), True) for _ in range(512)]
        out["p_plus_p"] = [add_case(jac_random(pt, rng), jac_random(pt, rng), lz) for pt in pool[:128] for lz in (False, True)]
        out["p_plus_minus_p"] = [add_case(jac_random(pt, rng), jac_random(neg(pt), rng), lz) for pt in pool[:128] for lz in (False, True)]
    else:
        corners = comb_corner_entries()
        out["random_z"] = [madd_case(jac_random(pick(), rng), pick()) for _ in range(nrandom)]
        out["lazy_representatives"] = [madd_case(jac_random(pick(), rng), pick(), True) for _ in range(512)]
        out["comb_corners"] = [madd_case(jac_random(pick(), rng), c, lz) for c in corners for lz in (False, True) for _ in range(4)]
        out["p_plus_p"] = [madd_case(jac_random(pt, rng), pt, lz) for pt in pool[:128] + corners for lz in (False, True)]
        out["p_plus_minus_p"] = [madd_case(jac_random(pt, rng), neg(pt), lz) for pt in pool[:128] + corners for lz in (False, True)]
    return out


def point_vector_census(op, vecs):
    n = 0
    for vs in vecs.values():
        for l, _ in vs:
            assert in_state_one(l[0:27])
            if op == "add":
                assert in_state_one(l[27:54])
            elif op == "madd":
                assert not contract_errors(l[27:36], gp.AFFINE) and not contract_errors(l[36:45], gp.AFFINE)
            n += 1
    return n


def point_errors(op, l, want, out45):
    """Compare one answer of gputest_point_op: X Y Z inside STATE_ONE, (X / Z^2, Y / Z^3) the affine result, h and rr what the formulas define."""
    errs = []
    X1, Y1, Z1, X2, Y2, Z2 = (fe_val(l[9 * i:9 * i + 9]) for i in range(6))
    X3, Y3, Z3, H, RR = (fe_val(out45[9 * i:9 * i + 9]) for i in range(5))
    S = gp.STATE_ONE
    for nm, i in (("X", 0), ("Y", 1), ("Z", 2)):
        errs += ["%s.%s" % (nm, e) for e in contract_errors(out45[9 * i:9 * i + 9], S[nm])]
    if op == "add":
        h = (X2 * Z1 * Z1 - X1 * Z2 * Z2) % P
        rr = (Y2 * Z1 * Z1 * Z1 - Y1 * Z2 * Z2 * Z2) % P
    elif op == "madd":
        h = (X2 * Z1 * Z1 - X1) % P
        rr = (Y2 * Z1 * Z1 * Z1 - Y1) % P
    if op != "dbl":
        if H != h:
            errs.append("h")
        if RR != rr:
            errs.append("rr")
    kind, w = want
    if kind == "exceptional":
        if H != 0 or (RR == 0) != w or Z3 != 0:
            errs.append("exceptional")
    else:
        if Z3 == 0 or X3 != w[0] * Z3 * Z3 % P or Y3 != w[1] * Z3 * Z3 * Z3 % P:
            errs.append("point")
    return errs


# ---- scalars ------------------------------------------------------------------------------------------------------------------------------
N = po.N


from scalar_sets import adversarial_u1s, adversarial_u2s, edge_u2_targets  # noqa: E402  (shared with test_host_logic / test_pair_helper_waves)


def loop_vectors(rng, dq):
    """{class: [(u1, u2)]} for R = u1 G + u2 Q, Q = dq G; u1, u2 < n and u2 != 0 (enforced here, asserted by the callers)."""
    u1s, u2s = adversarial_u1s(rng), adversarial_u2s(rng)
    out = {"adversarial_u2": [(u1s[k % len(u1s)], u2) for k, u2 in enumerate(u2s)],
           "adversarial_u1": [(u1, 12345) for u1 in u1s],
           "recoding_edges": [(u1s[k % len(u1s)], u2) for k, u2 in enumerate(edge_u2_targets())],
           "final_add_doubling": [(u2 * dq % N, u2) for u2 in (1, 7, rng.randrange(1, N))],
           "final_add_infinity": [((-u2 * dq) % N, u2) for u2 in (1, 7, rng.randrange(1, N))]}
    return {c: [(a, b) for a, b in vs if a < N and 0 < b < N] for c, vs in out.items()}


def range_status(r, s):
    st = po.ST_VALID
    if r >= N:
        st = po.ST_RANGE
    if s > po.HALF_N:
        st = po.ST_HIGH_S
    if r == 0 or s == 0:
        st = po.ST_RANGE
    return st


def scalar_vectors(op, rng):
    """{class: [(a, b, c)]} of 256-bit integers for gputest_scalar_op `op`."""
    sp = special_values(N)
    rnd = lambda: rng.getrandbits(256)
    if op in ("fn_to_mont", "sub256", "lt256", "sel256"):
        return {"special_values": [(x, y, (i ^ j) & 1) for i, x in enumerate(sp) for j, y in enumerate(sp)],
                "random": [(rnd(), rnd(), rnd()) for _ in range(NRANDOM)]}
    if op == "fn_mul":          # redc_n wants a b < n 2^256: the second factor is reduced
        return {"special_values": [(x, y % N, 0) for x in sp for y in sp], "random": [(rnd(), rnd() % N, 0) for _ in range(NRANDOM)]}
    if op == "range_status":
        edge = [0, 1, N - 1, N, N + 1, po.HALF_N, po.HALF_N + 1, po.HALF_N - 1, W256 - 1, po.P]
        return {"special_values": [(x, y, 0) for x in sp + edge for y in sp + edge], "random": [(rnd(), rnd() >> rng.randrange(0, 3), 0) for _ in range(NRANDOM)]}
    # ecdsa scalars (e, r, s): any 256-bit e and r, 0 <= s < n (s >= n reaches the inversion only on lanes the low-S gate rejected)
    inv = [0, 1, 2, N - 1, N - 2, (N + 1) // 2, (N - 1) // 2] + [1 << k for k in range(0, 256, 9)] + [pow(1 << k, -1, N) for k in range(1, 256, 9)]
    es = [0, 1, N - 1, N, N + 1, W256 - 1, 1 << 255, po.P]
    return {"special_values": [(e, r, s) for e in es for r in sp[:12] + [N - 1, N] for s in inv if s < N],
            "random": [(rnd(), rnd(), rnd() % N) for _ in range(NRANDOM)]}


SCALAR_OPS = {"fn_to_mont": 0, "fn_mul": 1, "sub256": 2, "sel256": 3, "lt256": 4, "range_status": 5, "ecdsa_scalars29": 6, "pair_ecdsa_scalars29": 7}
RN = W256                  # the Montgomery radix of the scalar field


def scalar_want(op, a, b, c):
    """(out0, out1, flag); None where the op leaves the slot unspecified."""
    if op == "fn_to_mont":
        return (a * RN % N, None, None)
    if op == "fn_mul":
        return (a * b * pow(RN, -1, N) % N, None, None)
    if op == "sub256":
        return ((a - b) % W256, None, 1 if a < b else 0)
    if op == "sel256":
        return (a if c & 1 else b, None, None)
    if op == "lt256":
        return (None, None, 1 if a < b else 0)
    if op == "range_status":
        return (None, None, range_status(a, b))
    w = pow(c, -1, N) if c else 0
    return ((a % N) * w % N, (b % N) * w % N, None)


# ---- the library --------------------------------------------------------------------------------------------------------------------------
def be(x):
    return int(x).to_bytes(32, "big")


def be_array(xs):
    return np.frombuffer(b"".join(be(x) for x in xs), dtype=np.uint8).reshape(-1, 32).copy()


def ints_of(arr):
    raw = arr.tobytes()
    return [int.from_bytes(raw[i:i + 32], "big") for i in range(0, len(raw), 32)]


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def hosttest():
    p = os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_hosttest.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(p)


@pytest.fixture(scope="module")
def dev():
    return ctypes.CDLL(os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_gputest.so"))


def flatten(vecs):
    """({class: [vector]}) -> ([vector], {class: (first, last + 1)})"""
    flat, spans = [], {}
    for cls, vs in vecs.items():
        spans[cls] = (len(flat), len(flat) + len(vs))
        flat += vs
    return flat, spans


def dev_field(dev, F, op, form, avals, bvals):
    n = len(avals)
    if form == 0:
        a, b = be_array(avals), be_array(bvals)
    else:
        a, b = np.array(avals, dtype=np.int32), np.array(bvals, dtype=np.int32)
    limbs = np.zeros((n, 9), dtype=np.int32)
    canon = np.zeros((n, 32), dtype=np.uint8)
    zero = np.zeros(n, dtype=np.uint32)
    rc = dev.gputest_field_op(F.fid, FIELD_OPS[op], form, ctypes.c_uint32(n), _ptr(a), _ptr(b), _ptr(limbs), _ptr(canon), _ptr(zero))
    assert rc == 0, rc
    return limbs.tolist(), ints_of(canon), zero.tolist()


# =========================================================================================================================================
# CPU half
# =========================================================================================================================================
def test_digit_helpers_and_special_values():
    rng = random.Random(1)
    for _ in range(2000):
        x = rng.randrange(-(1 << 262), 1 << 262)
        d = bal(x)
        assert value(d) == x and all(-B28 <= v < B28 for v in d[:8])
        if x >= 0:
            assert value(uns(x)) == x and all(0 <= v <= M29 for v in uns(x)[:8])
    for m in (po.P, po.N, io.P):
        sp = special_values(m)
        assert len(sp) >= 40 and len(set(sp)) == len(sp) and all(0 <= v < W256 for v in sp)
        for v in (0, m, m + 1, m - 2, W256 - 1, 1 << 232, (1 << 29) - 1, (1 << 224) - 1, int("1fffffff" * 8, 16)):
            assert v in sp
    assert limb_l([B28] * 9) == 1 and limb_l([B28 + 1] + [0] * 8) == 2 and limb_l([0] * 8 + [-3 * B28]) == 3


@pytest.mark.parametrize("fname", ["p256", "bn"])
def test_product_comparator_flags_what_it_must(fname):
    F = FIELDS[fname]
    rng = random.Random(2)
    for _ in range(200):
        a, b = _norm(rng), _norm(rng)
        T = value(a) * value(b)
        q = (-T * pow(F.p, -1, R)) % R
        good = bal((T + q * F.p) // R)
        canon = T * F.ri * F.ri % F.p
        assert product_errors(F, T, good, canon, canon == 0) == []
        i = rng.randrange(9)
        bad = list(good)
        bad[i] += rng.choice((-1, 1))
        assert "value" in product_errors(F, T, bad, canon, canon == 0)                    # a limb off by one
        for sign in (-1, 1):                                                               # the value off by p
            errs = product_errors(F, T, bal(value(good) + sign * F.p), canon, canon == 0)
            assert "representative" in errs and "value" not in errs
        assert "canon" in product_errors(F, T, good, canon + F.p if canon + F.p < W256 else canon - 1, canon == 0)
        assert "zero" in product_errors(F, T, good, canon, canon != 0)
    # right in value, one digit one step outside its contract: the representative chosen with digit i at 2^28 + 1
    for i in range(8):
        limbs = _norm(rng)
        limbs[i] = B28 + 1
        T = value(limbs) * R - rng.randrange(0, R) * F.p
        assert product_errors(F, T, limbs) == ["digit%d" % i]
        limbs[i] = B28
        T = value(limbs) * R - rng.randrange(0, R) * F.p
        assert product_errors(F, T, limbs) == []
        limbs[i] = -B28 - 1
        T = value(limbs) * R - rng.randrange(0, R) * F.p
        assert product_errors(F, T, limbs) == ["digit%d" % i]
    limbs = _norm(rng)
    T = value(limbs) * R - 5 * F.p
    top = list(limbs)
    top[8] += 2 + ((abs(T) // R + F.p) >> 232) * 2
    top[7] -= (top[8] - limbs[8]) << 29                                                     # same value, digit 8 (and 7) outside
    assert value(top) == value(limbs) and "digit8" in product_errors(F, T, top)
    # the contract comparator of the point outputs and the weak-norm comparator
    c = gp.STATE_ONE["X"]
    ok = [c[1]] * 8 + [c[3]]
    assert contract_errors(ok, c) == [] and contract_errors([c[1] + 1] + ok[1:], c) == ["digit0"] and contract_errors(ok[:8] + [c[2] - 1], c) == ["digit8"]
    a = [rng.randrange(-WEAK_NORM_IN, WEAK_NORM_IN + 1) for _ in range(9)]
    good = bal(value(a))
    assert weak_norm_errors(a, good) == []
    assert weak_norm_errors(a, [good[0] + 1] + good[1:]) != [] and "digit3" in weak_norm_errors(a, good[:3] + [good[3] + (1 << 29), good[4] - 1] + good[5:])


@pytest.mark.parametrize("fname", ["p256", "bn"])
def test_field_generators_enforce_their_preconditions(fname):
    F = FIELDS[fname]
    for op in ("mul", "sqr", "addsub_mul", "dbl_mul"):
        vecs = limb_vectors(F, op, random.Random(3))
        for cls, vs in vecs.items():
            assert len(vs) >= (NRANDOM if cls == "random_limbs" else 24), (op, cls, len(vs))
            for a, b in vs:
                la, lb = op_operand_ls(op, a, b)
                assert la * lb <= F.max_l
        # the bound is reached, not just respected: some pair sits exactly on it
        reach = max(op_operand_ls(op, a, b)[0] * op_operand_ls(op, a, b)[1] for a, b in vecs["lazy"])
        assert reach == {"mul": F.max_l, "dbl_mul": F.max_l, "sqr": 9}.get(op, reach) and reach >= 8, (op, reach)      # 9: the largest square inside either bound
        assert any(max(abs(x) for x in a[:8]) >= B28 for a, _ in vecs["limb_ends"])
    zv = zero_vectors(F, random.Random(4))
    assert len(zv["zero_multiples"]) >= 31 * 4 and len(zv["zero_neighbours"]) >= 31 * 8
    assert {value(a) // F.p for a in zv["zero_multiples"]} == set(range(-15, 16))
    assert all(value(a) % F.p == 0 and abs(value(a)) < 16 * F.p for a in zv["zero_multiples"])
    assert all(value(a) % F.p in (1, F.p - 1) and abs(value(a)) < 16 * F.p for a in zv["zero_neighbours"])
    assert any(limb_l(a) >= 2 for a in zv["zero_multiples"]) and any(limb_l(a) == 1 for a in zv["zero_multiples"])      # lazy and canonical digit forms
    # the quotient and result-target classes do what they say FOR EVERY PRODUCT OP: on the product the op forms, every cell the op can
    # have is forced, and the results land on every target the op can reach
    for op in ("mul", "sqr", "addsub_mul", "dbl_mul"):
        vecs = limb_vectors(F, op, random.Random(5))
        seen = set()
        for a, b in vecs["quotient"]:
            q = quotient_of(F, op, a, b)
            seen |= {(k, (q >> (29 * k)) & M29) for k in range(9) if (q >> (29 * k)) & M29 in (0, M29)}
        assert seen == quotient_cells(F, op) and len(seen) >= 17, (op, sorted(seen))
        assert len(vecs["quotient"]) == 24 * len(seen)                                   # the precondition dropped none of them
        reps, res = target_hits(F, op, vecs["result_targets"])
        assert reps == target_reps(F, op) and res == target_residues(F, op), (op, reps, res)
        assert {0, F.p} <= reps and len(res) >= 2
    assert quotient_cells(F, "mul") == quotient_cells(F, "addsub_mul") == {(k, v) for k in range(9) for v in (0, M29)}
    assert target_reps(F, "mul") == target_reps(F, "addsub_mul") == target_reps(F, "dbl_mul") == {0, 1, F.p - 1, F.p}


def test_sqrt_mod_2k():
    rng = random.Random(8)
    for _ in range(50):
        c = rng.getrandbits(261) & ~7 | 1
        x = sqrt_mod_2k(c, 261)
        assert x * x % R == c and 0 < x < R


def test_inversion_generator_arranges_the_wavefronts():
    for mname, (_, m) in MODULI.items():
        for lanes in (64, 32):
            xs, cls, known = inversion_vectors(m, random.Random(6), lanes)
            distinct, partial = inversion_census(xs, known, lanes)
            assert distinct >= (3 if mname != "bnp" else 2) and partial and len(xs) >= NRANDOM, (mname, distinct)
            assert all(0 <= x < m for x in xs)
            for name in ("wave_all_fast", "wave_one_slow", "wave_zero_beside_live", "wave_mixed_counts", "structured", "slow_search"):
                assert len(cls[name]) >= 4 * lanes or name in ("structured", "slow_search")
            fewest = min(known.values())
            assert all(known[i] <= max(fewest, 17) for i in cls["wave_all_fast"])
            for w in range(4):
                ws = cls["wave_one_slow"][w * lanes:(w + 1) * lanes]
                assert sorted(known[i] for i in ws)[-2:][0] <= 17 < max(known[i] for i in ws)
            assert any(xs[i] == 0 for i in cls["wave_zero_beside_live"]) and any(xs[i] != 0 for i in cls["wave_zero_beside_live"])
    assert divstep_count(po.N, 1) > 0 and batches(po.N, 0) == 0
    # the survey maxima the module docstring points to, with the seeds of the GPU launches
    got = {}
    for mname, (_, m) in MODULI.items():
        for pair in (0, 1):
            lanes = 32 if pair else 64
            inversion_vectors(m, random.Random("modinv/%s/%d" % (mname, pair)), lanes)
            got[(mname, pair)] = cls_max_steps[(m, lanes)]
    print("survey maxima", got)
    assert got == SURVEY_MAX_STEPS


def test_point_generators_and_comparator():
    rng = random.Random(7)
    for op in ("dbl", "add", "madd"):
        vecs = point_vectors(op, rng, nrandom=64)
        assert point_vector_census(op, vecs) == sum(len(v) for v in vecs.values())
        for cls, vs in vecs.items():
            kinds = {w[0] for _, w in vs}
            assert kinds == ({"exceptional"} if cls.startswith("p_plus") else {"point"}), (op, cls)
        assert any(l[18:27] != mont_rep(fe_val(l[18:27])) for l, _ in vecs["lazy_representatives"])
    # the comparator on answers computed here: right, off by one in a limb, and a digit outside STATE_ONE
    vecs = point_vectors("add", rng, nrandom=8)
    for cls, vs in vecs.items():
        for l, want in vs[:8]:
            X1, Y1, Z1, X2, Y2, Z2 = (fe_val(l[9 * i:9 * i + 9]) for i in range(6))
            h, rr = (X2 * Z1 * Z1 - X1 * Z2 * Z2) % P, (Y2 * Z1 ** 3 - Y1 * Z2 ** 3) % P
            if want[0] == "point":
                J = jac_random(want[1], rng)
            else:
                J = (5, 7, 0)
            good = mont_rep(J[0]) + mont_rep(J[1]) + mont_rep(J[2]) + mont_rep(h) + mont_rep(rr)
            assert point_errors("add", l, want, good) == []
            for i in (0, 9, 18, 27, 36) if want[0] == "point" else (18, 27, 36):      # X3, Y3 carry no meaning when P == +-Q
                bad = list(good)
                bad[i] += 1
                assert point_errors("add", l, want, bad) != []
            out = list(good)
            out[2] += 1 << 30
            out[3] -= 2
            errs = point_errors("add", l, want, out)
            assert "X.digit2" in errs and "point" not in errs and "exceptional" not in errs


def _host_fe29(hosttest, fn, o, a, b=0):
    out = ctypes.create_string_buffer(32)
    fn(o, be(a), be(b), out)
    return int.from_bytes(out.raw, "big")


@pytest.mark.parametrize("fname", ["p256", "bn"])
def test_host_bodies_on_the_same_value_vectors(hosttest, fname):
    """The 32-byte vectors of the GPU half through the host hooks (the C bodies): mul, sqr, (a + b)(a - b), the zero test of a - b and
    the round trip."""
    F = FIELDS[fname]
    vecs = value_vectors(F, random.Random(F.fid + 10))
    p = F.p
    if fname == "p256":
        fn, ops = hosttest.hosttest_fe29_op, {"mul": 0, "sqr": 1, "addsub": 4, "zero": 5, "ident": 6}
    else:
        fn, ops = hosttest.hosttest_bn29_op, {"mul": 0, "sqr": 1, "addsub": 2, "zero": 3, "ident": 4}
    n = 0
    for cls, vs in vecs.items():
        for x, y in (vs if cls == "special_values" else vs[:8192]):
            assert _host_fe29(hosttest, fn, ops["mul"], x, y) == x * y % p, (cls, hex(x), hex(y))
            assert _host_fe29(hosttest, fn, ops["sqr"], x) == x * x % p
            assert _host_fe29(hosttest, fn, ops["addsub"], x, y) == (x + y) * (x - y) % p
            assert _host_fe29(hosttest, fn, ops["zero"], x, y) == (1 if (x - y) % p == 0 else 0)
            assert _host_fe29(hosttest, fn, ops["ident"], x) == x % p
            n += 1
    assert n >= 8192 + 40 * 40


def test_host_scalar_field_and_inversion_on_the_same_vectors(hosttest):
    rng = random.Random(20)
    for op, hop in (("fn_to_mont", 8), ("fn_mul", 6)):
        vecs = scalar_vectors(op, rng)
        for cls, vs in vecs.items():
            for a, b, c in (vs if cls == "special_values" else vs[:4096]):
                if op == "fn_to_mont" or a * b < N * W256:
                    assert _host_fe29(hosttest, hosttest.hosttest_fieldop, hop, a, b) == scalar_want(op, a, b, c)[0], (op, hex(a), hex(b))
    for mname, (which, m) in MODULI.items():
        xs, cls, _ = inversion_vectors(m, random.Random(21), 64)
        for i in [j for name in cls for j in cls[name]][:6000]:
            out = ctypes.create_string_buffer(32)
            if which == 2:
                hosttest.hosttest_bn_modinv(be(xs[i]), out)
            else:
                hosttest.hosttest_modinv(which, be(xs[i]), out)
            assert int.from_bytes(out.raw, "big") == (pow(xs[i], -1, m) if xs[i] else 0), (mname, hex(xs[i]))


def test_host_scalar_loop_on_the_same_vectors(hosttest):
    rng = random.Random(22)
    dq = rng.randrange(1, N)
    Q = po.pt_mul(dq, G)
    vecs = loop_vectors(rng, dq)
    assert sum(len(v) for v in vecs.values()) >= 240 and all(0 < u2 < N and u1 < N for vs in vecs.values() for u1, u2 in vs)
    for cls, vs in vecs.items():
        for u1, u2 in vs[::3]:
            x = ctypes.create_string_buffer(32)
            y = ctypes.create_string_buffer(32)
            inf = hosttest.hosttest_combined_mult29(be(u1), be(u2), be(Q[0]), be(Q[1]), x, y)
            got = None if inf else (int.from_bytes(x.raw, "big"), int.from_bytes(y.raw, "big"))
            assert got == loop_want(u1, u2, Q), (cls, hex(u1), hex(u2))


def loop_want(u1, u2, Q):
    return po.pt_add(po.pt_mul(u1, G) if u1 else None, po.pt_mul(u2, Q) if u2 else None)


def test_the_gpu_test_library_exports_the_primitive_hooks_and_the_product_does_not():
    import subprocess

    import fabgpu
    fabgpu.load()
    hooks = {"gputest_field_op", "gputest_scalar_op", "gputest_modinv", "gputest_point_op", "gputest_combined", "gputest_pair_combined",
             "gputest_pair_verify", "gputest_bn_glv_decompose"}
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_gputest.so")], capture_output=True,
                        text=True, check=True).stdout
    assert hooks <= {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    nm = subprocess.run(["nm", "-D", "--defined-only", fabgpu.lib_path()], capture_output=True, text=True, check=True).stdout
    assert not [ln for ln in nm.splitlines() if "gputest" in ln]


# =========================================================================================================================================
# GPU half
# =========================================================================================================================================
_cache = {}


def field_run(dev, fname, op, form):
    """One launch per (field, op, form) with every class concatenated; cached for the cases that read it."""
    key = (fname, op, form)
    if key in _cache:
        return _cache[key]
    F = FIELDS[fname]
    rng = random.Random("%s/%s/%d" % key)
    if form == 0:
        vecs = value_vectors(F, rng)
    elif op == "weak_norm":
        vecs = {c: [(a, a) for a in vs] for c, vs in weak_norm_vectors(rng).items()}
    elif op == "ident":
        vecs = {c: [(a, a) for a in vs] for c, vs in zero_vectors(F, rng).items()}
        vecs["random_limbs"] = [(a, a) for a in (_norm(rng) for _ in range(NRANDOM))]
    else:
        vecs = limb_vectors(F, op, rng)
    flat, spans = flatten(vecs)
    assert len(flat) >= NRANDOM
    limbs, canon, zero = dev_field(dev, F, op, form, [a for a, _ in flat], [b for _, b in flat])
    _cache[key] = (flat, spans, limbs, canon, zero)
    return _cache[key]


def field_case_errors(F, op, form, a, b, limbs, canon, zero):
    if form == 0:
        x, y = a, b
        want = {"mul": x * y, "sqr": x * x, "addsub_mul": (x + y) * (x - y), "dbl_mul": 2 * x * y, "weak_norm": x, "ident": x}[op] % F.p
        errs = []
        if value(limbs) * F.ri % F.p != want:
            errs.append("value")
        if canon != want:
            errs.append("canon")
        if bool(zero) != (want == 0):
            errs.append("zero")
        if op == "weak_norm":
            errs += ["digit%d" % i for i in range(8) if not -B28 - 3 <= limbs[i] <= B28 + 2]
        else:
            errs += ["digit%d" % i for i in range(8) if not -B28 <= limbs[i] <= B28]
        if abs(limbs[8]) > (1 << 25) + 1:         # operands are fe_to_mont outputs, below 2 p: |T| / R + p < 2 p < 2^257
            errs.append("digit8")
        return errs
    va, vb = value(a), value(b)
    T = op_product(op, va, vb)
    if T is not None:
        small = abs(T) // R + F.p < 16 * F.p                       # fe_from_mont / fe_is_zero want |value| < 16 p: decided from the inputs
        return product_errors(F, T, limbs, canon if small else None, zero if small else None)
    errs = weak_norm_errors(a, limbs) if op == "weak_norm" else (["value"] if limbs != list(a) else [])
    if abs(va) < 16 * F.p:
        if canon != va * F.ri % F.p:
            errs.append("canon")
        if bool(zero) != (va % F.p == 0):
            errs.append("zero")
    return errs


FIELD_CASES = [(op, 0, cls) for op in FIELD_OPS for cls in ("special_values", "random")] + \
              [(op, 1, cls) for op in ("mul", "sqr", "addsub_mul", "dbl_mul") for cls in ("limb_ends", "lazy", "quotient", "result_targets", "random_limbs")] + \
              [("weak_norm", 1, "limb_ends"), ("weak_norm", 1, "random_limbs"), ("ident", 1, "zero_multiples"), ("ident", 1, "zero_neighbours"),
               ("ident", 1, "random_limbs")]
FIELD_IDS = ["%s-%s-%s" % (op, "bytes" if form == 0 else "limbs", cls) for op, form, cls in FIELD_CASES]


def _field_case(dev, fname, op, form, cls):
    F = FIELDS[fname]
    flat, spans, limbs, canon, zero = field_run(dev, fname, op, form)
    lo, hi = spans[cls]
    assert hi - lo >= (NRANDOM if cls.startswith("random") else 24)
    print("vectors %s %s %s-%s: %d" % (fname, op, "bytes" if form == 0 else "limbs", cls, hi - lo))
    bad = []
    for i in range(lo, hi):
        e = field_case_errors(F, op, form, flat[i][0], flat[i][1], limbs[i], canon[i], zero[i])
        if e:
            bad.append((i - lo, e, flat[i]))
    assert not bad, (len(bad), bad[:3])
    if cls == "zero_multiples":
        assert all(zero[i] == 1 and canon[i] == 0 for i in range(lo, hi))
    if cls == "zero_neighbours":
        assert all(zero[i] == 0 for i in range(lo, hi))


@pytest.mark.gpu
@pytest.mark.parametrize("op,form,cls", FIELD_CASES, ids=FIELD_IDS)
def test_p256_field_on_device(dev, op, form, cls):
    """fe_mul / fe_sqr as FE29_GCN_MUL / FE29_GCN_SQR, fed by fe_add / fe_sub / fe_dbl; fe_weak_norm, fe_is_zero, to_mont -> from_mont."""
    _field_case(dev, "p256", op, form, cls)


@pytest.mark.gpu
@pytest.mark.parametrize("op,form,cls", FIELD_CASES, ids=FIELD_IDS)
def test_bn_field_on_device(dev, op, form, cls):
    """The same for fbn: BN29_GCN_MUL / BN29_GCN_SQR (bound L(a) L(b) <= 12)."""
    _field_case(dev, "bn", op, form, cls)


def scalar_run(dev, op):
    if ("scalar", op) in _cache:
        return _cache[("scalar", op)]
    base = "ecdsa_scalars29" if op == "pair_ecdsa_scalars29" else op
    vecs = scalar_vectors(base, random.Random("scalar/" + base))
    flat, spans = flatten(vecs)
    n = len(flat)
    assert n >= NRANDOM
    if base == "ecdsa_scalars29":
        assert all(c < N for _, _, c in flat)
    lanes = n * (2 if op == "pair_ecdsa_scalars29" else 1)
    out = np.zeros((lanes, 64), dtype=np.uint8)
    flag = np.zeros(lanes, dtype=np.uint32)
    a, b, c = (be_array([v[k] for v in flat]) for k in range(3))
    rc = dev.gputest_scalar_op(SCALAR_OPS[op], ctypes.c_uint32(n), _ptr(a), _ptr(b), _ptr(c), _ptr(out), _ptr(flag))
    assert rc == 0, rc
    vals = ints_of(out)
    _cache[("scalar", op)] = (flat, spans, vals, flag.tolist())
    return _cache[("scalar", op)]


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(SCALAR_OPS))
@pytest.mark.parametrize("cls", ["special_values", "random"])
def test_scalars_mod_n_on_device(dev, op, cls):
    """fp256.h on the device: the v_mad_u64_u32 / s_nop / v_addc_co_u32 mac behind fn_to_mont and fn_mul, the 256-bit helpers,
    range_status, and (u1, u2) from the one-lane and the lane-pair inversion - the pair's two lanes compared separately."""
    flat, spans, vals, flag = scalar_run(dev, op)
    lo, hi = spans[cls]
    assert hi - lo >= (NRANDOM if cls == "random" else 1000)
    print("vectors scalars %s-%s: %d" % (op, cls, hi - lo))
    base = "ecdsa_scalars29" if op == "pair_ecdsa_scalars29" else op
    per = 2 if op == "pair_ecdsa_scalars29" else 1
    bad = []
    for i in range(lo, hi):
        w0, w1, wf = scalar_want(base, *flat[i])
        for lane in range(per * i, per * i + per):
            got = (vals[2 * lane], vals[2 * lane + 1], flag[lane])
            if (w0 is not None and got[0] != w0) or (w1 is not None and got[1] != w1) or (wf is not None and got[2] != wf):
                bad.append((i - lo, "odd" if lane & 1 and per == 2 else "even/one", [hex(v) for v in flat[i]]))
    assert not bad, (len(bad), bad[:3])


def modinv_run(dev, mname, pair):
    key = ("modinv", mname, pair)
    if key in _cache:
        return _cache[key]
    which, m = MODULI[mname]
    lanes_per_wave = 32 if pair else 64
    xs, cls, known = inversion_vectors(m, random.Random("modinv/%s/%d" % (mname, pair)), lanes_per_wave)
    distinct, partial = inversion_census(xs, known, lanes_per_wave)
    assert distinct >= (3 if mname != "bnp" else 2) and partial and len(xs) >= NRANDOM
    lanes = len(xs) * (2 if pair else 1)
    out = np.zeros((lanes, 32), dtype=np.uint8)
    inp = be_array(xs)
    rc = dev.gputest_modinv(which, pair, ctypes.c_uint32(len(xs)), _ptr(inp), _ptr(out))
    assert rc == 0, rc
    _cache[key] = (xs, cls, ints_of(out))
    return _cache[key]


INV_CLASSES = ["wave_all_fast", "wave_one_slow", "wave_zero_beside_live", "wave_mixed_counts", "structured", "slow_search", "random_partial_last_wave"]


def _modinv_case(dev, mname, pair, cls):
    _, m = MODULI[mname]
    xs, classes, got = modinv_run(dev, mname, pair)
    idx = classes[cls]
    print("vectors %s %s-%s: %d" % ("pair_modinv" if pair else "modinv", mname, cls, len(idx)))
    per = 2 if pair else 1
    bad = []
    for i in idx:
        want = pow(xs[i], -1, m) if xs[i] else 0
        for lane in range(per * i, per * i + per):
            if got[lane] != want:
                bad.append((i, "odd" if lane & 1 and pair else "even/one", hex(xs[i])))
    assert not bad, (len(bad), bad[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("mname", list(MODULI))
@pytest.mark.parametrize("cls", INV_CLASSES)
def test_one_lane_inversion_on_device(dev, mname, cls):
    """modinv (modinv30.h) leaves its loop on a wave-wide ballot: lanes whose g is already 0 keep applying batches while a neighbour works."""
    _modinv_case(dev, mname, 0, cls)


@pytest.mark.gpu
@pytest.mark.parametrize("mname", list(MODULI))
@pytest.mark.parametrize("cls", INV_CLASSES)
def test_pair_inversion_on_device(dev, mname, cls):
    """pair_modinv (p256_pair29.h): one matrix column per lane, (f, g) on the even lane, (d, e) on the odd one, exit on __any; the
    result of each lane of the pair is compared on its own."""
    _modinv_case(dev, mname, 1, cls)


def point_run(dev, op):
    if ("point", op) in _cache:
        return _cache[("point", op)]
    vecs = point_vectors(op, random.Random("point/" + op))
    assert point_vector_census(op, vecs) == sum(len(v) for v in vecs.values())
    flat, spans = flatten(vecs)
    n = len(flat)
    assert n >= NRANDOM
    inp = np.array([l for l, _ in flat], dtype=np.int32)
    out = np.zeros((n, 45), dtype=np.int32)
    flag = np.zeros(n, dtype=np.uint32)
    rc = dev.gputest_point_op({"dbl": 0, "add": 1, "madd": 2}[op], ctypes.c_uint32(n), _ptr(inp), _ptr(out), _ptr(flag))
    assert rc == 0, rc
    _cache[("point", op)] = (flat, spans, out.tolist())
    return _cache[("point", op)]


POINT_CASES = [("dbl", c) for c in ("random_z", "lazy_representatives", "small_coordinates")] + \
              [("add", c) for c in ("random_z", "lazy_representatives", "p_plus_p", "p_plus_minus_p")] + \
              [("madd", c) for c in ("random_z", "lazy_representatives", "comb_corners", "p_plus_p", "p_plus_minus_p")]


@pytest.mark.gpu
@pytest.mark.parametrize("op,cls", POINT_CASES, ids=["%s-%s" % c for c in POINT_CASES])
def test_one_lane_point_ops_on_device(dev, op, cls):
    """pt_dbl29 / pt_add29 / pt_add_mixed29 as the device resolves them: the generated programs of one29_gcn.h."""
    flat, spans, out = point_run(dev, op)
    lo, hi = spans[cls]
    print("vectors points %s-%s: %d" % (op, cls, hi - lo))
    assert hi - lo >= (NRANDOM if cls == "random_z" else 48)
    bad = []
    for i in range(lo, hi):
        e = point_errors(op, flat[i][0], flat[i][1], out[i])
        if e:
            bad.append((i - lo, e))
    assert not bad, (len(bad), bad[:5])


ON_CURVE_CLASSES = ["on_curve", "y_off", "x_off", "negated_y"]


def on_curve_run(dev):
    """One launch, the four classes interleaved lane by lane so that every wavefront mixes verdicts."""
    if "on_curve" in _cache:
        return _cache["on_curve"]
    rng = random.Random("on_curve")
    pool = point_pool(rng, 1024)
    rows, want = [], []
    for k in range(NRANDOM):
        x, y = pool[k % len(pool)]
        kind = ON_CURVE_CLASSES[k % 4]
        if kind == "y_off":
            y = (y + 1 + rng.randrange(3)) % P
        elif kind == "x_off":
            x = (x + 1) % P
        elif kind == "negated_y":
            y = P - y
        rows.append(mont_rep(x) + mont_rep(y) + [0] * 36)
        want.append(1 if po.on_curve(x, y) else 0)
    inp = np.array(rows, dtype=np.int32)
    out = np.zeros((len(rows), 45), dtype=np.int32)
    flag = np.zeros(len(rows), dtype=np.uint32)
    assert dev.gputest_point_op(3, ctypes.c_uint32(len(rows)), _ptr(inp), _ptr(out), _ptr(flag)) == 0
    _cache["on_curve"] = (want, flag.tolist())
    return _cache["on_curve"]


@pytest.mark.gpu
@pytest.mark.parametrize("cls", ON_CURVE_CLASSES, ids=["on_curve29-" + c for c in ON_CURVE_CLASSES])
def test_on_curve29_on_device(dev, cls):
    """on_curve29 on Montgomery-form affine limbs: points of the curve, y moved off it, x moved off it, and the negated point."""
    want, got = on_curve_run(dev)
    idx = range(ON_CURVE_CLASSES.index(cls), NRANDOM, 4)
    print("vectors points on_curve29-%s: %d" % (cls, len(idx)))
    assert len(idx) == NRANDOM // 4
    if cls in ("on_curve", "negated_y"):
        assert all(want[i] == 1 for i in idx)
    else:
        assert sum(want[i] for i in idx) < len(idx) // 2           # x + 1 may land on the curve again; y + d never does
    if cls == "y_off":
        assert not any(want[i] for i in idx)
    assert [got[i] for i in idx] == [want[i] for i in idx]


def loop_run(dev, keyed):
    if ("loop", keyed) in _cache:
        return _cache[("loop", keyed)]
    rng = random.Random("loop")
    dq = rng.randrange(1, N)
    Q = po.pt_mul(dq, G)
    vecs = loop_vectors(rng, dq)
    flat, spans = flatten(vecs)
    assert len(flat) >= 240 and all(u1 < N and 0 < u2 < N for u1, u2 in flat)
    n = len(flat)
    inp = np.frombuffer(b"".join(be(u1) + be(u2) + be(Q[0]) + be(Q[1]) for u1, u2 in flat), dtype=np.uint8).copy()
    key = np.frombuffer(be(Q[0]) + be(Q[1]), dtype=np.uint8).copy()
    out = np.zeros((n, 28), dtype=np.int32)
    rc = dev.gputest_combined(keyed, ctypes.c_uint32(n), _ptr(key), _ptr(inp), _ptr(out))
    assert rc == 0, rc
    _cache[("loop", keyed)] = (flat, spans, Q, out.tolist())
    return _cache[("loop", keyed)]


def jacobian_errors(l27, inf, want):
    """X Y Z limbs + infinity flag against an affine point (None: infinity)."""
    if want is None:
        return [] if inf else ["not_infinity"]
    if inf:
        return ["infinity"]
    X, Y, Z = (fe_val(l27[9 * i:9 * i + 9]) for i in range(3))
    return [] if Z and X == want[0] * Z * Z % P and Y == want[1] * Z ** 3 % P else ["point"]


LOOP_CLASSES = ["adversarial_u2", "adversarial_u1", "recoding_edges", "final_add_doubling", "final_add_infinity"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fresh_key", "keyed"])
@pytest.mark.parametrize("cls", LOOP_CLASSES)
def test_one_lane_scalar_loops_on_device(dev, path, cls):
    """u1 G + u2 Q on one lane: comb_mult29 over the generator table, then either the Booth-window chain over the per-lane table
    (fresh key) or a second comb over the key's table (keyed), and final_add29 - x, y and the infinity flag against pt_mul / pt_add."""
    flat, spans, Q, out = loop_run(dev, 1 if path == "keyed" else 0)
    lo, hi = spans[cls]
    print("vectors loops %s-%s: %d" % (path, cls, hi - lo))
    assert hi - lo >= 3
    bad = []
    for i in range(lo, hi):
        e = jacobian_errors(out[i][:27], out[i][27], loop_want(flat[i][0], flat[i][1], Q))
        if e:
            bad.append((e, hex(flat[i][0]), hex(flat[i][1])))
    assert not bad, bad[:5]


def _pair_point_errors(rows, k, want, a_off, inf):
    """Pair state of signature k in the per-lane rows of the two older hooks: E holds A = X, B = Y; O holds B = Z."""
    e, o = rows[2 * k], rows[2 * k + 1]
    return jacobian_errors(e[a_off:a_off + 18] + o[a_off + 9:a_off + 18], inf, want)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", ["recoding_edges_and_final_add", "recoding_edges_rest_and_adversarial", "adversarial"])
def test_pair_combined_hook_on_device(dev, cls):
    """gputest_pair_combined as it stands: pair_combined_mult29 on one wavefront, 32 signatures a launch.  The first two cases
    together hold every recoding-edge u2 and every exceptional final addition."""
    rng = random.Random("pair_combined/" + cls)
    dq = rng.randrange(1, N)
    Q = po.pt_mul(dq, G)
    vecs = loop_vectors(rng, dq)
    if cls == "adversarial":
        flat = vecs["adversarial_u2"][:21] + vecs["adversarial_u1"][:11]
    elif cls == "recoding_edges_and_final_add":
        flat = vecs["recoding_edges"][:28] + vecs["final_add_doubling"][:2] + vecs["final_add_infinity"][:2]
    else:
        assert len(vecs["recoding_edges"]) == 30 and len(vecs["final_add_doubling"]) == len(vecs["final_add_infinity"]) == 3
        flat = vecs["recoding_edges"][28:] + vecs["final_add_doubling"][2:] + vecs["final_add_infinity"][2:] + vecs["adversarial_u2"][21:49]
    assert len(flat) == 32 and all(u1 < N and 0 < u2 < N for u1, u2 in flat)
    print("vectors pair_combined-%s: 32" % cls)
    inp = np.frombuffer(b"".join(be(u1) + be(u2) + be(Q[0]) + be(Q[1]) for u1, u2 in flat), dtype=np.uint8).copy()
    out = np.zeros((64, 19), dtype=np.int32)
    assert dev.gputest_pair_combined(_ptr(inp), _ptr(out)) == 0
    rows = out.tolist()
    bad = []
    for k, (u1, u2) in enumerate(flat):
        want = loop_want(u1, u2, Q)
        if rows[2 * k][18] != rows[2 * k + 1][18]:
            bad.append(("r_inf differs between the lanes", k))
        e = _pair_point_errors(rows, k, want, 0, rows[2 * k][18])
        if e:
            bad.append((e, hex(u1), hex(u2)))
    assert not bad, bad[:5]


VERIFY_CASES = {"recoding_edges_and_gates": 0, "recoding_edges_rest_and_adversarial": 1}


def _verify_rows(rng, part):
    """32 rows (qx, qy, e, r, s) for gputest_pair_verify with what Python expects of each, and how many of the leading rows are valid
    signatures built for a chosen u2.  Part 0: the first 22 recoding-edge u2, then gated / wrong rows;  part 1: the other 8
    recoding-edge u2 and 24 adversarial ones.  The two parts together hold every recoding-edge u2."""
    rows = []
    edges = edge_u2_targets()
    assert len(edges) == 30
    targets = edges[:22] if part == 0 else edges[22:] + adversarial_u2s(rng)[:24]
    for u2 in targets:
        while True:
            k = rng.randrange(1, N)
            r = po.pt_mul(k, G)[0] % N
            s = r * pow(u2, -1, N) % N
            e = rng.getrandbits(256)
            d = (s * k - e) * pow(r, -1, N) % N if r else 0
            if r and d and po.is_low_s(s):
                break
        rows.append((po.pt_mul(d, G), e, r, s))
    if part == 1:
        assert len(rows) == 32
        return rows, 32
    d = rng.randrange(1, N)
    Q = po.pt_mul(d, G)
    e = rng.getrandbits(256)
    r, s = po.sign_raw(d, be(e), rng.randrange(1, N))
    rows += [(Q, e, r, s), (Q, e ^ 1, r, s), (Q, e, r, N - s), (Q, e, 0, s), (Q, e, r, 0), (Q, e, N, s), (Q, e, (r + 1) % N, s),
             ((Q[0], (Q[1] + 1) % P), e, r, s), (Q, 0, r, s), (Q, N, r, s)]
    assert len(rows) == 32
    return rows, 22


@pytest.mark.gpu
@pytest.mark.parametrize("cls", list(VERIFY_CASES))
def test_pair_verify_hook_on_device(dev, cls):
    """gputest_pair_verify as it stands: the internals of p256_verify_pair29 - u1, u2 on both lanes, the early gate status, r_inf,
    ok1 (X == r Z^2 on the even lane) and the final status - against Python."""
    rows, n_valid = _verify_rows(random.Random("pair_verify/" + cls), VERIFY_CASES[cls])
    print("vectors pair_verify-%s: 32" % cls)
    inp = np.frombuffer(b"".join(be(Q[0]) + be(Q[1]) + be(e) + be(r) + be(s) for Q, e, r, s in rows), dtype=np.uint8).copy()
    out = np.zeros((64, 48), dtype=np.int32)
    assert dev.gputest_pair_verify(_ptr(inp), _ptr(out)) == 0
    o = out.tolist()
    words = lambda row, off: sum((row[off + i] & 0xFFFFFFFF) << (32 * i) for i in range(8))
    bad = []
    n_chain = 0
    for k, (Q, e, r, s) in enumerate(rows):
        early = range_status(r, s)
        on = po.on_curve(*Q)
        if early == po.ST_VALID and not on:
            early = po.ST_OFF_CURVE
        w = pow(s, -1, N) if s else 0
        u1, u2 = (e % N) * w % N, r * w % N
        for lane in (2 * k, 2 * k + 1):
            if (words(o[lane], 0), words(o[lane], 8)) != (u1, u2):
                bad.append(("u1 u2", k, lane & 1))
            if o[lane][37] != early:
                bad.append(("early", k, lane & 1, o[lane][37], early))
        Rw = loop_want(u1, u2, Q) if on else None
        want_st = early if early != po.ST_VALID else (po.ST_VALID if Rw is not None and Rw[0] % N == r else po.ST_BAD_MATH)
        if o[2 * k][34] != want_st:
            bad.append(("status", k, o[2 * k][34], want_st))
        if on and u2:                                     # the point chain is defined: decided from the inputs
            n_chain += 1
            if o[2 * k][36] != (1 if Rw is None else 0) or o[2 * k + 1][36] != o[2 * k][36]:
                bad.append(("r_inf", k))
            if Rw is not None:
                if _pair_point_errors(o, k, Rw, 16, 0):
                    bad.append(("point", k))
                if o[2 * k][35] != (1 if Rw[0] == r else 0):
                    bad.append(("ok1", k, o[2 * k][35]))
    assert n_chain >= 28
    assert not bad, bad[:8]
    assert [o[2 * k][34] for k in range(n_valid)] == [0] * n_valid
