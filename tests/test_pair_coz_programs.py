"""PAIR29_DBLU and PAIR29_ZADDU (fabric-mod_amd/csrc/gen_pair_gcn.py build_pair_dblu / build_pair_zaddu): the doubling with update and
the co-Z addition with update that build the LDS table of odd multiples {Q, 3Q, .., 15Q} of the pair kernels.

CPU: the very instruction lists run in gcn_dsl.Program.run() against big-integer point arithmetic - random points, Z = 1, inputs at the
corners of their contracts, the whole table with the updated 2Q after every step - and Program.run_intervals closes the contracts
(gen_pair_gcn.coz_closed, part of contracts_closed) and refuses a widened input range.
GPU: each generated statement on one wavefront (gputest ops 8 and 9), every output register of every lane against the interpreter."""
import os
import random
import sys

import numpy as np
import pytest

import bccsp_sw_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-mod_amd", "csrc"))
import gen_pair_gcn as gp  # noqa: E402

P = po.P
R = 1 << 261
RI = pow(R, -1, P)
G = (po.GX, po.GY)


def bal(x):
    d = []
    for _ in range(8):
        t = x & ((1 << 29) - 1)
        if t >> 28:
            t -= 1 << 29
        d.append(t)
        x = (x - t) >> 29
    d.append(x)
    return d


def to_fe(x):
    return bal(x * R % P)


def digits_value(d):
    return sum(x << (29 * i) for i, x in enumerate(d)) * RI % P


def val(regs, name):
    return digits_value([regs["%s.%d" % (name, i)] for i in range(9)])


def put(regs, name, digits):
    for i in range(9):
        regs["%s.%d" % (name, i)] = digits[i]


def affine(X, Y, Z):
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def inside(regs, name, c):
    return all(c[0] <= regs["%s.%d" % (name, i)] <= c[1] for i in range(8)) and c[2] <= regs["%s.8" % name] <= c[3]


def junk(rng):
    return [rng.randrange(-(1 << 28), 1 << 28) for _ in range(9)]


def edge(rng, c, pattern):
    pick = {"hi": lambda i: 1, "lo": lambda i: 0, "alt": lambda i: i & 1, "tla": lambda i: 1 - (i & 1), "rnd": lambda i: rng.randrange(2)}[pattern]
    return [c[1] if pick(i) else c[0] for i in range(8)] + [c[3] if pick(8) else c[2]]


def zaddu_values(x1, y1, x2, y2, z):
    """The co-Z addition with update on VALUES: (X3, Y3, Z3, W1, A1)."""
    c, d = (x1 - x2) ** 2 % P, (y1 - y2) ** 2 % P
    w1, w2 = x1 * c % P, x2 * c % P
    a1 = y1 * (w1 - w2) % P
    x3 = (d - w1 - w2) % P
    return x3, ((y1 - y2) * (w1 - x3) - a1) % P, z * (x1 - x2) % P, w1, a1


def dblu_values(x, y, z):
    """The doubling (a = -3) on VALUES and the two products that are the update for z = 1: (X3, Y3, Z3, 4 x y^2, 8 y^4)."""
    g, d = y * y % P, z * z % P
    b4, al = 4 * x * g % P, 3 * (x - d) * (x + d) % P
    x3 = (al * al - 2 * b4) % P
    return x3, (al * (b4 - x3) - 8 * g * g) % P, 2 * y * z % P, b4, 8 * g * g % P


def run_zaddu(prog, rng, X2, Y2, Z, X1, Y1):
    """Digits in, (even lane, odd lane) registers out; every limb must still be a 32-bit value."""
    e, o = {}, {}
    put(e, "A", X2); put(e, "B", Y2); put(e, "DX", X1); put(e, "DY", Y1)
    put(o, "A", junk(rng)); put(o, "B", Z); put(o, "DX", junk(rng)); put(o, "DY", junk(rng))
    re_, ro = prog.run(e, o)
    assert all(-(1 << 31) <= v < (1 << 31) for regs in (re_, ro) for v in regs.values())
    return re_, ro


def run_dblu(prog, rng, X, Y, Z):
    e, o = {}, {}
    put(e, "A", X); put(e, "B", Y); put(o, "A", junk(rng)); put(o, "B", Z)
    re_, ro = prog.run(e, o)
    assert all(-(1 << 31) <= v < (1 << 31) for regs in (re_, ro) for v in regs.values())
    return re_, ro


@pytest.fixture(scope="module")
def zaddu():
    return gp.build_pair_zaddu()


@pytest.fixture(scope="module")
def dblu():
    return gp.build_pair_dblu()


def test_program_sizes(zaddu, dblu):
    """Four product steps: a little over half of the general addition's 1364 instructions, and the doubling with update costs what a
    doubling costs (732) plus the balanced digits its update needs."""
    nz = zaddu.emit_asm({n: "(%s)" % n for n in zaddu.order})[1]
    nd = dblu.emit_asm({n: "(%s)" % n for n in dblu.order})[1]
    na = gp.build_pair_add().emit_asm({n: "(%s)" % n for n in gp.build_pair_add().order})[1]
    assert na["instructions"] == 1364
    assert nz["instructions"] < 800 and nz["nops"] == 0, nz
    assert nd["instructions"] < 780 and nd["nops"] == 0, nd
    assert sum(1 for x in zaddu.ins if x[0] == "prod_begin") == 4 and sum(1 for x in dblu.ins if x[0] == "prod_begin") == 4


def test_zaddu_on_random_points_and_z_one(zaddu):
    rng = random.Random(1001)
    for trial in range(12):
        p1 = po.pt_mul(rng.randrange(1, po.N), G)
        p2 = po.pt_mul(rng.randrange(1, po.N), G)
        z = 1 if trial < 3 else rng.randrange(1, P)
        X1, Y1, X2, Y2 = p1[0] * z * z % P, p1[1] * z ** 3 % P, p2[0] * z * z % P, p2[1] * z ** 3 % P
        re_, ro = run_zaddu(zaddu, rng, to_fe(X2), to_fe(Y2), to_fe(z), to_fe(X1), to_fe(Y1))
        got = (val(re_, "AO"), val(re_, "BO"), val(ro, "BO"), val(re_, "DXO"), val(re_, "DYO"))
        assert got == zaddu_values(X1, Y1, X2, Y2, z)
        assert affine(got[0], got[1], got[2]) == po.pt_add(p1, p2)
        assert affine(got[3], got[4], got[2]) == p1                     # the same point over the sum's Z


def test_zaddu_at_the_corners_of_its_contracts(zaddu):
    """(A, B) a state, (DX, DY) the other point's contract (gen_pair_gcn.coz_other), every digit at an extreme: the exact 32 / 64-bit
    interpreter must give the formulas' values (such inputs are not curve points; the formulas do not care) and leave contracts."""
    rng = random.Random(1002)
    S, D = gp.STATE_P256, gp.coz_other(gp.STATE_P256)
    for pattern in ("hi", "lo", "alt", "tla", "rnd", "rnd", "rnd", "rnd", "rnd", "rnd"):
        for other in (pattern, "rnd"):
            X2, Y2, Z = edge(rng, S["X"], pattern), edge(rng, S["Y"], pattern), edge(rng, S["Z"], pattern)
            X1, Y1 = edge(rng, D["X"], other), edge(rng, D["Y"], "lo" if other == "hi" else other)      # (Y1 low against Y2 high: the widest dy)
            re_, ro = run_zaddu(zaddu, rng, X2, Y2, Z, X1, Y1)
            got = (val(re_, "AO"), val(re_, "BO"), val(ro, "BO"), val(re_, "DXO"), val(re_, "DYO"))
            assert got == zaddu_values(digits_value(X1), digits_value(Y1), digits_value(X2), digits_value(Y2), digits_value(Z)), (pattern, other)
            assert inside(re_, "AO", S["X"]) and inside(re_, "BO", S["Y"]) and inside(ro, "BO", S["Z"]), (pattern, other)
            assert inside(re_, "DXO", D["X"]) and inside(re_, "DYO", D["Y"]), (pattern, other)


def test_dblu_on_affine_points_and_at_the_corners(dblu):
    rng = random.Random(1003)
    S, D = gp.STATE_P256, gp.coz_other(gp.STATE_P256)
    one = to_fe(1)
    for _ in range(8):
        q = po.pt_mul(rng.randrange(1, po.N), G)
        re_, ro = run_dblu(dblu, rng, to_fe(q[0]), to_fe(q[1]), one)
        got = (val(re_, "A"), val(re_, "B"), val(ro, "B"), val(re_, "DXO"), val(re_, "DYO"))
        assert got == dblu_values(q[0], q[1], 1)
        assert affine(got[0], got[1], got[2]) == po.pt_add(q, q)
        assert affine(got[3], got[4], got[2]) == q                      # Q over 2Q's Z
    for pattern in ("hi", "lo", "alt", "tla", "rnd", "rnd", "rnd", "rnd"):
        X, Y, Z = edge(rng, gp.AFFINE, pattern), edge(rng, gp.AFFINE, pattern), edge(rng, gp.AFFINE, pattern)
        re_, ro = run_dblu(dblu, rng, X, Y, Z)
        got = (val(re_, "A"), val(re_, "B"), val(ro, "B"), val(re_, "DXO"), val(re_, "DYO"))
        assert got == dblu_values(digits_value(X), digits_value(Y), digits_value(Z)), pattern
        assert inside(re_, "A", D["X"]) and inside(re_, "B", D["Y"]) and inside(ro, "B", S["Z"]), pattern      # the first (DX, DY), and a Z
        assert inside(re_, "DXO", S["X"]) and inside(re_, "DYO", S["Y"]), pattern                             # the first (A, B)


def test_the_whole_table_and_the_updated_2q_after_every_step(zaddu, dblu):
    """pair_qtab_build_odd29's sequence in the interpreter: slot 1 = Q, a doubling with update, seven co-Z additions.  Every entry equals
    (2j - 1) Q, is a state, and the carried point equals 2Q over the entry's Z after every step."""
    rng = random.Random(1004)
    S, D = gp.STATE_P256, gp.coz_other(gp.STATE_P256)
    one = to_fe(1)
    for trial in range(3):
        q = po.pt_mul(rng.randrange(1, po.N), G)
        q2 = po.pt_add(q, q)
        table = {1: q}
        re_, ro = run_dblu(dblu, rng, to_fe(q[0]), to_fe(q[1]), one)
        grab = lambda regs, n: [regs["%s.%d" % (n, i)] for i in range(9)]
        DX, DY = grab(re_, "A"), grab(re_, "B")
        cur = (grab(re_, "DXO"), grab(re_, "DYO"), grab(ro, "B"))
        assert affine(digits_value(DX), digits_value(DY), digits_value(cur[2])) == q2
        for j in range(2, 9):
            re_, ro = run_zaddu(zaddu, rng, cur[0], cur[1], cur[2], DX, DY)
            cur = (grab(re_, "AO"), grab(re_, "BO"), grab(ro, "BO"))
            DX, DY = grab(re_, "DXO"), grab(re_, "DYO")
            table[j] = affine(*(digits_value(d) for d in cur))
            assert table[j] == po.pt_mul(2 * j - 1, q), j
            assert affine(digits_value(DX), digits_value(DY), digits_value(cur[2])) == q2, j
            assert inside(re_, "AO", S["X"]) and inside(re_, "BO", S["Y"]) and inside(ro, "BO", S["Z"]), j
            assert inside(re_, "DXO", D["X"]) and inside(re_, "DYO", D["Y"]), j
        assert len(set(table.values())) == 8


def test_contracts_close_with_the_new_programs_and_refuse_a_widened_input(zaddu, dblu):
    S = gp.STATE_P256
    U = gp.coz_closed(zaddu, dblu)
    for k in "XYZ":
        assert S[k][0] <= U[k][0] and U[k][1] <= S[k][1] and S[k][2] <= U[k][2] and U[k][3] <= S[k][3], (k, U[k])
    # the generator's own check covers them, named or not
    classic = {"dbl": gp.build_pair_dbl(), "add": gp.build_pair_add(), "madd": gp.build_pair_madd()}
    gp.contracts_closed(classic, S)
    gp.contracts_closed(dict(classic, zaddu=zaddu, dblu=dblu), S)
    # ... and says no: the other point's Y as wide as a state's Y (dy = DY - B is squared), a wider state, unsigned digits where they may not be
    full_y = gp.build_pair_zaddu()
    e, o = {}, {}
    e.update(gp.fe_range("A", S["X"])); e.update(gp.fe_range("B", S["Y"])); o.update(gp.fe_range("B", S["Z"]))
    e.update(gp.fe_range("DX", S["X"])); e.update(gp.fe_range("DY", S["Y"]))
    with pytest.raises(OverflowError):
        full_y.run_intervals(e, o)
    wide = dict(S, Y=(-4 << 28, 4 << 28, -4 << 24, 3 << 24))
    with pytest.raises(OverflowError):
        gp.coz_closed(zaddu, dblu, wide)
    with pytest.raises(OverflowError):
        gp.contracts_closed(dict(classic, zaddu=gp.build_pair_zaddu((0, 1, 2, 3)), dblu=dblu), S)
    with pytest.raises(OverflowError):
        gp.contracts_closed(dict(classic, zaddu=zaddu, dblu=gp.build_pair_dblu((2,))), S)


# ---- on the device ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op,name", [(8, "dblu"), (9, "zaddu")])
def test_coz_streams_on_gpu_match_the_interpreter_register_for_register(zaddu, dblu, op, name):
    """One wavefront (32 lane pairs) runs the generated statement; every output limb of every lane - the don't-care lanes included -
    must equal what Program.run() computes for the same inputs.  Even pairs hold curve points, odd pairs digits anywhere in the
    contracts, their extremes included."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_gputest.so"))
    rng = random.Random(1005 + op)
    S, D = gp.STATE_P256, gp.coz_other(gp.STATE_P256)
    prog = dblu if name == "dblu" else zaddu
    anyof = lambda c: [rng.choice((c[0], c[1], rng.randrange(c[0], c[1] + 1))) for _ in range(8)] + [rng.choice((c[2], c[3], rng.randrange(c[2], c[3] + 1)))]
    inp = np.zeros((64, 36), dtype=np.int32)
    want = {}
    for k in range(32):
        if name == "dblu":
            if k & 1:
                e = {"A": anyof(gp.AFFINE), "B": anyof(gp.AFFINE)}
                o = {"A": junk(rng), "B": anyof(gp.AFFINE)}
            else:
                q = po.pt_mul(rng.randrange(1, po.N), G)
                e = {"A": to_fe(q[0]), "B": to_fe(q[1])}
                o = {"A": junk(rng), "B": to_fe(1)}
            for regs in (e, o):
                regs.update(C=junk(rng), D=junk(rng))
        else:
            if k & 1:
                e = {"A": anyof(S["X"]), "B": anyof(S["Y"]), "C": anyof(D["X"]), "D": anyof(D["Y"])}
                o = {"A": junk(rng), "B": anyof(S["Z"]), "C": junk(rng), "D": junk(rng)}
            else:
                p1, p2 = po.pt_mul(rng.randrange(1, po.N), G), po.pt_mul(rng.randrange(1, po.N), G)
                z = rng.randrange(1, P)
                e = {"A": to_fe(p2[0] * z * z % P), "B": to_fe(p2[1] * z ** 3 % P), "C": to_fe(p1[0] * z * z % P), "D": to_fe(p1[1] * z ** 3 % P)}
                o = {"A": junk(rng), "B": to_fe(z), "C": junk(rng), "D": junk(rng)}
        for lane, regs in ((2 * k, e), (2 * k + 1, o)):
            inp[lane] = regs["A"] + regs["B"] + regs["C"] + regs["D"]
        re_, ro = {}, {}
        for src, dst in (("A", "A"), ("B", "B")) + ((("C", "DX"), ("D", "DY")) if name == "zaddu" else ()):
            put(re_, dst, e[src]); put(ro, dst, o[src])
        want[k] = prog.run(re_, ro)
    out = np.zeros((64, 36), dtype=np.int32)
    assert lib.gputest_pair_op(op, inp.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == 0
    names = (["A", "B"] if name == "dblu" else ["AO", "BO"]) + ["DXO", "DYO"]
    bad = set()
    for k in range(32):
        for lane, regs in ((2 * k, want[k][0]), (2 * k + 1, want[k][1])):
            for j, nm in enumerate(names):
                got = [int(v) for v in out[lane, 9 * j:9 * j + 9]]
                exp = [regs["%s.%d" % (nm, i)] for i in range(9)]
                if got != exp:
                    bad.add((nm, "odd" if lane & 1 else "even", tuple(i for i in range(9) if got[i] != exp[i])))
    assert not bad, (name, sorted(bad))
