"""PAIR29_DBL4 (fabric-mod_amd/csrc/gen_pair_gcn.py build_pair_dbln): the four doublings of a 4-bit window as ONE generated program.

CPU: the very instruction list runs in gcn_dsl.Program.run() on random states and on states at the corners of the state contract,
against four big-integer doublings and against four runs of the one-doubling program; Program.run_intervals closes STATE -> DBL4 ->
STATE (the contract BETWEEN the inner doublings is whatever the intervals give: it is printed when something fails).
GPU: the generated asm statement on one wavefront, every output register of every lane against the interpreter; and the whole verify
kernel with DBL4 (the default) against the per-doubling loop (FABGPU_FLAG_PAIR_DBL1), the one-wave form (FABGPU_FLAG_PAIR_SOLO) and the
CPU oracle, bit for bit, at batch sizes around a wavefront and a tile and on the scalars and keys where a window's doublings could differ."""
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


def val(regs, name):
    return sum(regs["%s.%d" % (name, i)] << (29 * i) for i in range(9)) * RI % P


def put(regs, name, digits):
    for i in range(9):
        regs["%s.%d" % (name, i)] = digits[i]


def dbl_values(x, y, z):
    """One doubling on the VALUES (a = -3), the formulas of build_pair_dbl: no curve membership asked."""
    g, d = y * y % P, z * z % P
    b4, al = 4 * x * g % P, 3 * (x - d) * (x + d) % P
    x3 = (al * al - 2 * b4) % P
    return x3, (al * (b4 - x3) - 8 * g * g) % P, 2 * y * z % P


@pytest.fixture(scope="module")
def dbl4():
    return gp.build_pair_dbl4()


@pytest.fixture(scope="module")
def dbl1():
    return gp.build_pair_dbl()


def inner_report():
    return "options per doubling %r; derived inner contracts %r" % ([sorted(o) for o in gp.dbln_options(4)], gp.dbln_inner_contracts(4))


def test_dbl4_is_shorter_than_four_doublings(dbl4, dbl1):
    n4 = dbl4.emit_asm({n: "(%s)" % n for n in dbl4.order})[1]
    n1 = dbl1.emit_asm({n: "(%s)" % n for n in dbl1.order})[1]
    assert n1["instructions"] == 732
    assert n4["instructions"] < 4 * n1["instructions"], n4          # scalar instructions (EXEC switches, pads) counted
    assert n4["nops"] == 0
    # the parameter the generator offers instead of a second hand-written program: two doublings twice
    d2 = gp.build_pair_dbln(2)
    assert d2.name == "PAIR29_DBL2" and d2.emit_asm({n: "(%s)" % n for n in d2.order})[1]["instructions"] < 2 * n1["instructions"]


def test_dbl4_contract_is_closed_by_intervals(dbl4):
    try:
        U = gp.dbln_closed(dbl4)
    except OverflowError as e:
        raise AssertionError("%s; %s" % (e, inner_report()))
    S = gp.STATE_P256
    for k in "XYZ":
        assert S[k][0] <= U[k][0] and U[k][1] <= S[k][1] and S[k][2] <= U[k][2] and U[k][3] <= S[k][3], (k, U[k], inner_report())
    inner = gp.dbln_inner_contracts(4)
    assert len(inner) == 4 and inner[3] == U, inner_report()
    # and the check the generator applies before it writes the header covers the program
    gp.contracts_closed({"dbl": gp.build_pair_dbl(), "add": gp.build_pair_add(), "madd": gp.build_pair_madd()}, S)
    # the proof can say no: with every step of every doubling taken (unsigned digits everywhere, gamma^2 with the factor -8) it does
    with pytest.raises(OverflowError):
        gp.dbln_closed(gp.build_pair_dbln(4, [frozenset(gp.DBLN_STEPS)] * 4))


def test_dbl4_on_random_states_and_at_the_edge_of_the_state_contract(dbl4, dbl1):
    """Random curve points in Jacobian form, and every input digit at an extreme of the state contract (all high, all low, alternating,
    random): the result equals four big-integer doublings, equals four runs of the one-doubling program modulo p, and lies inside the
    state contract.  The interpreter's arithmetic is exact 32 / 64-bit: a wrap shows as a wrong value."""
    rng = random.Random(808)
    S = gp.STATE_P256

    def edge(c, pattern):
        pick = {"hi": lambda i: 1, "lo": lambda i: 0, "alt": lambda i: i & 1, "tla": lambda i: 1 - (i & 1), "rnd": lambda i: rng.randrange(2)}[pattern]
        return [c[1] if pick(i) else c[0] for i in range(8)] + [c[3] if pick(8) else c[2]]

    def v(d):
        return sum(x << (29 * i) for i, x in enumerate(d)) * RI % P

    def inside(regs, name, c):
        return all(c[0] <= regs["%s.%d" % (name, i)] <= c[1] for i in range(8)) and c[2] <= regs["%s.8" % name] <= c[3]
    cases = []
    for _ in range(6):
        pt = po.pt_mul(rng.randrange(1, po.N), (po.GX, po.GY))
        z = rng.randrange(1, P)
        cases.append(("point", to_fe(pt[0] * z * z % P), to_fe(pt[1] * z * z * z % P), to_fe(z)))
    for pattern in ("hi", "lo", "alt", "tla", "rnd", "rnd", "rnd", "rnd", "rnd", "rnd"):
        cases.append((pattern, edge(S["X"], pattern), edge(S["Y"], pattern), edge(S["Z"], pattern)))
    for pattern, X, Y, Z in cases:
        e, o = {}, {}
        put(e, "A", X); put(e, "B", Y); put(o, "A", edge(gp.AFFINE, "rnd")); put(o, "B", Z)
        re4, ro4 = dbl4.run(dict(e), dict(o))
        assert all(-(1 << 31) <= x < (1 << 31) for regs in (re4, ro4) for x in regs.values())
        want = (v(X), v(Y), v(Z))
        e1, o1 = dict(e), dict(o)
        for _ in range(4):
            want = dbl_values(*want)
            e1, o1 = dbl1.run({k: x for k, x in e1.items() if k[:2] in ("A.", "B.")}, {k: x for k, x in o1.items() if k[:2] in ("A.", "B.")})
        got = (val(re4, "A"), val(re4, "B"), val(ro4, "B"))
        assert got == want, (pattern, inner_report())
        assert got == (val(e1, "A"), val(e1, "B"), val(o1, "B")), (pattern, inner_report())
        assert inside(re4, "A", S["X"]) and inside(re4, "B", S["Y"]) and inside(ro4, "B", S["Z"]), (pattern, inner_report())
        if pattern == "point":
            zi = pow(got[2], -1, P)
            acc = po.pt_mul(16, (v(X) * pow(v(Z), -2, P) % P, v(Y) * pow(v(Z), -3, P) % P))
            assert (got[0] * zi * zi % P, got[1] * zi * zi * zi % P) == acc


# ---- on the device ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dbl4_stream_on_gpu_matches_the_interpreter_register_for_register(dbl4):
    """One wavefront (32 lane pairs) runs the generated statement (gputest op 7); every output limb of every lane - the don't-care lanes
    included, the lane masks make them deterministic too - must equal what Program.run() computes for the same inputs."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_gputest.so"))
    rng = random.Random(809)
    S = gp.STATE_P256
    inp = np.zeros((64, 36), dtype=np.int32)
    want = {}
    for k in range(32):
        junk = lambda: [rng.randrange(-(1 << 28), 1 << 28) for _ in range(9)]
        anyof = lambda c: [rng.choice((c[0], c[1], rng.randrange(c[0], c[1] + 1))) for _ in range(8)] + [rng.choice((c[2], c[3], rng.randrange(c[2], c[3] + 1)))]
        if k & 1:          # digits anywhere in the state contract, its extremes included
            e = {"A": anyof(S["X"]), "B": anyof(S["Y"])}
            o = {"A": junk(), "B": anyof(S["Z"])}
        else:
            pt = po.pt_mul(rng.randrange(1, po.N), (po.GX, po.GY))
            z = rng.randrange(1, P)
            e = {"A": to_fe(pt[0] * z * z % P), "B": to_fe(pt[1] * z * z * z % P)}
            o = {"A": junk(), "B": to_fe(z)}
        for regs in (e, o):
            regs.update(C=junk(), D=junk())
        for lane, regs in ((2 * k, e), (2 * k + 1, o)):
            inp[lane] = regs["A"] + regs["B"] + regs["C"] + regs["D"]
        re_, ro = {}, {}
        for nm in "AB":
            put(re_, nm, e[nm]); put(ro, nm, o[nm])
        want[k] = dbl4.run(re_, ro)
    out = np.zeros((64, 36), dtype=np.int32)
    assert lib.gputest_pair_op(7, inp.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == 0
    bad = set()
    for k in range(32):
        for lane, regs in ((2 * k, want[k][0]), (2 * k + 1, want[k][1])):
            for j, nm in enumerate(("A", "B")):
                got = [int(x) for x in out[lane, 9 * j:9 * j + 9]]
                exp = [regs["%s.%d" % (nm, i)] for i in range(9)]
                if got != exp:
                    bad.add((nm, "odd" if lane & 1 else "even", tuple(i for i in range(9) if got[i] != exp[i])))
    assert not bad, sorted(bad)


def _be(x):
    return int(x).to_bytes(32, "big")


def _row_for_u2(rng, u2):
    """A valid low-S signature whose u2 = r / s is the given scalar."""
    for _ in range(400):
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
        return [_be(Q[0]), _be(Q[1]), _be(e), _be(r), _be(s)]
    raise AssertionError("no low-S signature for u2 = %x" % u2)


@pytest.fixture(scope="module")
def special_rows():
    """(row, expected status or None): the scalars and keys the issue names.  Computed once, shared by every size."""
    rng = np.random.default_rng(810)
    rows = []
    rows.append((_row_for_u2(rng, po.N - 2), 0))                                   # the one exceptional scalar of W = 4
    rows.append((_row_for_u2(rng, (1 << 180) + 0x1234567), 0))                     # top windows zero: t_inf stays set through 19 DBL4s
    rows.append((_row_for_u2(rng, 5), 0))                                          # ... through all but the last
    mid = (0xF123456789ABCDEF << 192) | 0xFEDCBA987654321                          # zero digits in the middle (bits 60 .. 191)
    rows.append((_row_for_u2(rng, mid), 0))
    rows.append((_row_for_u2(rng, (0x8001 << 240) | (1 << 128) | (0x7 << 61) | 1), 0))
    base = _row_for_u2(rng, int(rng.integers(1, 1 << 62)) ** 4 % po.N)
    qx, qy = int.from_bytes(base[0], "big"), int.from_bytes(base[1], "big")
    rows.append(([_be(qx + P) if qx + P < (1 << 256) else _be(P), base[1], base[2], base[3], base[4]], 4))     # qx >= p: qx + p, or p itself
    rows.append(([_be(P + 1), base[1], base[2], base[3], base[4]], 4))                                          # ... strictly above p
    rows.append(([_be((1 << 256) - 1), base[1], base[2], base[3], base[4]], 4))                                 # ... the largest field of 32 bytes
    rows.append(([base[0], _be(qy + P) if qy + P < (1 << 256) else _be((1 << 256) - 1), base[2], base[3], base[4]], 4))  # qy >= p
    rows.append(([base[0], _be((qy + 1) % P), base[2], base[3], base[4]], 4))      # off the curve
    return rows


@pytest.fixture(scope="module")
def verify_forms():
    import fabgpu
    forms = {"dbl4": fabgpu.Context(device=0, flags=fabgpu.FLAG_PAIR_TABLE_LDS),
             "dbl1": fabgpu.Context(device=0, flags=fabgpu.FLAG_PAIR_TABLE_LDS | fabgpu.FLAG_PAIR_DBL1),
             "solo": fabgpu.Context(device=0, flags=fabgpu.FLAG_PAIR_TABLE_LDS | fabgpu.FLAG_PAIR_SOLO),
             "solo-dbl1": fabgpu.Context(device=0, flags=fabgpu.FLAG_PAIR_TABLE_LDS | fabgpu.FLAG_PAIR_SOLO | fabgpu.FLAG_PAIR_DBL1)}
    yield forms
    for c in forms.values():
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 257])
def test_whole_verify_dbl4_against_the_doubling_loop_the_solo_form_and_the_oracle(verify_forms, special_rows, n):
    """Verdict words and status bytes bit-identical between DBL4 (default), FABGPU_FLAG_PAIR_DBL1, FABGPU_FLAG_PAIR_SOLO and the CPU oracle:
    a partial wave, a partial tile, a second tile through the two-barrier handoff; 1 % invalid, and the special rows spread over the batch
    (a batch smaller than their number: one batch per special row)."""
    import coracle
    import fabgpu
    b = fabgpu.synth_batch(n, seed=8000 + n, invalid_permille=10)
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
        got = {m: c.p256_verify_batch(*cols) for m, c in verify_forms.items()}
        for m, (bits, st) in got.items():
            print(n, m, "status", st[:8].tolist(), "mismatches against the oracle", int((st != want).sum()))
        for m, (bits, st) in got.items():
            assert (st == want).all(), (m, np.nonzero(st != want)[0][:20])
            assert (bits == (want == 0)).all(), m
            assert (st == got["dbl1"][1]).all() and (bits == got["dbl1"][0]).all(), m
