"""The 16-bit comb tables of registered P-384 keys on the host compilation (csrc/p384_tables16.h) through the stand-alone program
csrc/hosttest_p384_tables16.cpp: the host builder build_comb384x16 against Python integers (p384_ref.py), and the 24-window instantiation
of verify_core_keyed beside the 48-window one and the reference.  No device."""
import os
import random
import subprocess

import pytest

import p384_keyed_cases as K
import p384_ref as R
import p384_tables16_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fabric-mod_amd", "csrc")
WINDOWS = (0, 11, 23)


@pytest.fixture(scope="module")
def exe():
    """csrc/hosttest_p384_tables16.cpp without sanitizers, through the Makefile (`make sanitize-p384-tables16 P384_T16_CASES=...` runs the
    same program under -fsanitize=address,undefined)"""
    out = subprocess.run(["make", "-C", CSRC, "-s", "../lib/hosttest_p384_tables16"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_p384_tables16")


def v_line(row, key_ok=True):
    return "V %x %x %x %x %x %d\n" % (row + (int(key_ok),))


def t_line(q, w, d):
    return "T %x %x %x %x\n" % (q[0], q[1], w, d)


def table_digits():
    rng = random.Random(384016)
    return (0,) + C.DIGITS16 + tuple(rng.randrange(1, 65536) for _ in range(64))


def table_keys():
    """the generator and two keys of the KATs"""
    kats = K.kat_rows()
    qs = []
    for t in kats:
        if (t[0], t[1]) not in qs:
            qs.append((t[0], t[1]))
    assert len(qs) >= 2
    return [R.G] + qs[:2]


def write_commands(path):
    """the command file `make sanitize-p384-tables16 P384_T16_CASES=path` reads: every line the tests below send"""
    with open(path, "w") as f:
        for q in table_keys():
            for w in WINDOWS:
                for d in table_digits():
                    f.write(t_line(q, w, d))
        for row in K.kat_rows() + list(K.mixed257()[0]) + list(K.exceptional()[0]) + [r for _n, _k, r in C.steering()]:
            f.write(v_line(row))


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert out.returncode in (0, 1), out.stdout + out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(lines), out.stderr
    return got


def test_builder_entries_against_python_integers(exe):
    lines, want = [], []
    for q in table_keys():
        for w in WINDOWS:
            base = R.mul(1 << (16 * w), q)
            for d in table_digits():
                lines.append(t_line(q, w, d))
                want.append(R.mul(d, base) if d else None)
    got = _run(exe, lines)
    for ln, g, pt in zip(lines, got, want):
        if pt is None:
            assert g == "0 0", ln                                 # entry 0 is all zero
        else:
            x, y = (int(v, 16) for v in g.split())
            assert (x, y) == pt, ln


def _both(exe, rows, want, key_ok=True):
    got = [tuple(int(v) for v in g.split()) for g in _run(exe, [v_line(r, key_ok) for r in rows])]
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if not g[0] == g[1] == w]
    assert not bad, bad[:8]


def test_the_24_window_core_on_the_kats(exe):
    rows = K.kat_rows()
    _both(exe, rows, K.want(rows))


def test_the_24_window_core_on_the_keyed_cases(exe):
    rows, want = K.mixed257()
    _both(exe, rows, want)
    rows, want = K.exceptional()
    _both(exe, rows, want)


def test_the_24_window_core_on_rows_steered_by_their_16_bit_digits(exe):
    cases, want = C.steering(), C.steering_expected()
    names = [n for n, _k, _r in cases]
    for w in WINDOWS:
        assert "doubling in window %d" % w in names and "infinity in window %d" % w in names
    for n in ("u1 has zero digits", "u2 has zero digits", "low bytes zero", "high bytes zero", "all-ones digits"):
        assert n in names
    # the digits are where the names say
    for (name, _key, row), st in zip(cases, want):
        ws = pow(row[4], -1, R.N)
        u1, u2 = row[2] * ws % R.N, row[3] * ws % R.N
        dig = lambda u: [(u >> (16 * w)) & 0xFFFF for w in range(24)]
        if name.startswith("doubling") or name.startswith("infinity"):
            assert u1 == u2 and sum(1 for d in dig(u1) if d) == 1
            assert st == (0 if name.startswith("doubling") else 1)
        if name == "u1 has zero digits":
            assert dig(u1).count(0) == 21
        if name == "u2 has zero digits":
            assert dig(u2).count(0) == 21
        if name == "low bytes zero":
            assert all(d & 0xFF == 0 for d in dig(u1) + dig(u2)) and all(d >> 8 for d in dig(u1))
        if name == "high bytes zero":
            assert all(d >> 8 == 0 and d for d in dig(u1) + dig(u2))
        if name == "all-ones digits":
            assert dig(u1)[:23] == dig(u2)[:23] == [0xFFFF] * 23
    _both(exe, [r for _n, _k, r in cases], want)
    # a row that names no live key runs the whole stream on the generator's comb and answers 4
    _both(exe, [r for _n, _k, r in cases], [4] * len(cases), key_ok=False)
