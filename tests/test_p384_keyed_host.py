"""Registered P-384 keys on the host compilation: the comb-table builder and the keyed verification core of csrc/p384_tables.h, the book
of keys of csrc/p384_keys.h, and the stand-alone program csrc/hosttest_p384_keyed.cpp - all against Python integers (p384_ref.py,
p384_keyed_cases.py).  No device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fabgpu
import p384_keyed_cases as C
import p384_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = R.N


@pytest.fixture(scope="module")
def gcomb():
    return fabgpu.p384_comb_host()


@pytest.fixture(scope="module")
def combs(gcomb):
    """host-built tables by key, made on demand and kept"""
    cache = {R.G: gcomb}

    def get(q):
        if q not in cache:
            cache[q] = fabgpu.p384_comb_host(R.b48(q[0]), R.b48(q[1]))
        return cache[q]
    return get


def _check_table(table, q):
    wantw = np.array(C.comb_words(q), dtype=np.uint32)
    assert table.size == wantw.size == 48 * 256 * 24 == fabgpu.P384_COMB_WORDS
    bad = np.nonzero(table != wantw)[0]
    assert bad.size == 0, "first differing word %d (window %d, digit %d)" % (bad[0], bad[0] // (256 * 24), bad[0] // 24 % 256)
    ent = table.reshape(48, 256, 24)
    assert not ent[:, 0, :].any()                                # the 48 zero entries
    assert ent[:, 1:, :].reshape(-1, 24).any(axis=1).all()       # ... and 12 240 points


def test_builder_for_a_key_equals_python_integers(combs):
    _check_table(combs(C.keys()[0][1]), C.keys()[0][1])


def test_builder_for_the_generator_equals_python_integers(gcomb):
    _check_table(gcomb, R.G)


def test_builder_refuses_a_point_off_the_curve():
    q = C.keys()[1][1]
    with pytest.raises(fabgpu.FabgpuError):
        fabgpu.p384_comb_host(R.b48(q[0]), R.b48((q[1] + 1) % R.P))
    with pytest.raises(fabgpu.FabgpuError):
        fabgpu.p384_comb_host(R.b48(R.P), R.b48(q[1]))


def _keyed(gcomb, combs, rows):
    return [fabgpu.p384_verify_keyed_host(gcomb, combs((t[0], t[1])), R.b48(t[2]), R.b48(t[3]), R.b48(t[4])) for t in rows]


def test_keyed_core_on_every_kat(gcomb, combs):
    rows = C.kat_rows()
    assert len(rows) >= 48
    want = C.want(rows)
    assert 0 in want and 2 in want                                # (as produced: some s are high)
    assert _keyed(gcomb, combs, rows) == want


def test_keyed_core_on_the_257_row_mix(gcomb, combs):
    rows, want = C.mixed257()
    assert _keyed(gcomb, combs, rows) == list(want)


def test_keyed_core_on_the_exceptional_rows(gcomb, combs):
    rows, want = C.exceptional()
    assert _keyed(gcomb, combs, rows) == list(want)


def test_keyed_core_answers_4_for_a_row_without_a_key_unless_the_gate_refuses_it(gcomb):
    """key_ok = false (the kernel's row whose id names no live key: the generator's table stands in): 4, behind the gate's 2 and 3"""
    rows, want = C.mixed257()
    for t, w in list(zip(rows, want))[:45]:
        st = fabgpu.p384_verify_keyed_host(gcomb, gcomb, R.b48(t[2]), R.b48(t[3]), R.b48(t[4]), key_ok=False)
        assert st == (w if w in (2, 3) else 4)


def test_the_book_of_p384_keys_follows_the_id_rules():
    """register, retire, re-register: the next generation on the same slot; the snapshot a launch is handed shows a retired slot empty"""
    H = fabgpu.load_hooks()
    b = H.fabgpu_test_p384_book_new(0xFFFFF)
    try:
        name = lambda i: bytes([i]) * 96
        ids = [H.fabgpu_test_p384_book_register(b, name(i), 1000 + i) for i in range(3)]
        assert ids == [0, 1, 2]
        assert H.fabgpu_test_p384_book_register(b, name(1), 7777) == 1          # twice: the first id, the first table
        tags, gens = (ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 8)()
        assert H.fabgpu_test_p384_book_snapshot(b, tags, gens, 8) == 3
        assert list(tags)[:3] == [1000, 1001, 1002] and list(gens)[:3] == [0, 0, 0]
        tag = ctypes.c_uint64(0)
        assert H.fabgpu_test_p384_book_retire(b, 1, ctypes.byref(tag)) == 0 and tag.value == 1001
        assert H.fabgpu_test_p384_book_retire(b, 1, ctypes.byref(tag)) == 1      # idempotent
        assert H.fabgpu_test_p384_book_lookup(b, name(1)) == -1 and H.fabgpu_test_p384_book_lookup(b, name(2)) == 2
        assert H.fabgpu_test_p384_book_snapshot(b, tags, gens, 8) == 3           # the high-water mark stays
        assert list(tags)[:3] == [1000, 0, 1002] and list(gens)[:3] == [0, 0xFFFFFFFF, 0]
        nid = H.fabgpu_test_p384_book_register(b, name(9), 2009)                 # another key: the lowest reclaimable slot, next generation
        assert nid == (1 << 12 | 1)
        assert H.fabgpu_test_p384_book_register(b, name(1), 2001) == 3           # the retired key again: a new slot, generation 0
        assert H.fabgpu_test_p384_book_snapshot(b, tags, gens, 8) == 4
        assert list(tags)[:4] == [1000, 2009, 1002, 2001] and list(gens)[:4] == [0, 1, 0, 0]
        assert H.fabgpu_test_p384_book_retire(b, 1, ctypes.byref(tag)) == 1      # the stale id names nobody
        assert H.fabgpu_test_p384_book_retire(b, nid, ctypes.byref(tag)) == 0 and tag.value == 2009
    finally:
        H.fabgpu_test_p384_book_free(b)
    b = H.fabgpu_test_p384_book_new(1)                                           # two generations per slot: then the slot is parked
    try:
        tag = ctypes.c_uint64(0)
        assert H.fabgpu_test_p384_book_register(b, b"a" * 96, 1) == 0
        assert H.fabgpu_test_p384_book_retire(b, 0, ctypes.byref(tag)) == 0
        assert H.fabgpu_test_p384_book_register(b, b"b" * 96, 2) == 1 << 12
        assert H.fabgpu_test_p384_book_retire(b, 1 << 12, ctypes.byref(tag)) == 0
        assert H.fabgpu_test_p384_book_register(b, b"c" * 96, 3) == 1            # slot 0 is used up
    finally:
        H.fabgpu_test_p384_book_free(b)


def test_standalone_keyed_program_over_the_fixtures(tmp_path):
    """csrc/hosttest_p384_keyed.cpp (its own main, built by the Makefile): the builder's invariants and the keyed core over the KATs and
    the exceptional rows; `make sanitize-p384-keyed P384_VECTORS=...` runs the same program under -fsanitize=address,undefined."""
    exe = os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_p384_keyed")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    rows = C.kat_rows() + list(C.exceptional()[0])
    want = C.want(C.kat_rows()) + list(C.exceptional()[1])
    q = C.keys()[2][1]
    rows.append((q[0], (q[1] + 1) % R.P, 5, 6, 7)); want.append(4)           # a key off the curve: no table, status 4
    vec = tmp_path / "p384_keyed_vectors.txt"
    vec.write_text("".join("%x %x %x %x %x %d\n" % (t + (w,)) for t, w in zip(rows, want)))
    out = subprocess.run([exe, str(vec)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "%d tuples, 0 failures" % len(rows) in out.stdout
