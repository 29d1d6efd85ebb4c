"""The layout of the block pass's four buffers (fabric-mod_amd/csrc/walk_layout.h), on the CPU through libfabgpu_hosttest.so:
the header lays every region out where walk_block_pass carved it by hand before (tests/golden/walk_layout_parent.json, recorded from
that version's own lines), every layout is well-formed, and no pass within the stated bounds needs more than walk_worst_case - what
walk_preallocate makes, never less than the estimates it made before."""
import ctypes
import json
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_LAUNCH_MAX = 8192          # kernels.h
MSPS_MAX = 16                   # block_walk_dev.h WALK_IDEMIX_MSPS_MAX
ENV, TUP, PIN, MAP = 0, 1, 2, 3
N_REGIONS = {ENV: 17, TUP: 48, PIN: 9, MAP: 7}
ALIGN = {ENV: 256, TUP: 256, PIN: 64, MAP: 64}
# names of the tuple buffer's regions the tests speak of, by position
T_NYMF, T_NYMI, T_NYMSP, T_NYMIO = 26, 27, 28, 29


@pytest.fixture(scope="module")
def hosttest():
    p = os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_hosttest.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(p)
    lib.hosttest_walk_layout.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    lib.hosttest_walk_layout.restype = ctypes.c_int
    lib.hosttest_walk_worst_case.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    lib.hosttest_walk_worst_case.restype = None
    return lib


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "walk_layout_parent.json")))


def layout(lib, shape, which):
    """-> (offsets, sizes, scalars) of one buffer's layout for a 16-word shape"""
    buf = (ctypes.c_uint64 * 128)()
    n = lib.hosttest_walk_layout((ctypes.c_uint32 * 16)(*shape), which, buf, 128)
    k = N_REGIONS[which]
    assert n > 2 * k
    v = list(buf[:n])
    return v[0:2 * k:2], v[1:2 * k:2], v[2 * k:]


def worst_case(lib, n_tx, n_tuples):
    """-> (walk_worst_case, the floor kept from before, what walk_preallocate makes), four totals each"""
    buf = (ctypes.c_uint64 * 12)()
    lib.hosttest_walk_worst_case(n_tx, n_tuples, buf)
    v = list(buf)
    return v[0:4], v[4:8], v[8:12]


def slot_cap(nt):
    """the slot table the provider gives a pass of nt tuples (GPUCSP::MemoPinLayout)"""
    c = 16
    while c < 2 * nt:
        c <<= 1
    return c


def random_shape(rng, n_tx, n_tuples):
    """a pass of at most n_tx envelopes and n_tuples tuples, within the bounds walk_worst_case states"""
    edge = rng.random() < 0.25
    ne = n_tx if edge else rng.randint(1, n_tx)
    nt = rng.choice([n_tuples, min(n_tuples, WIDE_LAUNCH_MAX), min(n_tuples, WIDE_LAUNCH_MAX + 1)]) if edge else rng.randint(1, n_tuples)
    creators = min(ne, nt) if edge else rng.randint(0, min(ne, nt))
    np_ = nt if edge else rng.randint(0, nt)
    nc = creators + np_ if edge else rng.randint(0, creators + np_)
    memo = rng.random() < 0.7
    keys = rng.choice([1, nt * 205 + creators * 32 + 256, nt * 1165 + 256]) if memo else 0
    return [ne, rng.choice([0, 1, MSPS_MAX]), rng.randint(0, 1), rng.randint(0, 1), rng.randint(0, 1), nt, np_, nc, creators, rng.randint(0, 1),
            int(memo), rng.randint(0, 1), slot_cap(nt) if memo else 0, keys, nt if edge else rng.randint(0, nt), rng.randint(0, 1)]


def test_the_recorded_shapes_switch_every_conditional_region(golden):
    f = golden["shape_fields"]
    col = lambda name: {c["shape"][f.index(name)] for c in golden["cases"]}   # noqa: E731
    assert {1, 65536} <= col("ne") | col("nt") and 1 in col("ne") and 1 in col("nt")
    assert 0 in col("np") and 0 in col("nc") and 0 in col("creators")
    assert {0, 1, MSPS_MAX} <= col("n_msps")
    for flag in ("early_hash", "host_counted", "has_issuer_hashes", "tuple_qxy", "memo", "hmemo", "nym_issuer"):
        assert col(flag) == {0, 1}, flag
    assert any(c["shape"][f.index("memo")] and c["shape"][f.index("hmemo")] for c in golden["cases"])
    assert {WIDE_LAUNCH_MAX, WIDE_LAUNCH_MAX + 1, 63, 65, 255, 257, 65536} <= col("nt")


def test_layout_equals_the_hand_carved_layout_it_replaces(hosttest, golden):
    assert len(golden["cases"]) >= 40
    for c in golden["cases"]:
        s = c["shape"]
        off, size, sc = layout(hosttest, s, ENV)
        assert off == c["env"] and sc == c["env_scalars"], s
        off, size, sc = layout(hosttest, s, TUP)
        dev_keys_cap, nym_memset, total = c["tup_scalars"]
        assert off == c["tup"] and sc[0] == dev_keys_cap and sc[5] == total, s
        assert sc[1] == off[T_NYMF] and sc[2] == nym_memset, s         # the one fill over the nym rows: same start, same length
        off, size, sc = layout(hosttest, s, PIN)
        assert off == c["pin"] and sc == c["pin_scalars"], s
        off, size, sc = layout(hosttest, s, MAP)
        assert off == c["map"] and sc == c["map_scalars"], s


def _check_well_formed(lib, s):
    totals = []
    for which in (ENV, TUP, PIN, MAP):
        off, size, sc = layout(lib, s, which)
        total, a = sc[-1], ALIGN[which]
        for i in range(len(off)):
            assert off[i] % a == 0, (s, which, i)
            assert off[i] + size[i] <= total, (s, which, i)
            nxt = off[i + 1] if i + 1 < len(off) else total
            assert off[i] + size[i] <= nxt, (s, which, i)               # in carving order, so: pairwise disjoint
            if size[i] == 0:
                assert nxt == off[i], (s, which, i)                     # an empty region takes no room
            else:
                assert nxt - (off[i] + size[i]) < a, (s, which, i)      # ... and nobody leaves more than the rounding
        if which == TUP:
            r = lambda v: (v + 255) // 256 * 256                        # noqa: E731
            assert sc[4] == 1, s
            assert off[T_NYMI] == r(off[T_NYMF] + size[T_NYMF]) and off[T_NYMSP] == r(off[T_NYMI] + size[T_NYMI]), s
            assert off[T_NYMIO] == r(off[T_NYMSP] + size[T_NYMSP]) == sc[1] + sc[2] and sc[1] == off[T_NYMF], s
            assert sc[3] == 32 * s[8] and size[T_NYMF] == (6 * sc[3] if s[1] else 0), s   # six columns of 32 bytes by creator rank
        if which == PIN:
            env_off, env_size, env_sc = layout(lib, s, ENV)
            assert sc[0] % 256 == 0 and env_sc[1] <= sc[0] == off[0], s  # behind the mirror of what goes up
        if which == MAP:
            assert sc[:6] == [0, 64, 128, 192, 256, 320] and off[0] == 320, s
        totals.append(total)
    return totals


def test_every_layout_is_well_formed(hosttest, golden):
    for c in golden["cases"]:
        _check_well_formed(hosttest, c["shape"])
    rng = random.Random(20241)
    for _ in range(3000):
        n_tuples = rng.choice([rng.randint(1, 300), rng.randint(1, 20000), rng.randint(1, 70000)])
        _check_well_formed(hosttest, random_shape(rng, max(1, rng.randint(1, n_tuples + 10)), n_tuples))


def test_no_pass_within_the_bounds_needs_more_than_the_preallocation(hosttest):
    rng = random.Random(77)
    sizes = [(max(1024, 65536 // 3), 65536), (1024, 512), (1, 1), (1024, WIDE_LAUNCH_MAX), (1024, WIDE_LAUNCH_MAX + 1), (70000, 100)]
    sizes += [(max(1024, nt // 3), nt) for nt in (rng.randint(1, 200000) for _ in range(40))]
    sizes += [(rng.randint(1, 70000), rng.randint(1, 200000)) for _ in range(60)]
    above_floor = []
    for n_tx, n_tuples in sizes:
        worst, floor, made = worst_case(hosttest, n_tx, n_tuples)
        assert all(m >= w and m >= f for m, w, f in zip(made, worst, floor)), (n_tx, n_tuples)
        assert all(m == max(w, f) for m, w, f in zip(made, worst, floor)), (n_tx, n_tuples)
        if any(w > f for w, f in zip(worst, floor)):
            above_floor.append((n_tx, n_tuples, worst, floor))
        for _ in range(40):
            s = random_shape(rng, n_tx, n_tuples)
            env = layout(hosttest, s, ENV)[2][-1]
            tup = layout(hosttest, s, TUP)[2][-1]
            pin = layout(hosttest, s, PIN)[2][-1]
            mp = layout(hosttest, s, MAP)[2]
            assert env <= worst[0] and tup <= worst[1] and pin <= worst[2] and max(mp[-1], mp[-2]) <= worst[3], (n_tx, n_tuples, s)
    print("worst case above the earlier estimate:", above_floor)
