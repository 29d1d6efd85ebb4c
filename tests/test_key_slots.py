"""The allocator of key slots and key ids (fabric-mod_amd/csrc/key_slots.h) by itself, through libfabgpu_testhooks.so: no device.

A key id is generation << 12 | slot.  What the contexts of one provider rely on: the ids follow from the SEQUENCE of register / retire
calls alone - never from when a device happened to finish draining a retired slot."""
import ctypes

import numpy as np
import pytest

import fabgpu

SLOT_BITS = 12
MAX_KEYS = 1 << SLOT_BITS
GEN_LAST = (1 << 20) - 1


class Slots:
    def __init__(self, gen_last=GEN_LAST):
        self.H = fabgpu.load_hooks()
        self.h = ctypes.c_void_p(self.H.fabgpu_test_key_slots_new(gen_last))

    def register(self):
        return int(self.H.fabgpu_test_key_slots_register(self.h))

    def retire(self, key_id):
        return int(self.H.fabgpu_test_key_slots_retire(self.h, key_id))

    def drain(self, slot):
        return int(self.H.fabgpu_test_key_slots_drain(self.h, slot))

    def stats(self):
        v = (ctypes.c_uint64 * 6)()
        self.H.fabgpu_test_key_slots_stats(self.h, v)
        return dict(zip(("live", "draining", "reused", "parked", "slots_used", "waits"), (int(x) for x in v)))

    def close(self):
        self.H.fabgpu_test_key_slots_free(self.h)


@pytest.fixture()
def slots():
    made = []

    def make(*a):
        made.append(Slots(*a))
        return made[-1]
    yield make
    for s in made:
        s.close()


def test_header_constants_are_the_tests():
    assert fabgpu.load() is not None
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fabgpu.h")).read()
    assert int(re.search(r"#define FABGPU_MAX_KEYS (\d+)", hdr).group(1)) == MAX_KEYS


def test_ids_without_retirement_are_the_registration_order(slots):
    s = slots()
    n = 300
    assert [s.register() for _ in range(n)] == list(range(n))
    assert s.stats() == dict(live=n, draining=0, reused=0, parked=0, slots_used=n, waits=0)


def test_lowest_slot_is_reused_first_with_the_next_generation(slots):
    s = slots()
    assert [s.register() for _ in range(6)] == list(range(6))
    assert s.retire(4) == 0 and s.retire(1) == 0
    assert s.retire(1) == 1 and s.retire(77) == 1                          # idempotent; never handed out
    assert s.drain(4) == 1                                                 # slot 4 has drained, slot 1 has not: slot 1 goes first all the same
    assert s.register() == (1 << SLOT_BITS | 1)
    assert s.stats()["waits"] == 1
    assert s.register() == (1 << SLOT_BITS | 4)
    assert s.register() == 6                                               # nothing to reclaim: a slot that never had a tenant
    assert s.retire(1) == 1                                                # the first tenant's id stays dead
    assert s.retire(1 << SLOT_BITS | 1) == 0
    assert s.register() == (2 << SLOT_BITS | 1)
    st = s.stats()
    assert (st["live"], st["draining"], st["reused"], st["parked"], st["slots_used"]) == (7, 0, 3, 0, 7)


def test_same_sequence_other_drain_timing_same_ids(slots):
    """10^5 seeded register / retire steps into two allocators: one whose slots drain at once, one whose slots drain late and in another
    order (so its registrations keep finding their slot still draining).  Every id is the same."""
    a, b = slots(), slots()
    rng = np.random.default_rng(20240607)
    live, late = [], []
    steps = 100_000
    ops = rng.random(steps)
    picks = rng.integers(0, 1 << 30, size=steps)
    for t in range(steps):
        if live and (ops[t] < 0.48 or len(live) >= 600):
            kid = live.pop(int(picks[t]) % len(live))
            assert a.retire(kid) == 0 and b.retire(kid) == 0
            assert a.drain(kid & (MAX_KEYS - 1)) == 1                      # a: drained the moment it retires
            late.append(kid & (MAX_KEYS - 1))
            if len(late) > 40:                                             # b: some time later, newest first
                for sl in reversed(late[:20]):
                    b.drain(sl)
                del late[:20]
        else:
            ia, ib = a.register(), b.register()
            assert ia == ib and ia >= 0, (t, ia, ib)
            live.append(ia)
    sa, sb = a.stats(), b.stats()
    assert sa["waits"] == 0 and sb["waits"] > 1000                          # the timings did differ
    for k in ("live", "reused", "parked", "slots_used"):
        assert sa[k] == sb[k], k
    assert sa["reused"] > 10_000 and len(set(live)) == len(live) == sa["live"]


def test_a_slot_at_its_last_generation_parks(slots):
    s = slots(2)                                                           # generations 0, 1, 2
    assert [s.register() for _ in range(3)] == [0, 1, 2]
    for gen in range(2):
        assert s.retire(gen << SLOT_BITS | 1) == 0
        assert s.register() == ((gen + 1) << SLOT_BITS | 1)
    assert s.retire(2 << SLOT_BITS | 1) == 0                               # the last generation: parked, not draining
    st = s.stats()
    assert (st["parked"], st["draining"], st["live"]) == (1, 0, 2)
    assert s.drain(1) == 0
    got = [s.register() for _ in range(5)]
    assert got == [3, 4, 5, 6, 7] and all((g & (MAX_KEYS - 1)) != 1 for g in got)
    assert s.retire(0) == 0
    assert s.register() == (1 << SLOT_BITS | 0)                            # other slots go on as before


def test_the_cap_is_on_live_keys_not_on_registrations(slots):
    s = slots()
    ids = [s.register() for _ in range(MAX_KEYS)]
    assert ids == list(range(MAX_KEYS))
    assert s.register() == -1 and s.stats()["live"] == MAX_KEYS
    rng = np.random.default_rng(5)
    for step in range(3 * MAX_KEYS):                                       # 3 x 4096 retire + register steps at the cap
        j = int(rng.integers(0, MAX_KEYS))
        assert s.retire(ids[j]) == 0
        new = s.register()
        assert new >= 0 and (new & (MAX_KEYS - 1)) == (ids[j] & (MAX_KEYS - 1)) and new >> SLOT_BITS == (ids[j] >> SLOT_BITS) + 1
        ids[j] = new
        if step % 512 == 0:
            assert s.register() == -1
    st = s.stats()
    assert st["live"] == MAX_KEYS and st["reused"] == 3 * MAX_KEYS and st["slots_used"] == MAX_KEYS and s.register() == -1
