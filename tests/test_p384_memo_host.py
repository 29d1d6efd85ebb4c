"""P384Memo (csrc/p384_memo.h), the verdict memo of the P-384 tuples of a block pass, on the CPU: the table is a pure function of bytes
and is driven here through the stand-alone program csrc/hosttest_p384_memo.cpp - this file writes scripts of table commands, the
program answers one line per command, every answer is checked (the sanitizer build of the same program is `make sanitize-p384-memo`)."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_p384_memo")


def _hex(b: bytes) -> str:
    return b.hex() if b else "-"


class Script:
    """commands for the program, and the answer each must get"""

    def __init__(self):
        self.lines, self.want = [], []

    def do(self, cmd: str, want: str):
        self.lines.append(cmd)
        self.want.append(want)

    def record(self, seq, entries, published=True):
        self.do("begin %d %d" % (seq, len(entries)), "ok")
        for qx, qy, sig, dg, st in entries:
            self.do("add %s %s %s %s %d" % (_hex(qx), _hex(qy), _hex(sig), _hex(dg), st), "ok")
        self.do("publish", "published %d" % len(entries) if published else "refused")

    def hit(self, e, status, seq):
        self.do("lookup %s %s %s %s" % tuple(_hex(x) for x in e[:4]), "hit %d %d" % (status, seq))

    def miss(self, qx, qy, sig, dg):
        self.do("lookup %s %s %s %s" % (_hex(qx), _hex(qy), _hex(sig), _hex(dg)), "miss")

    def run(self, tmp_path):
        f = tmp_path / "memo_script.txt"
        f.write_text("\n".join(self.lines) + "\n")
        out = subprocess.run([EXE, str(f)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        got = out.stdout.splitlines()
        assert len(got) == len(self.want)
        wrong = [(i, self.lines[i][:60], g, w) for i, (g, w) in enumerate(zip(got, self.want)) if g != w]
        assert not wrong, wrong[:5]


def _entries(rnd, n, sig_len=lambda i: 8 + i % 97, dig_len=lambda i: 48 if i & 1 else 32, status=lambda i: i % 4):
    return [(rnd.randbytes(48), rnd.randbytes(48), rnd.randbytes(sig_len(i)), rnd.randbytes(dig_len(i)), status(i)) for i in range(n)]


def _flip(rnd, b: bytes) -> bytes:
    bit = rnd.randrange(8 * len(b))
    return b[:bit >> 3] + bytes([b[bit >> 3] ^ (1 << (bit & 7))]) + b[(bit >> 3) + 1:]


@pytest.fixture(scope="module")
def seeded():
    """257 entries: signatures of 8 .. 104 bytes (every length of P-384's DER range), digests of 32 and 48 bytes, statuses 0 .. 3"""
    rnd = random.Random(384257)
    es = _entries(rnd, 257)
    assert {len(e[2]) for e in es} == set(range(8, 105)) and {len(e[3]) for e in es} == {32, 48}
    return es


def test_every_entry_hits_with_its_own_status(seeded, tmp_path):
    s = Script()
    s.record(41, seeded)
    for e in seeded:
        s.hit(e, e[4], 41)
    s.do("has 41", "has 257")
    s.do("stats", "stats 257 257 0 0")
    s.run(tmp_path)


def test_near_misses_all_miss(seeded, tmp_path):
    rnd = random.Random(1)
    s = Script()
    s.record(41, seeded)
    for qx, qy, sig, dg, _ in seeded:
        s.miss(_flip(rnd, qx), qy, sig, dg)
        s.miss(qx, _flip(rnd, qy), sig, dg)
        s.miss(qx, qy, _flip(rnd, sig), dg)
        s.miss(qx, qy, sig, _flip(rnd, dg))
        s.miss(qx, qy, sig[:-1], dg)                         # siglen - 1
        s.miss(qx, qy, sig + b"\0", dg)                      # siglen + 1
    s.miss(seeded[0][0], seeded[0][1], b"", seeded[0][3])    # parts a lookup does not take: empty, longer than 1024 bytes
    s.miss(seeded[0][0], seeded[0][1], seeded[0][2], b"")
    s.miss(seeded[0][0], seeded[0][1], b"\1" * 1025, seeded[0][3])
    s.do("stats", "stats 257 0 %d 0" % (6 * 257))            # (those three are refused before the table is asked)
    s.run(tmp_path)


def test_the_lengths_frame_signature_and_digest(tmp_path):
    """two entries whose sig || digest concatenations are equal but split differently do not alias"""
    rnd = random.Random(2)
    qx, qy, both = rnd.randbytes(48), rnd.randbytes(48), rnd.randbytes(72)
    a = (qx, qy, both[:40], both[40:], 0)
    b = (qx, qy, both[:24], both[24:], 1)
    s = Script()
    s.record(1, [a])
    s.hit(a, 0, 1)
    s.miss(*b[:4])
    s.record(2, [b])
    s.hit(a, 0, 1)
    s.hit(b, 1, 2)
    s.run(tmp_path)
    s = Script()                                             # ... nor inside one record
    s.record(3, [a, b])
    s.hit(b, 1, 3)
    s.hit(a, 0, 3)
    s.run(tmp_path)


def test_a_key_seeded_twice_answers_with_the_first(tmp_path):
    rnd = random.Random(3)
    e = _entries(rnd, 1)[0]
    s = Script()
    s.record(5, [e[:4] + (1,), e[:4] + (0,)] + _entries(rnd, 30))
    s.hit(e, 1, 5)
    s.do("has 5", "has 32")                                  # (both are held, as the P-256 host seeding holds both)
    s.run(tmp_path)


def test_capacity_drops_the_oldest_blocks_whole(tmp_path):
    rnd = random.Random(4)
    blocks = [_entries(rnd, 100) for _ in range(4)]
    s = Script()
    s.do("cap 250", "ok")
    for b, es in enumerate(blocks):
        s.record(10 + b, es)
    s.do("stats", "stats 200 0 0 200")
    for b, es in enumerate(blocks):
        s.do("has %d" % (10 + b), "has %d" % (0 if b < 2 else 100))
        for e in es:
            if b < 2:
                s.miss(*e[:4])
            else:
                s.hit(e, e[4], 10 + b)
    s.do("stats", "stats 200 200 200 200")
    s.run(tmp_path)


def test_eviction(tmp_path):
    rnd = random.Random(5)
    a, b = _entries(rnd, 20), _entries(rnd, 30)
    s = Script()
    s.do("evict 7", "evicted 0")                             # nothing is held at all
    s.record(7, a)
    s.record(8, b)
    s.do("evict 9", "evicted 0")                             # a block that is not held
    s.do("evict 7", "evicted 20")
    s.do("evict 7", "evicted 0")
    for e in a:
        s.miss(*e[:4])
    for e in b:
        s.hit(e, e[4], 8)
    s.do("stats", "stats 30 30 20 20")
    s.do("begin 9 0", "ok")
    s.do("publish", "refused")                               # an empty record is not published
    s.do("has 9", "has 0")
    s.run(tmp_path)


def test_the_programs_own_cases():
    """the cases the sanitizer build runs by default, threads beside a writer among them"""
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout + out.stderr
