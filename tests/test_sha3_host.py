"""SHA3-256 as the device computes it (fabric-mod_amd/csrc/sha3_256.h), compiled for the host and run through libfabgpu_hosttest.so:
NIST known answers, every length over three rate blocks, the mid-state form on a grid of prefix and suffix lengths around the
136-byte rate, and the exported 200-byte mid-state against a plain Keccak absorb written here in Python integers."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RATE = 136
PREFIX_LENS = (0, 1, 135, 136, 137, 271, 272, 273, 300)
SUFFIX_LENS = (0, 1, 134, 135, 136, 137)


@pytest.fixture(scope="module")
def hosttest():
    lib = ctypes.CDLL(os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_hosttest.so"))
    lib.hosttest_sha3_256.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    lib.hosttest_sha3_256.restype = None
    lib.hosttest_sha3_256_prefixed.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    lib.hosttest_sha3_256_prefixed.restype = None
    lib.hosttest_sha3_256_midstate.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    lib.hosttest_sha3_256_midstate.restype = None
    lib.hosttest_sha3_256_at.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p]
    lib.hosttest_sha3_256_at.restype = None
    return lib


def _sha3(lib, msg: bytes) -> bytes:
    out = ctypes.create_string_buffer(32)
    lib.hosttest_sha3_256(msg, len(msg), out)
    return out.raw


def _sha3_prefixed(lib, prefix: bytes, msg: bytes) -> bytes:
    out = ctypes.create_string_buffer(32)
    lib.hosttest_sha3_256_prefixed(prefix, len(prefix), msg, len(msg), out)
    return out.raw


def _bytes(seed: int, n: int) -> bytes:
    return bytes(np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8))


def test_nist_known_answers(hosttest):
    assert _sha3(hosttest, b"").hex() == "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a"
    assert _sha3(hosttest, b"abc").hex() == "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532"


def test_every_length_over_three_rate_blocks(hosttest):
    data = _bytes(1, 410)
    bad = [n for n in range(411) if _sha3(hosttest, data[:n]) != hashlib.sha3_256(data[:n]).digest()]
    assert not bad, "lengths that disagree with hashlib.sha3_256: %s" % bad


def test_prefixed_form_on_the_rate_grid(hosttest):
    pre, suf = _bytes(2, max(PREFIX_LENS)), _bytes(3, max(SUFFIX_LENS))
    bad = [(p, s) for p in PREFIX_LENS for s in SUFFIX_LENS
           if _sha3_prefixed(hosttest, pre[:p], suf[:s]) != hashlib.sha3_256(pre[:p] + suf[:s]).digest()]
    assert not bad, "(prefix, suffix) lengths that disagree with hashlib.sha3_256 of the concatenation: %s" % bad


# ---- Keccak-f[1600] in Python integers (FIPS 202 section 3.2), for the exported mid-state ----
_RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
       0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
       0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
       0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
_M = (1 << 64) - 1


def _rol(v, n):
    n %= 64
    return ((v << n) | (v >> (64 - n))) & _M if n else v


def _keccak_f(a):
    """a[x][y], 24 rounds; the rotation offsets come from the (t + 1)(t + 2) / 2 walk of the specification, not from a table"""
    for rc in _RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[0] * 5 for _ in range(5)]
        b[0][0] = a[0][0]
        x, y = 1, 0
        for t in range(24):
            b[y][(2 * x + 3 * y) % 5] = _rol(a[x][y], (t + 1) * (t + 2) // 2)
            x, y = y, (2 * x + 3 * y) % 5
        a = [[b[x][y] ^ (~b[(x + 1) % 5][y] & _M & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        a[0][0] ^= rc
    return a


def _plain_absorb(data: bytes) -> bytes:
    """the 200-byte state after absorbing whole rate blocks, no padding"""
    assert len(data) % RATE == 0
    a = [[0] * 5 for _ in range(5)]
    for o in range(0, len(data), RATE):
        for i in range(RATE // 8):
            a[i % 5][i // 5] ^= int.from_bytes(data[o + 8 * i:o + 8 * i + 8], "little")
        a = _keccak_f(a)
    return b"".join(a[i % 5][i // 5].to_bytes(8, "little") for i in range(25))


def test_python_keccak_is_sha3(hosttest):
    """the yardstick of the mid-state test: padded by hand, it gives hashlib's digest"""
    m = _bytes(4, 200)
    padded = bytearray(m + b"\x06" + bytes(2 * RATE - 201))
    padded[-1] |= 0x80
    assert _plain_absorb(bytes(padded))[:32] == hashlib.sha3_256(m).digest()


@pytest.mark.parametrize("plen", (272, 273, 300, 135))
def test_exported_midstate_is_the_plain_absorb_of_the_whole_blocks(hosttest, plen):
    prefix = _bytes(5, plen)
    out = ctypes.create_string_buffer(200)
    hosttest.hosttest_sha3_256_midstate(prefix, plen, out)
    assert out.raw == _plain_absorb(prefix[:plen // RATE * RATE])


# ---- arena offsets up to 2^32 - 1: the stream code over an arena of 2^32 - 4 bytes that exists only as a function of the position ----
ARENA_BYTES = (1 << 32) - 4
HIGH_STARTS = (0, (1 << 31) - 300, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 31) + 2, (1 << 31) + 3, 3 * (1 << 30) + 1, ARENA_BYTES - 500)
HIGH_LENS = (0, 1, 135, 136, 137, 300, 409)
HIGH_PREFIX_LENS = (135, 136, 272)


def _arena_bytes(start: int, n: int) -> bytes:
    """hosttest.cpp Sha3SyntheticArena::byte_at: the top byte of position * 0x9E3779B97F4A7C15 mod 2^64"""
    p = np.arange(start, start + n, dtype=np.uint64)
    return ((p * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(56)).astype(np.uint8).tobytes()


def _sha3_at(lib, start, n, pre_start=0, pre_len=0) -> bytes:
    out = ctypes.create_string_buffer(32)
    lib.hosttest_sha3_256_at(start, n, pre_start, pre_len, out)
    return out.raw


def test_offsets_on_both_sides_of_2_to_the_31_and_at_the_arenas_end(hosttest):
    """A byte offset is a u32 and goes up to the arena's size, 2^32 - 1 at the most: messages that start below, at, above and across
    2^31, at every byte phase, and in the arena's last bytes (one ending on its last byte: the 35th dword of the last block is the
    clamped one); then each behind a prefix that lies on the other side of 2^31, and behind one that crosses it."""
    starts = HIGH_STARTS + tuple(ARENA_BYTES - n for n in HIGH_LENS if n)      # ... and ending on the arena's last byte
    bad = []
    for start in starts:
        for n in HIGH_LENS:
            if start + n > ARENA_BYTES:
                continue
            msg = _arena_bytes(start, n)
            if _sha3_at(hosttest, start, n) != hashlib.sha3_256(msg).digest():
                bad.append((start, n))
            other_side = (1 << 31) + 4097 if start < (1 << 31) else 4099         # byte phases 1 and 3
            for ps in (other_side, (1 << 31) - 101):
                for pl in HIGH_PREFIX_LENS:
                    if _sha3_at(hosttest, start, n, ps, pl) != hashlib.sha3_256(_arena_bytes(ps, pl) + msg).digest():
                        bad.append((start, n, ps, pl))
    assert not bad, "(start, length[, prefix start, prefix length]) that disagree with hashlib.sha3_256: %s" % [tuple(hex(x) for x in b) for b in bad]
