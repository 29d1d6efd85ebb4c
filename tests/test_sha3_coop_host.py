"""The 32-lanes-per-message SHA3-256 of csrc/sha3_coop.h as the host compiles it - the very body of the kernels of sha3_coop_kernels.hip,
with a 32-entry array where they have a half-wavefront - against hashlib.sha3_256, through the stand-alone program
csrc/hosttest_sha3_coop.cpp (cases on stdin, two digests per case: the array model's and the one-lane host code's; the sanitizer build of
the same program is `make sanitize-sha3-coop`).

The grid is the one tests/test_sha3_coop_gpu.py runs on the device: every length around the 136-byte block boundaries at the four byte
phases of its start, prefixes that put the seam between prefix and message at every position of a block, and a message that ends on the
buffer's last byte at every buffer size mod 4."""
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fabric-mod_amd", "csrc")
EXE = os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_sha3_coop")

LENGTHS = [0, 1, 7, 8, 9] + list(range(134, 139)) + list(range(270, 275)) + list(range(406, 411)) + [14 * 136 - 1, 14 * 136, 14 * 136 + 1]
PREFIX_LENS = (0, 1, 135, 136, 137, 300)
_BYTES = np.random.default_rng(1600).integers(0, 256, size=6000, dtype=np.uint8).tobytes()


def cases():
    """[(buffer, sa, la, sb, lb)]: the message is buffer[sa, sa + la) || buffer[sb, sb + lb)"""
    out = []
    for ln in LENGTHS:
        for phase in range(4):
            out.append((_BYTES, 0, 0, 16 + phase, ln))
    for pl in PREFIX_LENS:
        for ln in LENGTHS:
            phase = (pl + ln) % 4
            out.append((_BYTES, 3000 + (phase ^ 3), pl, 21 + phase, ln))
            out.append((_BYTES, 40 + phase, pl, 3000 + (phase ^ 1), ln))        # (the prefix in front of the message's own bytes, and behind them)
    for cut in range(4):                                                      # the message ends on the buffer's last byte
        buf = _BYTES[:900 + cut]
        out.append((buf, 0, 0, 500, len(buf) - 500))
        out.append((buf, 1, 137, 501, len(buf) - 501))
        out.append((buf, len(buf) - 137, 137, 2, 9))                          # ... and so does the prefix
    out.append((b"", 0, 0, 0, 0))
    return out


def run(cs):
    subprocess.run(["make", "-s", "-C", CSRC, "../lib/hosttest_sha3_coop"], check=True, timeout=600)
    text = "".join("%s %d %d %d %d\n" % (buf.hex() or "-", sa, la, sb, lb) for buf, sa, la, sb, lb in cs)
    out = subprocess.run([EXE], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode in (0, 1), out.stderr
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(cs), out.stderr
    return [ln.split() for ln in lines]


def test_array_model_against_hashlib_over_the_grid():
    cs = cases()
    assert len(cs) == len(LENGTHS) * (4 + 2 * len(PREFIX_LENS)) + 13
    got = run(cs)
    bad = []
    for (buf, sa, la, sb, lb), cols in zip(cs, got):
        want = hashlib.sha3_256(buf[sa:sa + la] + buf[sb:sb + lb]).hexdigest()
        if cols[0] != want or cols[1] != want or len(cols) != 2:
            bad.append((len(buf), sa, la, sb, lb, cols))
    assert not bad, "(buffer size, sa, la, sb, lb) whose digests are not hashlib.sha3_256's: %s" % bad[:6]


def test_the_programs_own_grid():
    subprocess.run(["make", "-s", "-C", CSRC, "../lib/hosttest_sha3_coop"], check=True, timeout=600)
    out = subprocess.run([EXE, "self"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and " 0 disagreements" in out.stderr, out.stdout[-2000:] + out.stderr

