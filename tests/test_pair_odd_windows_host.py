"""The all-odd signed 4-bit recoding of u2 (csrc/p256_odd4.h: u2_fold_odd, odd_digit4 and the top-down walk the device loop uses), on the
CPU against Python integers, through the stand-alone program csrc/hosttest_pair_odd.cpp: this file writes scalars, the program answers
the folded k and the 64 digits of each (and ends with an error if its two ways to a digit differ), every answer is checked.  The
sanitizer build of the same program is `make sanitize-pair-odd`."""
import os
import random
import subprocess

import pair_odd_targets as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_pair_odd")
N = pt.N


def _run(tmp_path, scalars):
    f = tmp_path / "scalars.txt"
    f.write_text("".join("%064x\n" % u for u in scalars))
    out = subprocess.run([EXE, str(f)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(scalars)
    return [ln.split() for ln in lines]


def _check(u2, answer, walk_prefixes=True):
    """One answer against the integers; returns the windows at which the chain would meet an exceptional addition."""
    assert len(answer) == 65, (hex(u2), len(answer))
    sign = 0 if u2 & 1 else 1
    k = (N - u2) if sign else u2
    assert 0 < k < (1 << 256) and k & 1
    assert int(answer[0], 16) == (k & ~1) | sign, hex(u2)              # bit 0 of the folded word carries the sign
    digits = []
    for tok in answer[1:]:
        assert tok[0] in "+-" and tok[1:] in "01234567", (hex(u2), tok)
        digits.append((-1 if tok[0] == "-" else 1) * (2 * int(tok[1:]) + 1))    # odd and within +-15 by construction of the entry
    assert all(d & 1 and abs(d) <= 15 for d in digits)
    flip = -1 if sign else 1
    assert digits[63] * flip > 0, hex(u2)                             # the top digit of k is positive
    total = sum(d << (4 * i) for i, d in enumerate(digits))
    assert total * flip == k, hex(u2)                                   # the program applies the fold's sign: the digits sum to +-k
    assert total % N == u2 % N
    want_k, want_sign, want_digits = pt.recode(u2) if u2 < N else (k, sign, None)
    if want_digits is not None:
        assert (want_k, want_sign) == (k, sign) and [d * flip for d in digits] == want_digits, hex(u2)
    return pt.exceptional_windows([d * flip for d in digits]) if walk_prefixes else []


def test_named_scalars_and_window_patterns(tmp_path):
    below = pt.device_u2()
    for u in pt.named_u2():
        assert u in below
    above = [k for k in pt.window_patterns() if k >= N]                 # odd, so the fold leaves them: k = u2
    assert (1 << 256) - 1 in above and all(k & 1 for k in above)
    scalars = below + above
    bad = {}
    for u2, ans in zip(scalars, _run(tmp_path, scalars)):
        w = _check(u2, ans)
        if w:
            bad[u2] = w
    # k = n - 2 (from u2 = n - 2 and from u2 = 2) at window 0, and nothing else
    assert bad == {N - 2: [0], 2: [0]}, {hex(u): w for u, w in bad.items()}


def test_window_patterns_are_what_they_say(tmp_path):
    ks = pt.window_patterns()
    for k, ans in zip(ks, _run(tmp_path, ks)):
        entries = [int(tok[1:]) for tok in ans[1:]]
        h = k >> 1
        for i in range(63):
            x = (h >> (4 * i)) & 15
            assert entries[i] == (x - 8 if x >= 8 else 7 - x) and (ans[1 + i][0] == "+") == (x >= 8)
        assert entries[63] == h >> 252 and ans[64][0] == "+"
    tops = {int(ans[64][1:]) * 2 + 1 for ans in _run(tmp_path, ks)}
    assert tops == {1, 15}


def test_65536_random_scalars(tmp_path):
    rng = random.Random(20261021)
    scalars = [rng.randrange(1, N) for _ in range(65536)]
    bad = [hex(u2) for u2, ans in zip(scalars, _run(tmp_path, scalars)) if _check(u2, ans)]
    assert not bad, bad[:5]
