"""The eight-lanes-per-signature form of the registered-key P-384 verification on the host compilation: csrc/p384_wide.h's
verify_core_keyed_split - the partial sums of the eight lanes and the tree, the bodies the kernels of csrc/p384_wide_kernels.hip run -
beside verify_core_keyed, through the stand-alone program csrc/hosttest_p384_wide.cpp, against Python integers (p384_ref.py,
p384_wide_cases.py).  No device."""
import os
import subprocess

import pytest

import p384_ref as R
import p384_wide_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fabric-mod_amd", "csrc")


@pytest.fixture(scope="module")
def exe():
    """csrc/hosttest_p384_wide.cpp without sanitizers, through the Makefile (`make sanitize-p384-wide P384_WIDE_CASES=...` runs the same
    program under -fsanitize=address,undefined)"""
    out = subprocess.run(["make", "-C", CSRC, "-s", "../lib/hosttest_p384_wide"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_p384_wide")


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert out.returncode in (0, 1), out.stdout + out.stderr
    pairs = [tuple(int(v) for v in ln.split()) for ln in out.stdout.splitlines()]
    assert len(pairs) == len(lines), out.stderr
    return pairs


def test_the_crafted_list_is_what_the_issue_asks_for():
    cases, want = W.crafted(), W.crafted_expected()
    names = [c[0] for c in cases]
    for j in range(W.LANES):
        assert "lane %d idle: x(R) = r" % j in names and "only lane %d: x(R) = r" % j in names
    by = dict(zip(names, want))
    for lvl in (1, 2, 3):
        assert by["doubling at level %d: x(R) = r" % lvl] == 0 and by["doubling at level %d: one bit of e flipped" % lvl] == 1
        assert by["infinity at the root from level %d" % lvl] == 1
    assert by["infinity at level 1, live sums behind it: x(R) = r"] == 0 and by["infinity at level 2, live sums behind it: x(R) = r"] == 0
    assert by["eight lanes cancel pairwise"] == 1
    assert [by["gate: " + g] for g in ("r = 0", "s = 0", "r = n", "s = n", "r > n", "s > n", "s high")] == [3, 3, 3, 2, 3, 2, 2]
    assert [w for c, w in zip(cases, want) if c[3] != W.LIVE] == [4, 4, 4, 2, 3]
    for n, w in by.items():
        if n.endswith("x(R) = r") or n.startswith("signature under") and "flipped" not in n:
            assert w == 0, n
        if n.endswith("flipped") or n.endswith("any s") or n.startswith("in-lane cancellation"):
            assert w == 1, n
    # the digits are where the names say: a lane the case calls idle has twelve zero digits (the twin's flipped e moves u1: not looked at)
    for (name, _key, row, _kind), w in zip(cases, want):
        if name.startswith("lane ") and "idle" in name and not name.endswith("flipped"):
            j = int(name.split()[1])
            ws = pow(row[4], -1, R.N)
            for u in (row[2] * ws % R.N, row[3] * ws % R.N):
                assert (u >> (48 * j)) & (2**48 - 1) == 0 and u != 0


def test_split_and_one_lane_cores_agree_with_the_reference_on_the_crafted_list(exe):
    cases, want = W.crafted(), W.crafted_expected()
    got = _run(exe, [W.case_line(row, kind == W.LIVE) for _n, _k, row, kind in cases])
    for (name, _k, _row, _kind), (one, split), w in zip(cases, got, want):
        assert one == split == w, (name, one, split, w)


def test_split_and_one_lane_cores_agree_with_the_reference_on_256_signatures(exe):
    rows, want = W.random256()
    got = _run(exe, [W.case_line(row) for _k, row in rows])
    assert [g[0] for g in got] == list(want)
    assert [g[1] for g in got] == list(want)
