"""KeyedFence (csrc/keyed_fence.h), the wait between the retirement of a registered key and the reuse of what a keyed launch may still
read of it, on the CPU: the stand-alone program csrc/hosttest_keyed_fence.cpp runs the fence over a model of streams and events and
prints one line per case; every line is checked here (the sanitizer builds of the same program are `make sanitize-keyed-fence` and
`make sanitize-keyed-fence-thread`)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_keyed_fence")

CASES = ["quiet", "record", "done", "pooling", "drain_loops", "protocol"]


@pytest.fixture(scope="module")
def answers():
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    return out.returncode, out.stdout.splitlines(), out.stderr


def test_the_program_ran_every_case_and_counted_no_failure(answers):
    rc, lines, err = answers
    assert rc == 0 and lines[-1] == "0 failures", "\n".join(lines) + err
    assert [ln.split()[0] for ln in lines[:-1]] == CASES, lines


@pytest.mark.parametrize("case", CASES)
def test_case(answers, case):
    """quiet: the launcher count and its waiter; record: the remembered streams, destroyed and stuck ones; done: up to the recorded
    point; pooling: as many events made as were ever outstanding; drain_loops: advance and wait_for; protocol: launchers, a retirer
    and a completer in threads, and no read of a poisoned table"""
    rc, lines, err = answers
    assert case + " ok" in lines, "\n".join(lines) + err
