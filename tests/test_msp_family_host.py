"""MspFamilyTable and ParseHashFamily (csrc/msp_family.h), the registry mspid -> hash family that the P-384 stage of the block pass reads,
on the CPU: pure functions of strings, driven through the stand-alone program csrc/hosttest_msp_family.cpp - this file writes scripts of
registry commands, the program answers one line per command, every answer is checked (the sanitizer build of the same program is
`make sanitize-msp-family`)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_msp_family")

NOT_RECOGNIZED = "refused hash familiy not recognized [%s]"          # identity.getHashOpt's text (msp/identities.go:216-224), its spelling
SW_SERVES_IT = "refused failed computing digest: SHA3 is served by bccsp/sw, not by the GPU provider"


def _hex(s) -> str:
    b = s.encode() if isinstance(s, str) else s
    return b.hex() if b else "-"


class Script:
    """commands for the program, and the answer each must get"""

    def __init__(self):
        self.lines, self.want = [], []

    def do(self, cmd: str, want: str):
        self.lines.append(cmd)
        self.want.append(want)

    def set(self, mspid, family, want="ok"):
        self.do("set %s %s" % (_hex(mspid), _hex(family)), want)

    def get(self, mspid, want):
        self.do("get %s" % _hex(mspid), want)

    def run(self, tmp_path):
        f = tmp_path / "msp_family_script.txt"
        f.write_text("\n".join(self.lines) + "\n")
        out = subprocess.run([EXE, str(f)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        got = out.stdout.splitlines()
        assert len(got) == len(self.want)
        wrong = [(i, self.lines[i][:60], g, w) for i, (g, w) in enumerate(zip(got, self.want)) if g != w]
        assert not wrong, wrong[:5]


def test_every_msp_is_sha2_until_set_and_again_after_it_is_set_back(tmp_path):
    s = Script()
    s.do("sha3 1", "ok")
    s.get("Org1MSP", "SHA2")
    s.get("", "SHA2")
    s.do("count", "count 0")
    s.set("Org1MSP", "SHA3")
    s.get("Org1MSP", "SHA3")
    for near in ("Org1MS", "Org1MSPx", "org1msp", "Org2MSP", b"Org1MSP\0"):
        s.get(near, "SHA2")
    s.set("Org1MSP", "SHA3")                                 # twice: one entry
    s.do("count", "count 1")
    s.set("Org1MSP", "SHA2")
    s.get("Org1MSP", "SHA2")
    s.do("count", "count 0")
    s.set("Org2MSP", "SHA2")                                 # the default, said aloud
    s.do("count", "count 0")
    s.run(tmp_path)


def test_refused_families_carry_the_references_text_and_store_nothing(tmp_path):
    s = Script()
    s.do("sha3 1", "ok")
    for family in ("SHA1", "sha3", "SHA3 ", "SHA256", "SHA3_256", "SHA2x"):
        s.set("Org1MSP", family, NOT_RECOGNIZED % family)
    s.set("Org1MSP", "", NOT_RECOGNIZED % "")
    s.get("Org1MSP", "SHA2")
    s.set("", "SHA3", "refused invalid mspid")
    s.set("a" * 1025, "SHA3", "refused invalid mspid")
    s.set("a" * 1024, "SHA3")
    s.get("a" * 1024, "SHA3")
    s.get("a" * 1025, "SHA2")
    s.do("count", "count 1")
    s.run(tmp_path)


def test_sha3_is_refused_while_the_option_is_off(tmp_path):
    s = Script()
    s.set("Org1MSP", "SHA3", SW_SERVES_IT)                   # (the program starts with the option off, as the provider does)
    s.get("Org1MSP", "SHA2")
    s.set("Org1MSP", "SHA2")                                 # SHA2 needs no option
    s.set("Org1MSP", "SHA5", NOT_RECOGNIZED % "SHA5")        # an unknown family is unknown either way
    s.do("sha3 1", "ok")
    s.set("Org1MSP", "SHA3")
    s.do("sha3 0", "ok")
    s.get("Org1MSP", "SHA3")                                 # what was set stays set (the pass reads it only while the option is on)
    s.set("Org2MSP", "SHA3", SW_SERVES_IT)
    s.set("Org1MSP", "SHA2")                                 # ... and can be set back
    s.do("count", "count 0")
    s.run(tmp_path)


def test_many_msps(tmp_path):
    names = ["Org%dMSP" % i for i in range(3000)] + [bytes([1 + i % 255, 0, i // 255]) + b"MSP" for i in range(500)]     # (zero bytes inside a name)
    s = Script()
    s.do("sha3 1", "ok")
    for i, n in enumerate(names):
        if i % 3 == 0:
            s.set(n, "SHA3")
    s.do("count", "count %d" % len(range(0, len(names), 3)))
    for i, n in enumerate(names):
        s.get(n, "SHA3" if i % 3 == 0 else "SHA2")
    for i, n in enumerate(names):
        if i % 6 == 0:
            s.set(n, "SHA2")
    for i, n in enumerate(names):
        s.get(n, "SHA3" if i % 6 == 3 else "SHA2")
    s.run(tmp_path)


def test_the_programs_own_cases():
    """the cases the sanitizer build runs by default, readers beside a writer among them"""
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "0 failures", out.stdout + out.stderr
