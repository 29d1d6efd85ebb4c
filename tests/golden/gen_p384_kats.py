#!/usr/bin/env python3
"""Writes tests/golden/p384_kats.json: ECDSA P-384 signatures made by the `openssl` command line.

Fresh secp384r1 keys; each signs SHA-256 and SHA-384 digests of short messages (`openssl pkeyutl -sign` over the raw digest).  A
signature that was low-S as produced is stored as produced; one that was not is stored both as produced (`as_produced`: true,
`low_s`: false) and with s replaced by n - s.  Every vector carries what `openssl pkeyutl -verify` said about the stored (r, s).

    python3 tests/golden/gen_p384_kats.py            # needs openssl on PATH; rewrites the file (fresh keys every time)
"""
import hashlib
import json
import os
import re
import subprocess
import tempfile

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFC7634D81F4372DDF581A0DB248B0A77AECEC196ACCC52973
HERE = os.path.dirname(os.path.abspath(__file__))


def run(*a, **kw):
    return subprocess.run(a, check=True, capture_output=True, **kw).stdout


def der_int(v):
    b = v.to_bytes((v.bit_length() + 8) // 8 or 1, "big")
    return b"\x02" + bytes([len(b)]) + b


def der_sig(r, s):
    body = der_int(r) + der_int(s)
    return b"\x30" + (bytes([len(body)]) if len(body) < 128 else b"\x81" + bytes([len(body)])) + body


def parse_sig(der):
    assert der[0] == 0x30
    i = 2 if der[1] < 128 else 3
    out = []
    for _ in range(2):
        assert der[i] == 2
        ln = der[i + 1]
        out.append(int.from_bytes(der[i + 2:i + 2 + ln], "big"))
        i += 2 + ln
    return out


def main():
    vectors = []
    with tempfile.TemporaryDirectory() as td:
        for k in range(6):
            key = os.path.join(td, "k%d.pem" % k)
            pub = os.path.join(td, "p%d.pem" % k)
            run("openssl", "ecparam", "-name", "secp384r1", "-genkey", "-noout", "-out", key)
            run("openssl", "ec", "-in", key, "-pubout", "-out", pub)
            text = run("openssl", "ec", "-in", key, "-noout", "-text").decode()
            hexpub = re.sub(r"[\s:]", "", text.split("pub:")[1].split("ASN1 OID")[0])
            assert hexpub.startswith("04") and len(hexpub) == 2 + 192
            qx, qy = hexpub[2:98], hexpub[98:]
            for j in range(4):
                msg = ("p384 kat key %d message %d" % (k, j)).encode() * (j + 1)
                for hname in ("sha256", "sha384"):
                    dg = hashlib.new(hname, msg).digest()
                    dgf, sgf = os.path.join(td, "d.bin"), os.path.join(td, "s.bin")
                    open(dgf, "wb").write(dg)
                    run("openssl", "pkeyutl", "-sign", "-inkey", key, "-in", dgf, "-out", sgf)
                    r, s = parse_sig(open(sgf, "rb").read())
                    forms = [(r, s, True)] + ([(r, N - s, False)] if s > N >> 1 else [])
                    for rr, ss, produced in forms:
                        open(sgf, "wb").write(der_sig(rr, ss))
                        ok = subprocess.run(["openssl", "pkeyutl", "-verify", "-pubin", "-inkey", pub, "-in", dgf, "-sigfile", sgf],
                                            capture_output=True).returncode == 0
                        vectors.append({"key": k, "qx": qx, "qy": qy, "msg": msg.hex(), "hash": hname, "digest": dg.hex(),
                                        "r": "%096x" % rr, "s": "%096x" % ss, "der": der_sig(rr, ss).hex(), "as_produced": produced,
                                        "low_s": ss <= N >> 1, "openssl_verifies": ok})
    out = {"generator": "tests/golden/gen_p384_kats.py (openssl %s)" % run("openssl", "version").decode().split()[1], "vectors": vectors}
    with open(os.path.join(HERE, "p384_kats.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(len(vectors), "vectors;", sum(1 for v in vectors if not v["low_s"]), "high-S as produced")


if __name__ == "__main__":
    main()
