"""ECDSA P-384 on the CPU: the Python-integer reference (p384_ref.py) pinned against openssl, and the host compilation of csrc/p384.h
run primitive by primitive against Python integers (libfabgpu_hosttest.so).  No GPU."""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import pytest

import fabgpu
import p384_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
P, N = R.P, R.N


@pytest.fixture(scope="module")
def H():
    p = os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_hosttest.so")
    if not os.path.exists(p):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(p)
    L.hosttest_p384_verify.restype = ctypes.c_uint32
    return L


@pytest.fixture(scope="module")
def kats():
    return json.load(open(os.path.join(GOLD, "p384_kats.json")))["vectors"]


def _tuple(v):
    return (int(v["qx"], 16), int(v["qy"], 16), R.hash_to_int(bytes.fromhex(v["digest"])), int(v["r"], 16), int(v["s"], 16))


# ---- the reference itself ----
def test_reference_agrees_with_openssl_on_the_fixtures(kats):
    assert len(kats) >= 48 and {v["hash"] for v in kats} == {"sha256", "sha384"}
    assert any(not v["low_s"] for v in kats) and any(v["low_s"] and not v["as_produced"] for v in kats)
    for v in kats:
        qx, qy, e, r, s = _tuple(v)
        assert v["openssl_verifies"] and R.on_curve(qx, qy)
        assert R.verify_math((qx, qy), e, r, s)                          # openssl accepts both s and n - s
        assert R.status(qx, qy, e, r, s) == (R.ST_VALID if v["low_s"] else R.ST_HIGH_S)
        assert R.status(qx, qy, e ^ 1, r, s) in (R.ST_BAD_MATH, R.ST_HIGH_S)


def test_reference_knows_the_p384_certificate_of_the_block_fixtures():
    ids = json.load(open(os.path.join(GOLD, "block_identities.json")))["identities"]
    p384 = [i for i in ids if i.get("curve") == "secp384r1"]
    assert len(p384) == 1
    d, qx, qy = (int(p384[0][k], 16) for k in ("d", "qx", "qy"))
    assert R.mul(d, R.G) == (qx, qy) and R.on_curve(qx, qy)
    pub = subprocess.run(["openssl", "x509", "-noout", "-pubkey"], input=p384[0]["pem"].encode(), capture_output=True, check=True).stdout
    text = subprocess.run(["openssl", "ec", "-pubin", "-noout", "-text"], input=pub, capture_output=True, check=True).stdout.decode()
    hexpub = "".join(text.split("pub:")[1].split("ASN1 OID")[0].replace(":", "").split())
    assert hexpub == "04" + p384[0]["qx"] + p384[0]["qy"]


def test_openssl_verifies_signatures_the_reference_produces(tmp_path):

    rng = random.Random(384)
    key = tmp_path / "k.pem"
    subprocess.run(["openssl", "ecparam", "-name", "secp384r1", "-genkey", "-noout", "-out", str(key)], check=True, capture_output=True)
    text = subprocess.run(["openssl", "ec", "-in", str(key), "-noout", "-text"], check=True, capture_output=True).stdout.decode()
    d = int("".join(text.split("priv:")[1].split("pub:")[0].replace(":", "").split()), 16)
    for hname in ("sha256", "sha384"):
        dg = hashlib.new(hname, b"made by the reference " + hname.encode()).digest()
        r, s = R.sign(d, R.hash_to_int(dg), rng.randrange(1, N))
        (tmp_path / "d.bin").write_bytes(dg)
        (tmp_path / "s.bin").write_bytes(R.der_sig(r, s))
        rc = subprocess.run(["openssl", "pkeyutl", "-verify", "-inkey", str(key), "-in", str(tmp_path / "d.bin"), "-sigfile", str(tmp_path / "s.bin")],
                            capture_output=True)
        assert rc.returncode == 0, rc.stdout + rc.stderr
        (tmp_path / "s.bin").write_bytes(R.der_sig(r, (s + 1) % N or 1))
        assert subprocess.run(["openssl", "pkeyutl", "-verify", "-inkey", str(key), "-in", str(tmp_path / "d.bin"), "-sigfile", str(tmp_path / "s.bin")],
                              capture_output=True).returncode != 0


# ---- the host compilation of p384.h, primitive by primitive ----
def _op(fn, op, a, b, n=48):
    out = ctypes.create_string_buffer(n)
    fn(op, a, b, out)
    return out.raw


def _limb_patterns(m):
    vals = {0, 1, 2, m - 1, m - 2, (m - 1) // 2, 2**383 % m, (2**384 - 1) % m}
    for k in range(1, 12):                                   # limb ends: 2^(32k) - 1, 2^(32k), 2^(32k) + 1, all-ones words alternating
        vals |= {(2**(32 * k) - 1) % m, 2**(32 * k) % m, (2**(32 * k) + 1) % m, (m - 2**(32 * k)) % m}
    vals.add(int("ffffffff00000000" * 6, 16) % m)
    vals.add(int("00000000ffffffff" * 6, 16) % m)
    return sorted(vals)


def test_field_operations_against_python_integers(H):
    rng = random.Random(1)
    special = _limb_patterns(P)
    pairs = [(a, b) for a in special for b in special[::3]] + [(rng.randrange(P), rng.randrange(P)) for _ in range(3000)]
    for a, b in pairs:
        A_, B_ = R.b48(a), R.b48(b)
        assert int.from_bytes(_op(H.hosttest_p384_fp_op, 0, A_, B_), "big") == a * b % P
        assert int.from_bytes(_op(H.hosttest_p384_fp_op, 2, A_, B_), "big") == (a + b) % P
        assert int.from_bytes(_op(H.hosttest_p384_fp_op, 3, A_, B_), "big") == (a - b) % P
    for a in special + [rng.randrange(P) for _ in range(500)]:
        A_ = R.b48(a)
        assert int.from_bytes(_op(H.hosttest_p384_fp_op, 1, A_, A_), "big") == a * a % P
        assert int.from_bytes(_op(H.hosttest_p384_fp_op, 4, A_, A_), "big") == a
    for a in (1, 2, P - 1, rng.randrange(1, P)):
        assert int.from_bytes(_op(H.hosttest_p384_fp_op, 5, R.b48(a), R.b48(0)), "big") == pow(a, -1, P)


def test_raw_montgomery_products_for_both_moduli(H):
    rng = random.Random(2)
    for field, m in ((1, P), (0, N)):
        rinv = pow(2**384, -1, m)
        sp = _limb_patterns(m)
        for a, b in [(a, b) for a in sp[::2] for b in sp[::5]] + [(rng.randrange(m), rng.randrange(m)) for _ in range(2000)]:
            assert int.from_bytes(_op(H.hosttest_p384_mont_mul, field, R.b48(a), R.b48(b)), "big") == a * b * rinv % m


def test_scalar_operations_and_the_inverse(H):
    rng = random.Random(3)
    for a in [1, 2, N - 1, N - 2, 2**192 % N, (N - 1) // 2] + [rng.randrange(1, N) for _ in range(60)]:
        assert int.from_bytes(_op(H.hosttest_p384_fn_op, 1, R.b48(a), R.b48(0)), "big") == pow(a, -1, N)
        b = rng.randrange(N)
        assert int.from_bytes(_op(H.hosttest_p384_fn_op, 0, R.b48(a), R.b48(b)), "big") == a * b % N
    assert int.from_bytes(_op(H.hosttest_p384_fn_op, 1, R.b48(0), R.b48(0)), "big") == 0
    for a in (0, N - 1, N, N + 1, 2**384 - 1):
        assert int.from_bytes(_op(H.hosttest_p384_fn_op, 2, R.b48(a), R.b48(0)), "big") == a % N


def _jac(pt, z):
    """an affine point (None: infinity) as Jacobian bytes with the given Z"""
    if pt is None:
        return R.b48(1) + R.b48(1) + R.b48(0)
    return R.b48(pt[0] * z * z % P) + R.b48(pt[1] * z * z * z % P) + R.b48(z % P)


def _aff(raw):
    x, y, z = (int.from_bytes(raw[48 * k:48 * k + 48], "big") for k in range(3))
    if z == 0:
        return None
    zi = pow(z, -1, P)
    return (x * zi * zi % P, y * zi * zi * zi % P)


def test_point_operations_every_case(H):
    rng = random.Random(4)
    pts = [R.mul(rng.randrange(1, N), R.G) for _ in range(12)] + [R.G, R.neg(R.G)]
    for p in pts:
        z1, z2 = rng.randrange(1, P), rng.randrange(1, P)
        q = pts[rng.randrange(len(pts))]
        assert _aff(_op(H.hosttest_p384_pt_op, 0, _jac(p, z1), _jac(p, 1), 144)) == R.add(p, p)
        assert _aff(_op(H.hosttest_p384_pt_op, 1, _jac(p, z1), _jac(q, z2), 144)) == R.add(p, q)
        assert _aff(_op(H.hosttest_p384_pt_op, 2, _jac(p, z1), _jac(q, 1), 144)) == R.add(p, q)
        for op, zb in ((1, z2), (2, 1)):
            assert _aff(_op(H.hosttest_p384_pt_op, op, _jac(p, z1), _jac(p, zb), 144)) == R.add(p, p)           # P + P
            assert _aff(_op(H.hosttest_p384_pt_op, op, _jac(p, z1), _jac(R.neg(p), zb), 144)) is None            # P + (-P)
            assert _aff(_op(H.hosttest_p384_pt_op, op, _jac(None, 0), _jac(p, zb), 144)) == p                    # infinity on the left
        assert _aff(_op(H.hosttest_p384_pt_op, 1, _jac(p, z1), _jac(None, 0), 144)) == p                         # ... on the right
    assert _aff(_op(H.hosttest_p384_pt_op, 1, _jac(None, 0), _jac(None, 0), 144)) is None
    assert _aff(_op(H.hosttest_p384_pt_op, 0, _jac(None, 0), _jac(None, 0), 144)) is None


def test_generator_table_is_the_multiples_of_g(H):
    for j in range(1, 16):
        out = ctypes.create_string_buffer(96)
        H.hosttest_p384_gtab_entry(j, out)
        assert (int.from_bytes(out.raw[:48], "big"), int.from_bytes(out.raw[48:], "big")) == R.mul(j, R.G)


def test_both_acceptance_branches(H):
    rng = random.Random(5)
    k = 0
    while R.lift_x(N + k) is None:
        k += 1
    pt = R.lift_x(N + k)                     # x = n + k < p: x mod n = k
    z = rng.randrange(1, P)
    assert H.hosttest_p384_x_equals_r(_jac(pt, z), R.b48(k)) == 1            # the second branch: X == (r + n) Z^2
    assert H.hosttest_p384_x_equals_r(_jac(pt, z), R.b48(k + 1)) == 0
    q = R.mul(77, R.G)
    assert H.hosttest_p384_x_equals_r(_jac(q, z), R.b48(q[0] % N)) == 1
    assert H.hosttest_p384_x_equals_r(_jac(None, 0), R.b48(1)) == 0          # infinity rejects


def test_host_core_on_the_fixtures_and_their_mutations(H, kats):
    rng = random.Random(6)
    for v in kats[::3]:
        t = list(_tuple(v))
        assert H.hosttest_p384_verify(*map(R.b48, t)) == R.status(*t)
        i = rng.randrange(5)
        t[i] ^= 1 << rng.randrange(384 if i != 2 else 256)
        assert H.hosttest_p384_verify(*map(R.b48, t)) == R.status(*t)


# ---- the pure-host entries of the C ABI ----
def test_hash_to_int_at_every_digest_length():
    for ln in (20, 32, 48, 64):
        dg = bytes(range(1, ln + 1))
        e = fabgpu.hash_to_int_p384(dg)
        assert len(e) == 48 and int.from_bytes(e, "big") == R.hash_to_int(dg) == int.from_bytes(dg[:48], "big")


def test_low_s_and_curve_gates():
    assert fabgpu.is_low_s_p384(R.b48(R.HALF_N)) and not fabgpu.is_low_s_p384(R.b48(R.HALF_N + 1))
    assert fabgpu.is_low_s_p384(R.b48(1)) and not fabgpu.is_low_s_p384(R.b48(N - 1))
    assert fabgpu.p384_pubkey_on_curve(R.b48(R.GX), R.b48(R.GY))
    assert not fabgpu.p384_pubkey_on_curve(R.b48(R.GX), R.b48(R.GY ^ 1))
    assert not fabgpu.p384_pubkey_on_curve(R.b48(P), R.b48(R.GY))            # a coordinate >= p
    x = 2**384 - 1                                                           # x mod p on the curve would still be refused
    assert not fabgpu.p384_pubkey_on_curve(R.b48(x), R.b48(1))


def test_der_gate_on_the_p256_vectors_and_48_byte_values(kats):
    vec = json.load(open(os.path.join(GOLD, "der_kats.json")))["vectors"]
    assert len(vec) > 10
    for v in vec:                                    # the DER rules do not depend on the curve: same verdict as the P-256 entry
        raw = bytes.fromhex(v["der"])
        rc32, r32, s32, fl32 = fabgpu.unmarshal_ecdsa_signature(raw)
        rc, r48, s48, fl = fabgpu.unmarshal_signature_p384(raw)
        assert rc == rc32 and (rc == 0) == bool(v["ok"]), v["name"]
        if rc == 0 and fl32 == 0:
            assert fl == 0 and r48 == bytes(16) + r32 and s48 == bytes(16) + s32
    for v in kats[:20]:                              # 48-byte values
        rc, r48, s48, fl = fabgpu.unmarshal_signature_p384(bytes.fromhex(v["der"]))
        assert (rc, fl) == (0, 0) and r48.hex() == v["r"] and s48.hex() == v["s"]

    rc, r48, s48, fl = fabgpu.unmarshal_signature_p384(R.der_sig(2**384 + 5, 2**400))
    assert rc == 0 and fl == 3 and int.from_bytes(r48, "big") == 5 and int.from_bytes(s48, "big") == 0
    rc, r48, s48, fl = fabgpu.unmarshal_signature_p384(R.der_sig(2**384 - 1, 1))
    assert rc == 0 and fl == 0 and r48 == b"\xff" * 48
    assert fabgpu.unmarshal_signature_p384(R.der_sig(0, 1))[0] == 2 and fabgpu.unmarshal_signature_p384(R.der_sig(1, 0))[0] == 3


def test_standalone_host_program_over_the_fixtures(tmp_path, kats):
    """csrc/hosttest_p384.cpp (its own main, built by the Makefile) over the fixture vectors and their mutations; the Makefile's
    sanitize-p384 target runs the same program under -fsanitize=address,undefined."""
    exe = os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_p384")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    rng = random.Random(7)
    lines = []
    for v in kats:
        t = list(_tuple(v))
        lines.append(t + [R.status(*t)])
        t = list(t)
        t[rng.randrange(5)] ^= 1 << rng.randrange(256)
        lines.append(t + [R.status(*t)])
    vec = tmp_path / "p384_vectors.txt"
    vec.write_text("".join("%x %x %x %x %x %d\n" % tuple(ln) for ln in lines))
    out = subprocess.run([exe, str(vec)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "%d tuples, 0 failures" % len(lines) in out.stdout


def test_refusal_text_of_a_provider_whose_p384_option_is_off():
    """The text itself, from the product library without a device (a provider needs one: tests/test_p384_gpu.py asks a real provider
    with the option off), and the header documents the same words."""
    text = fabgpu.load_hooks().fabgpu_test_p384_refusal_text().decode()
    assert text == "P-384 is served by bccsp/sw, not by the GPU provider"
    assert text in " ".join(open(os.path.join(ROOT, "include", "fabgpu_bccsp.h")).read().replace(" * ", " ").split())
