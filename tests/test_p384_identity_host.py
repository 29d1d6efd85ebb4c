"""IdentityToP384 (csrc/block_prepass.cpp), the identity decoder of the P-384 stage of the block pass, on the CPU: what it accepts, what
it refuses, and the stand-alone program that runs it over every prefix and every bit flip of an identity (the sanitizer build of the
same program is `make sanitize-p384-ident`)."""
import json
import os
import random
import subprocess

import pytest

import blockbuilder as bb
import fabgpu
import p384_blocks as pb
import p384_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def key():
    rnd = random.Random(384)
    return ref.mul(rnd.randrange(1, ref.N), ref.G)


def test_a_p384_certificate_yields_its_key(key):
    got = fabgpu.identity_to_p384(pb.identity(key))
    assert got == (ref.b48(key[0]), ref.b48(key[1]), True)
    # a v1 certificate (no [0] version) and another MSP id read the same
    assert fabgpu.identity_to_p384(pb.identity(key, mspid="AnotherOrgMSP"))[:2] == got[:2]


def test_identity_to_p256_refuses_the_p384_certificate(key):
    assert fabgpu.identity_to_p256(pb.identity(key)) is None


def test_p256_fixture_certificates_are_refused():
    ids = json.load(open(os.path.join(ROOT, "tests", "golden", "block_identities.json")))["identities"]
    seen = 0
    for i in ids:
        if i["curve"] != "prime256v1":
            continue
        ident = bb.serialized_identity("Org1MSP", i["pem"])
        assert fabgpu.identity_to_p256(ident) is not None and fabgpu.identity_to_p384(ident) is None
        seen += 1
    assert seen >= 1


def test_secp384r1_oid_with_a_65_byte_point_is_refused(key):
    short = b"\x04" + ref.b48(key[0])[:32] + ref.b48(key[1])[:32]
    assert fabgpu.identity_to_p384(bb.serialized_identity("Org1MSP", pb.pem(pb.cert_der(short)))) is None


@pytest.mark.parametrize("lead", [2, 3])
def test_compressed_points_are_refused(key, lead):
    assert fabgpu.identity_to_p384(bb.serialized_identity("Org1MSP", pb.pem(pb.cert_der(bytes([lead]) + ref.b48(key[0]))))) is None
    # ... and so is a 97-byte point that does not start with 04
    assert fabgpu.identity_to_p384(bb.serialized_identity("Org1MSP", pb.pem(pb.cert_der(bytes([lead]) + ref.b48(key[0]) + ref.b48(key[1]))))) is None


def test_p384_point_under_the_p256_oid_is_refused(key):
    prime256v1 = bytes.fromhex("2a8648ce3d030107")
    ident = bb.serialized_identity("Org1MSP", pb.pem(pb.cert_der(pb.uncompressed(key), curve_oid=prime256v1)))
    assert fabgpu.identity_to_p384(ident) is None and fabgpu.identity_to_p256(ident) is None


def test_off_curve_point_is_decoded_and_refused_by_the_on_curve_gate(key):
    bad = (key[0], (key[1] + 1) % ref.P)
    assert not ref.on_curve(*bad)
    got = fabgpu.identity_to_p384(pb.identity(bad))
    assert got == (ref.b48(bad[0]), ref.b48(bad[1]), False)
    assert fabgpu.load().fabgpu_p384_pubkey_on_curve(got[0], got[1]) == 0
    # coordinates that are not field elements: decoded, refused
    big = fabgpu.identity_to_p384(pb.identity((ref.P, key[1])))
    assert big is not None and big[2] is False


def test_every_truncation_is_refused(key):
    ident = pb.identity(key)
    assert all(fabgpu.identity_to_p384(ident[:n]) is None for n in range(len(ident)))


def test_idemix_identity_is_refused():
    assert fabgpu.identity_to_p384(bb.serialized_idemix_identity("IdemixOrg", b"\x01" * 32, b"\x02" * 32)) is None
    assert fabgpu.identity_to_p384(b"") is None


def test_stand_alone_program_over_prefixes_and_bit_flips(key, tmp_path):
    """the plain build of csrc/hosttest_p384_ident.cpp: its own generator identity, then one of this file's"""
    exe = os.path.join(ROOT, "fabric-mod_amd", "lib", "hosttest_p384_ident")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout + out.stderr
    f = tmp_path / "ident.bin"
    f.write_bytes(pb.identity(key))
    out = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout + out.stderr
    n_inputs = int(out.stdout.split(":")[1].split()[0])
    assert n_inputs == 1 + 9 * len(pb.identity(key))
