"""Test helper beside tests/p384_blocks.py: signers of an MSP of the SHA3 hash family, whose signatures are over the SHA3-256 digest of
the message (msp/identities.go:216-224), for the tests of the P-384 stage's split by family.  Ground truth is p384_ref + hashlib, as there;
nothing of csrc/ is imported."""
import ctypes
import hashlib
import random

import numpy as np

import bccsp_sw_oracle as po
import blockbuilder as bb
import blockgen
import coracle
import p384_blocks as pb
import p384_ref as ref


def digest(msg: bytes, sha3: bool) -> bytes:
    return hashlib.sha3_256(msg).digest() if sha3 else hashlib.sha256(msg).digest()


class Signer(pb.Signer):
    """a P-384 key pair of MSP `mspid`; sign(msg) -> DER signature (low-S) over SHA3-256(msg) when sha3, over SHA-256(msg) otherwise"""

    def __init__(self, rnd: random.Random, cn: str, mspid: str, sha3: bool):
        super().__init__(rnd, cn)
        self.ident = pb.identity(self.q, mspid=mspid, cn=cn)
        self.mspid, self.sha3 = mspid, sha3

    def sign_rs(self, msg: bytes):
        e = ref.hash_to_int(digest(msg, self.sha3))
        while True:
            rs = ref.sign(self.d, e, self.rnd.randrange(1, ref.N))
            if rs:
                return rs[0], ref.low_s(rs[1])


class P256Sha3Signer:
    """P-256 fixture identity `which` (tests/golden/block_identities.json) under MSP `mspid`, signing over SHA3-256(msg)"""

    def __init__(self, which: int, mspid: str, seed: int):
        i = blockgen._IDS[which]
        self.ident = bb.serialized_identity(mspid, i["pem"])
        self.d32 = int(i["d"], 16).to_bytes(32, "big")
        self.rng = np.random.default_rng(seed)

    def sign(self, msg: bytes) -> bytes:
        nonce = b"\x00" + bytes(self.rng.integers(1, 255, size=31, dtype=np.uint8))
        r, s = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        assert coracle.lib().oracle_p256_sign(self.d32, hashlib.sha3_256(msg).digest(), nonce, 1, r, s) == 0
        return po.marshal_ecdsa_signature(int.from_bytes(r.raw, "big"), int.from_bytes(s.raw, "big"))


def tuple_status(q, msg: bytes, sig: bytes, sha3: bool) -> int:
    """p384_blocks.tuple_status with the digest of the family the pass hashes this tuple with"""
    if len(sig) == 0:
        return pb.TUPLE_ST_EMPTY_SIG
    rs = pb.parse_der_sig(sig)
    if rs is None:
        return pb.TUPLE_ST_BAD_DER
    return ref.status(q[0], q[1], ref.hash_to_int(digest(msg, sha3)), rs[0], rs[1])
