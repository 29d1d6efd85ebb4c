"""Test helper: P-384 identities and blocks signed by them, for the tests of the P-384 stage of the block pass.

A certificate is DER built here (blockgen.der_tlv) around a secp384r1 SubjectPublicKeyInfo; its own signature field is arbitrary bytes -
the pass reads the key out of the certificate and never checks chains (msp/mspimplvalidate.go does).  Signatures come from p384_ref.sign
under a seeded `random`; blocks from blockgen's / blockbuilder's envelope helpers.  Ground truth for the tests that use this file is
p384_ref + hashlib + the flag fold restated in fold_flags below; nothing of csrc/ is imported.
"""
import base64
import hashlib
import random

import blockbuilder as bb
import blockgen
import p384_ref as ref

OID_EC_PUBLIC_KEY = bytes.fromhex("2a8648ce3d0201")      # 1.2.840.10045.2.1
OID_SECP384R1 = bytes.fromhex("2b81040022")              # 1.3.132.0.34
OID_ECDSA_SHA384 = bytes.fromhex("2a8648ce3d040303")

TUPLE_ST_BAD_DER, TUPLE_ST_NEEDS_SW, TUPLE_ST_EMPTY_SIG = 5, 6, 7
TX_VALID, TX_BAD_CREATOR, TX_BAD_ENDORSEMENT, TX_NOT_UNDERSTOOD, TX_NEEDS_SW, TX_BAD_TXID, TX_BAD_PHASH = 0, 1, 2, 3, 4, 5, 6

tlv = blockgen.der_tlv


def _name(cn: str) -> bytes:
    return tlv(0x30, tlv(0x31, tlv(0x30, tlv(0x06, bytes.fromhex("550403")) + tlv(0x0C, cn.encode()))))


def spki(point: bytes, curve_oid: bytes = OID_SECP384R1) -> bytes:
    """SubjectPublicKeyInfo{{id-ecPublicKey, curve}, BIT STRING 00 || point}"""
    return tlv(0x30, tlv(0x30, tlv(0x06, OID_EC_PUBLIC_KEY) + tlv(0x06, curve_oid)) + tlv(0x03, b"\x00" + point))


def cert_der(point: bytes, curve_oid: bytes = OID_SECP384R1, cn: str = "peer0.org1.example.com", serial: int = 0x5A5A) -> bytes:
    """an x509 v3 certificate around `point` (the bytes behind the BIT STRING's unused-bits octet: 04 || X || Y for a usual key)"""
    alg = tlv(0x30, tlv(0x06, OID_ECDSA_SHA384))
    validity = tlv(0x30, tlv(0x17, b"250101000000Z") + tlv(0x17, b"350101000000Z"))
    tbs = tlv(0x30, tlv(0xA0, tlv(0x02, b"\x02")) + tlv(0x02, serial.to_bytes(8, "big")) + alg + _name("ca.org1.example.com") + validity + _name(cn) +
              spki(point, curve_oid))
    return tlv(0x30, tbs + alg + tlv(0x03, b"\x00" + hashlib.sha384(tbs).digest() * 2))


def pem(der: bytes) -> str:
    b = base64.b64encode(der).decode()
    return "-----BEGIN CERTIFICATE-----\n" + "\n".join(b[i:i + 64] for i in range(0, len(b), 64)) + "\n-----END CERTIFICATE-----\n"


def uncompressed(q) -> bytes:
    return b"\x04" + ref.b48(q[0]) + ref.b48(q[1])


def identity(q, mspid: str = "Org1MSP", cn: str = "peer0.org1.example.com") -> bytes:
    """SerializedIdentity{mspid, PEM certificate with the P-384 key q = (x, y)}"""
    return bb.serialized_identity(mspid, pem(cert_der(uncompressed(q), cn=cn)))


class Signer:
    """a P-384 key pair with its identity; sign(msg) -> DER signature (low-S) over SHA-256(msg), nonces from the shared seeded generator"""

    def __init__(self, rnd: random.Random, cn: str):
        self.d = rnd.randrange(1, ref.N)
        self.q = ref.mul(self.d, ref.G)
        self.ident = identity(self.q, cn=cn)
        self.rnd = rnd

    def sign_rs(self, msg: bytes):
        e = ref.hash_to_int(hashlib.sha256(msg).digest())
        while True:
            rs = ref.sign(self.d, e, self.rnd.randrange(1, ref.N))
            if rs:
                return rs[0], ref.low_s(rs[1])

    def sign(self, msg: bytes) -> bytes:
        return ref.der_sig(*self.sign_rs(msg))


def signers(n: int, seed: int):
    rnd = random.Random(seed)
    return [Signer(rnd, "signer%d.org1.example.com" % i) for i in range(n)]


def off_curve_identity(seed: int) -> bytes:
    """a certificate whose secp384r1 point is not on the curve (y + 1)"""
    rnd = random.Random(seed)
    q = ref.mul(rnd.randrange(1, ref.N), ref.G)
    return identity((q[0], (q[1] + 1) % ref.P), cn="offcurve.org1.example.com")


def tuple_status(q, msg: bytes, sig: bytes) -> int:
    """what the pass must say of one P-384 tuple: the host gate's outcomes (empty, DER, high S, r of more than 384 bits) and then
    p384_ref.status over SHA-256(msg) as a 256-bit e"""
    if len(sig) == 0:
        return TUPLE_ST_EMPTY_SIG
    rs = parse_der_sig(sig)
    if rs is None:
        return TUPLE_ST_BAD_DER
    r, s = rs
    return ref.status(q[0], q[1], ref.hash_to_int(hashlib.sha256(msg).digest()), r, s)


def parse_der_sig(sig: bytes):
    """SEQUENCE{INTEGER r, INTEGER s} with minimal positive integers -> (r, s), or None (what UnmarshalECDSASignature refuses)"""
    def take(b, tag):
        if len(b) < 2 or b[0] != tag:
            return None
        n, i = b[1], 2
        if n & 0x80:
            k = n & 0x7F
            if k == 0 or k > 2 or len(b) < 2 + k:
                return None
            n = int.from_bytes(b[2:2 + k], "big")
            i = 2 + k
            if n < 128 or (k == 2 and n < 256):
                return None
        if len(b) < i + n:
            return None
        return b[i:i + n], b[i + n:]
    seq = take(sig, 0x30)
    if seq is None:
        return None
    body = seq[0]
    out = []
    for _ in range(2):
        t = take(body, 0x02)
        if t is None:
            return None
        v, body = t
        if len(v) == 0 or v[0] & 0x80 or (len(v) > 1 and v[0] == 0 and not v[1] & 0x80):
            return None
        out.append(int.from_bytes(v, "big"))
    if out[0] == 0 or out[1] == 0:
        return None
    return out[0], out[1]


def fold_flags(n_tx, understood, tuple_tx, tuple_kind, tuple_st, bad_txid=None, bad_phash=None):
    """block_prepass.h SummarizeTransactions, restated: not understood > bad creator > bad TxID > bad proposal hash > bad endorsement >
    needs bccsp/sw > valid"""
    flags = []
    for t in range(n_tx):
        mine = [(k, s) for tx, k, s in zip(tuple_tx, tuple_kind, tuple_st) if tx == t and s != 0]
        if not understood[t]:
            flags.append(TX_NOT_UNDERSTOOD)
        elif any(k == 0 and s != TUPLE_ST_NEEDS_SW for k, s in mine):
            flags.append(TX_BAD_CREATOR)
        elif bad_txid is not None and bad_txid[t]:
            flags.append(TX_BAD_TXID)
        elif bad_phash is not None and bad_phash[t]:
            flags.append(TX_BAD_PHASH)
        elif any(k != 0 and s != TUPLE_ST_NEEDS_SW for k, s in mine):
            flags.append(TX_BAD_ENDORSEMENT)
        elif any(s == TUPLE_ST_NEEDS_SW for _, s in mine):
            flags.append(TX_NEEDS_SW)
        else:
            flags.append(TX_VALID)
    return flags


def endorser_tx(rnd: random.Random, creator, endorsers, creator_sig=None, end_sig=None, ext_bytes=200):
    """One envelope.  creator / endorsers: objects with .ident and .sign(msg).  creator_sig(payload, sig) / end_sig(j, msg, sig) may
    replace a signature's bytes.  -> (envelope, [(kind, identity, message, signature)]: the tuples as the pass lists them)"""
    tuples = []

    def ends(prp):
        out = []
        for j, e in enumerate(endorsers):
            msg = prp + e.ident
            sig = e.sign(msg)
            if end_sig is not None:
                sig = end_sig(j, msg, sig)
            out.append((e.ident, sig))
            tuples.append((1, e, msg, sig))
        return out
    payload, _ = bb.consistent_endorser_tx("mychannel", creator.ident, rnd.randbytes(24), rnd.randbytes(120), rnd.randbytes(ext_bytes), ends)
    sig = creator.sign(payload)
    if creator_sig is not None:
        sig = creator_sig(payload, sig)
    tuples.insert(0, (0, creator, payload, sig))
    return bb.envelope(payload, sig), tuples
