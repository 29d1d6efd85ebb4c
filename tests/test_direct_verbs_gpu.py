"""The provider's direct-call verbs (csrc/bccsp_host.cpp VerifyBatchT / IdentityVerifyBatchT / VerifyCoalescedT, one body for P-256 and
P-384) on rows the host gate does NOT submit, sitting between submitted rows at tile and word edges: every row's (valid, text) against
the oracle of its own curve, with fresh keys and with every key registered, in both hash families; the coalesced verbs and the
single-row C entries give each row the answer it got in the batch.

Oracles: P-256 - oracle/bccsp_sw_oracle.py (csp_verify, identity_verify, the exceptions' texts).  P-384 - tests/p384_ref.py for the
arithmetic and the half order, behind the same checks in bccsp/sw's order and with the texts tests/test_p384_gpu.py expects (they are
literals inside its tests, so there is no table to import); the DER texts come from the oracle's parser, which knows no curve, and are
compared whole, with the class Go's asn1 package prints in front of the reason.  The text for a key that is not on the curve is the provider's own (the reference refuses such a key at import)."""
import ctypes
import hashlib
import random
import threading

import pytest

import bccsp_sw_oracle as po
import fabgpu
import p384_ref as R

pytestmark = pytest.mark.gpu

WRAP = "Failed verifing with opts [<nil>]: "
IDENT = "could not determine the validity of the signature: "
POISONED = "GPU provider poisoned: the CPU audit disagrees with the device (use bccsp/sw)"
SIZES = [1, 2, 63, 64, 65, 129]
# row kinds; the gate submits VALID, BAD_MATH and TRAILING (Go's parser discards bytes behind the SEQUENCE), nothing else
VALID, BAD_MATH, HIGH_S, NON_MINIMAL, EMPTY_SIG, OFF_CURVE, WIDE_R, TRAILING = range(8)
SUBMITTED = (VALID, BAD_MATH, TRAILING)
NOT_SUBMITTED = (HIGH_S, NON_MINIMAL, EMPTY_SIG, OFF_CURVE, WIDE_R)
FILLER_MSGS = [b"", b"f" * 64, b"seven b", b"g" * 129]         # messages of non-submitted identity rows: never staged


class P256:
    name, width, n, half_n, g = "P-256", 32, po.N, po.HALF_N, (po.GX, po.GY)
    mul = staticmethod(po.pt_mul)
    on_curve = staticmethod(po.on_curve)

    @staticmethod
    def sign(d, digest, k):
        return po.sign_raw(d, digest, k)

    @staticmethod
    def verify(key, sig, digest):
        """(valid, text or None) of CSP.Verify"""
        try:
            return po.csp_verify(key, sig, digest), None
        except po.BCCSPError as e:
            return False, str(e)

    @staticmethod
    def provider_key(key):
        return fabgpu.ECDSAPublicKey(*key)


class P384:
    name, width, n, half_n, g = "P-384", 48, R.N, R.HALF_N, R.G
    mul = staticmethod(R.mul)
    on_curve = staticmethod(R.on_curve)

    @staticmethod
    def sign(d, digest, k):
        r, s = R.sign(d, R.hash_to_int(digest), k)
        return r, R.low_s(s)

    @staticmethod
    def verify(key, sig, digest):
        if key is None:
            return False, "Invalid Key. It must not be nil."
        if not sig:
            return False, "Invalid signature. Cannot be empty."
        if not digest:
            return False, "Invalid digest. Cannot be empty."
        try:
            r, s = po.unmarshal_ecdsa_signature(sig)
        except po.BCCSPError as e:
            return False, WRAP + "Failed unmashalling signature [%s]" % e
        if s > R.HALF_N:
            return False, WRAP + "Invalid S. Must be smaller than half the order [%d][%d]." % (s, R.HALF_N)
        return R.status(key[0], key[1], R.hash_to_int(digest), r, s) == R.ST_VALID, None

    @staticmethod
    def provider_key(key):
        return key


def _go_text(text):
    """The oracle's parser names the reason of an asn1 failure alone; Go's asn1.StructuralError prints it behind its class (encoding/asn1
    asn1.go: parseBigInt's "integer not minimally-encoded" is a StructuralError).  The only DER failure among the rows is that one."""
    return text and text.replace("[integer not minimally-encoded]", "[asn1: structure error: integer not minimally-encoded]")


def _hash(sha3, msg):
    return (hashlib.sha3_256 if sha3 else hashlib.sha256)(msg).digest()


class Rows:
    """One row of every kind per signed message, for one curve and one hash family, and the oracle's answer to each - computed once."""

    def __init__(self, curve, sha3):
        self.curve, self.sha3 = curve, sha3
        rng = random.Random(20260 + curve.width + sha3)
        self.keys = []
        for _ in range(3):
            d = rng.randrange(1, curve.n)
            self.keys.append((d, curve.mul(d, curve.g)))
        self.rows = {k: [] for k in range(8)}                    # kind -> [(key, sig, digest, msg)]
        for j, mlen in enumerate([0, 1, 55, 56, 64, 65]):
            d, q = self.keys[j % 3]
            msg = bytes(rng.randrange(256) for _ in range(mlen))
            dg = _hash(sha3, msg)
            while True:
                r, s = curve.sign(d, dg, rng.randrange(1, curve.n))
                if r and s:
                    break
            sig = po.marshal_ecdsa_signature(r, s)
            off = (q[0], q[1] ^ 1)
            assert not curve.on_curve(*off)
            other = msg + b"!"
            self.rows[VALID].append((q, sig, dg, msg))
            self.rows[BAD_MATH].append((q, sig, bytes([dg[0] ^ 1]) + dg[1:], other))
            self.rows[HIGH_S].append((q, po.marshal_ecdsa_signature(r, curve.n - s), dg, msg))
            self.rows[NON_MINIMAL].append((q, self._non_minimal(r, s), dg, msg))
            self.rows[EMPTY_SIG].append((q, b"", dg, msg))
            self.rows[OFF_CURVE].append((off, sig, dg, msg))
            self.rows[WIDE_R].append((q, po.marshal_ecdsa_signature(r + (1 << 8 * curve.width), s), dg, msg))
            self.rows[TRAILING].append((q, sig + b"\x00", dg, msg))
        self._verify, self._identity = {}, {}

    @staticmethod
    def _non_minimal(r, s):
        """r with one zero byte more in front than its minimal encoding has"""
        def der_int(v, pad):
            raw = pad + v.to_bytes((v.bit_length() + 8) // 8, "big")
            return b"\x02" + bytes([len(raw)]) + raw
        body = der_int(r, b"\x00") + der_int(s, b"")
        return b"\x30" + (bytes([len(body)]) if len(body) < 128 else b"\x81" + bytes([len(body)])) + body

    def batch(self, kinds):
        """rows of the given kinds, taking turns through the signed messages"""
        return [self.rows[k][i % 6] for i, k in enumerate(kinds)]

    def want_verify(self, row):
        key, sig, dg, _ = row
        if (key, sig, dg) not in self._verify:
            if not self.curve.on_curve(*key):                    # (these rows carry a good signature: the key is the first thing wrong)
                a = (False, "public key is not on %s: the GPU provider does not decide this tuple (use bccsp/sw)" % self.curve.name)
            else:
                valid, text = self.curve.verify(key, sig, dg)
                a = (valid, _go_text(text))
            self._verify[(key, sig, dg)] = a
        return self._verify[(key, sig, dg)]

    def want_identity(self, row, msg):
        key, sig, _, _ = row
        if (key, sig, msg) not in self._identity:
            if self.curve is P256 and not self.sha3 and self.curve.on_curve(*key):
                a = _go_text(po.identity_verify(key, msg, sig))
            else:
                valid, text = self.want_verify((key, sig, _hash(self.sha3, msg), msg))
                a = IDENT + text if text else None if valid else "The signature is invalid"
            self._identity[(key, sig, msg)] = a
        return self._identity[(key, sig, msg)]


def _cycle(kinds, n):
    return [kinds[i % len(kinds)] for i in range(n)]


def _layouts(n):
    """kind per row: the first and the last row not submitted / submitted, and at some sizes nothing / everything submitted"""
    mixed = (HIGH_S, VALID, NON_MINIMAL, BAD_MATH, EMPTY_SIG, TRAILING, OFF_CURVE, VALID, WIDE_R)
    edges_out = _cycle(mixed, n)
    edges_out[-1] = NOT_SUBMITTED[n % 5]
    edges_in = _cycle((VALID,) + mixed, n)
    edges_in[-1] = BAD_MATH if n % 2 else VALID
    out = {"edges_not_submitted": edges_out, "edges_submitted": edges_in}
    if n in (2, 65):
        out["none_submitted"] = _cycle(NOT_SUBMITTED, n)
    if n in (64, 129):
        out["all_submitted"] = _cycle(SUBMITTED, n)
    for kinds in out.values():
        assert len(kinds) == n
    assert edges_out[0] in NOT_SUBMITTED and edges_out[-1] in NOT_SUBMITTED and edges_in[0] in SUBMITTED and edges_in[-1] in SUBMITTED
    return out


@pytest.fixture(scope="module")
def rowsets():
    return {(c.name, sha3): Rows(c, sha3) for c in (P256, P384) for sha3 in (False, True)}


@pytest.fixture(scope="module")
def providers(rowsets):
    """one provider that has met no key, one that has imported every on-curve key of the rows (all_registered holds)"""
    fresh = fabgpu.GPUCSP(device=0, p384=1, hash_sha3=1)
    keyed = fabgpu.GPUCSP(device=0, p384=1, hash_sha3=1)
    for (name, _), rs in rowsets.items():
        for _, q in rs.keys:
            if name == "P-256":
                keyed.key_import(q)
            else:
                assert keyed.key_import_p384(q) == (True, "")
    yield {"fresh": fresh, "keyed": keyed}
    fresh.close()
    keyed.close()


def _verify_batch(csp, curve, rows):
    keys = [curve.provider_key(r[0]) for r in rows]
    call = csp.verify_batch if curve is P256 else csp.verify_batch_p384
    return call(keys, [r[1] for r in rows], [r[2] for r in rows])


def _identity_msgs(kinds, rows):
    return [r[3] if k in SUBMITTED else FILLER_MSGS[i % 4] for i, (k, r) in enumerate(zip(kinds, rows))]


def _identity_batch(csp, curve, rows, msgs, sha3):
    keys = [curve.provider_key(r[0]) for r in rows]
    call = csp.identity_verify_batch if curve is P256 else csp.identity_verify_batch_p384
    return call(keys, msgs, [r[1] for r in rows], hash_family="SHA3" if sha3 else "SHA2")


@pytest.mark.parametrize("mode", ["fresh", "keyed"])
@pytest.mark.parametrize("curve", [P256, P384], ids=["p256", "p384"])
def test_batches_with_rows_the_gate_does_not_submit(providers, rowsets, curve, mode):
    csp = providers[mode]
    for n in SIZES:
        for layout, kinds in _layouts(n).items():
            where = "%s n=%d %s %s" % (curve.name, n, layout, mode)
            rs = rowsets[(curve.name, False)]
            rows = rs.batch(kinds)
            got = _verify_batch(csp, curve, rows)                   # (a FabgpuError here is the infrastructure error the batch must not have)
            for i, (g, row) in enumerate(zip(got, rows)):
                assert g == rs.want_verify(row), (where, i, kinds[i], g)
            for sha3 in (False, True):
                rs = rowsets[(curve.name, sha3)]
                rows = rs.batch(kinds)
                msgs = _identity_msgs(kinds, rows)
                got = _identity_batch(csp, curve, rows, msgs, sha3)
                for i, (g, row, m) in enumerate(zip(got, rows, msgs)):
                    assert g == rs.want_identity(row, m), (where, "sha3" if sha3 else "sha2", i, kinds[i], g)
    assert not csp.poisoned()


def test_the_oracles_see_every_kind_as_meant(rowsets):
    """the rows are what their kinds say: which the gate submits, and the texts of those it does not"""
    for (name, sha3), rs in rowsets.items():
        for kind, rows in rs.rows.items():
            for row in rows:
                valid, text = rs.want_verify(row)
                assert valid == (kind in (VALID, TRAILING)), (name, kind)
                if kind in (VALID, BAD_MATH, TRAILING, WIDE_R):
                    assert text is None
                elif kind == HIGH_S:
                    assert text.startswith(WRAP + "Invalid S. Must be smaller than half the order [")
                elif kind == NON_MINIMAL:
                    assert text == WRAP + "Failed unmashalling signature [failed unmashalling signature [asn1: structure error: integer not minimally-encoded]]"
                elif kind == EMPTY_SIG:
                    assert text == "Invalid signature. Cannot be empty."
                else:
                    assert text.startswith("public key is not on " + name)


def test_coalesced_verbs_from_8_threads_equal_the_batch(providers, rowsets):
    csp = providers["fresh"]
    csp.coalescer_configure(window_us=2000, max_batch=64)
    kinds = _layouts(65)["edges_not_submitted"]
    r256, r384 = rowsets[("P-256", False)], rowsets[("P-384", False)]
    rows256, rows384 = r256.batch(kinds), r384.batch(kinds)
    msgs = _identity_msgs(kinds, rows256)
    batch256, batch384 = _verify_batch(csp, P256, rows256), _verify_batch(csp, P384, rows384)
    ident256 = _identity_batch(csp, P256, rows256, msgs, False)
    got256, got384, goti = [None] * 65, [None] * 65, [None] * 65

    def one(call, *args):
        try:
            return call(*args), None
        except fabgpu.BCCSPError as x:
            return False, str(x)

    def worker(t):
        for i in range(t, 65, 8):
            got256[i] = one(csp.verify_coalesced, P256.provider_key(rows256[i][0]), rows256[i][1], rows256[i][2])
            got384[i] = one(csp.verify_coalesced_p384, rows384[i][0], rows384[i][1], rows384[i][2])
            goti[i] = csp.identity_verify_coalesced(P256.provider_key(rows256[i][0]), msgs[i], rows256[i][1])
    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got256 == batch256 and got384 == batch384 and goti == ident256
    assert [g == r256.want_verify(row) for g, row in zip(got256, rows256)] == [True] * 65


def _c_verify(csp, entry, key, width, sig, digest):
    """(rc, valid, flags, err) of one of the three single-row C entries"""
    valid, flags = ctypes.c_int(-1), ctypes.c_int(-1)
    err = ctypes.create_string_buffer(1024)
    qx, qy = (None, None) if key is None else (key[0].to_bytes(width, "big"), key[1].to_bytes(width, "big"))
    rc = getattr(csp._L, entry)(csp._h, qx, qy, sig, len(sig), digest, len(digest), ctypes.byref(valid), ctypes.byref(flags), err, 1024)
    return rc, valid.value, flags.value, err.value.decode()


def test_c_answer_path_on_one_row_of_every_kind(providers, rowsets):
    csp = providers["fresh"]
    r256, r384 = rowsets[("P-256", False)], rowsets[("P-384", False)]
    for kind in range(8):
        row256, row384 = r256.rows[kind][1], r384.rows[kind][1]
        a = _c_verify(csp, "fabgpu_csp_verify", row256[0], 32, row256[1], row256[2])
        b = _c_verify(csp, "fabgpu_csp_verify_coalesced", row256[0], 32, row256[1], row256[2])
        c = _c_verify(csp, "fabgpu_csp_verify_coalesced_p384", row384[0], 48, row384[1], row384[2])
        assert a == b, kind
        assert a[:3] == c[:3] == (fabgpu.FABGPU_OK, int(kind in (VALID, TRAILING)), int(kind == OFF_CURVE)), kind
        # ... and with the batch of one row, which the oracle pins above
        assert (bool(a[1]), a[3] or None) == _verify_batch(csp, P256, [row256])[0] and (bool(a[1]), a[3] or None) == r256.want_verify(row256), kind
        assert (bool(c[1]), c[3] or None) == _verify_batch(csp, P384, [row384])[0] and (bool(c[1]), c[3] or None) == r384.want_verify(row384), kind
    for entry, width, rs in (("fabgpu_csp_verify", 32, r256), ("fabgpu_csp_verify_coalesced", 32, r256), ("fabgpu_csp_verify_coalesced_p384", 48, r384)):
        _, sig, dg, _ = rs.rows[VALID][0]
        assert _c_verify(csp, entry, None, width, sig, dg) == (fabgpu.FABGPU_OK, 0, 0, "Invalid Key. It must not be nil.")


def test_c_answer_path_of_a_poisoned_call(rowsets):
    rs = rowsets[("P-384", False)]
    good, bad = rs.rows[VALID][0], rs.rows[BAD_MATH][0]
    csp = fabgpu.GPUCSP(device=0, p384=1, audit_permille=1000)    # a provider of its own: poisoning is for good
    try:
        assert _c_verify(csp, "fabgpu_csp_verify_coalesced_p384", good[0], 48, good[1], good[2]) == (fabgpu.FABGPU_OK, 1, 0, "")
        fabgpu.p384_corrupt(csp, 1)                               # the device's next arithmetic reject is read as "valid": the audit must see it
        rc, valid, _, err = _c_verify(csp, "fabgpu_csp_verify_coalesced_p384", bad[0], 48, bad[1], bad[2])
        assert (rc, valid, err) == (fabgpu.FABGPU_EPOISONED, 0, POISONED)
        assert csp.poisoned()
    finally:
        csp.close()
