"""ECDSA P-384 verification with Python integers: the reference the P-384 tests compare the device and the host compilation against.

Shares no code with csrc/.  Field, group law (affine, with the point at infinity as None), Go 1.14's hashToInt for a 384-bit order, and
the status precedence of the C ABI (fabgpu.h): 4 key not on the curve (coordinates >= p included) after 3 (r or s zero or >= n) and
2 (s above the half order), 1 arithmetic reject, 0 valid.  tests/test_p384_host.py pins this file against openssl.
"""
P = 2**384 - 2**128 - 2**96 + 2**32 - 1
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFC7634D81F4372DDF581A0DB248B0A77AECEC196ACCC52973
A = P - 3
B = 0xB3312FA7E23EE7E4988E056BE3F82D19181D9C6EFE8141120314088F5013875AC656398D8A2ED19D2A85C8EDD3EC2AEF
GX = 0xAA87CA22BE8B05378EB1C71EF320AD746E1D3B628BA79B9859F741E082542A385502F25DBF55296C3A545E3872760AB7
GY = 0x3617DE4A96262C6F5D9E98BF9292DC29F8F41DBD289A147CE9DA3113B5F0B8C00A60B1CE1D7E819D7A431D7C90EA0E5F
G = (GX, GY)
HALF_N = N >> 1

ST_VALID, ST_BAD_MATH, ST_HIGH_S, ST_RANGE, ST_OFF_CURVE = 0, 1, 2, 3, 4


def on_curve(x, y):
    return 0 <= x < P and 0 <= y < P and (y * y - (x * x * x + A * x + B)) % P == 0


def neg(p):
    return None if p is None else (p[0], (-p[1]) % P)


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % P == 0:
            return None
        lam = (3 * p[0] * p[0] + A) * pow(2 * p[1], -1, P) % P
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return (x, (lam * (p[0] - x) - p[1]) % P)


def mul(k, p):
    k %= N
    acc = None
    while k:
        if k & 1:
            acc = add(acc, p)
        p = add(p, p)
        k >>= 1
    return acc


def sqrt_mod_p(v):
    """p = 3 mod 4: the root, or None."""
    r = pow(v, (P + 1) // 4, P)
    return r if r * r % P == v % P else None


def lift_x(x):
    y = sqrt_mod_p((x * x * x + A * x + B) % P)
    return None if y is None else (x, y)


def hash_to_int(digest: bytes) -> int:
    """Go 1.14 crypto/ecdsa hashToInt, order of 384 bits: at most the leftmost 48 bytes, no shift."""
    return int.from_bytes(digest[:48], "big")


def verify_math(q, e, r, s) -> bool:
    """ecdsa.Verify's arithmetic on an on-curve key, r and s in [1, n)."""
    w = pow(s, -1, N)
    u1, u2 = e * w % N, r * w % N
    pt = add(mul(u1, G), mul(u2, q))
    return pt is not None and pt[0] % N == r


def status(qx, qy, e, r, s) -> int:
    if r == 0 or s == 0:
        return ST_RANGE
    if s > HALF_N:
        return ST_HIGH_S
    if r >= N:
        return ST_RANGE
    if not on_curve(qx, qy):
        return ST_OFF_CURVE
    return ST_VALID if verify_math((qx, qy), e, r, s) else ST_BAD_MATH


def sign(d, e, k):
    """(r, s) with s as produced (not normalised), or None when r or s is zero."""
    r = mul(k, G)[0] % N
    s = pow(k, -1, N) * (e + r * d) % N
    return (r, s) if r and s else None


def low_s(s):
    return s if s <= HALF_N else N - s


def b48(v: int) -> bytes:
    return v.to_bytes(48, "big")


def _der_int(v):
    raw = v.to_bytes((v.bit_length() + 8) // 8 or 1, "big")
    return b"\x02" + bytes([len(raw)]) + raw


def der_sig(r, s) -> bytes:
    """SEQUENCE { INTEGER r, INTEGER s }, minimal."""
    body = _der_int(r) + _der_int(s)
    return b"\x30" + (bytes([len(body)]) if len(body) < 128 else b"\x81" + bytes([len(body)])) + body
