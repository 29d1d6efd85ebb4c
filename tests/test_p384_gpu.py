"""ECDSA P-384 on the device (csrc/p384_kernels.hip) against the Python-integer reference (p384_ref.py).

Status precedence is the P-256 gate's (p256_point.h range_status): r or s zero -> 3; otherwise s above the half order -> 2 (so s = n
reports 2, as s = n reports for P-256); otherwise r >= n -> 3; then the key: 4; then the arithmetic: 1 / 0."""
import hashlib
import random

import numpy as np
import pytest

import fabgpu
import p384_ref as R

pytestmark = pytest.mark.gpu
P, N = R.P, R.N


@pytest.fixture(scope="module")
def ctx():
    c = fabgpu.Context(device=0)
    yield c
    c.close()


_rng = random.Random(20384)
_KEYS = []
for _ in range(4):
    _d = _rng.randrange(1, N)
    _KEYS.append((_d, R.mul(_d, R.G)))


def _valid():
    d, q = _KEYS[_rng.randrange(len(_KEYS))]
    e = _rng.randrange(2**384 if _rng.random() < 0.5 else 2**256)
    while True:
        sg = R.sign(d, e, _rng.randrange(1, N))
        if sg:
            return [q[0], q[1], e, sg[0], R.low_s(sg[1])]


def _pack(tuples):
    cols = [np.frombuffer(b"".join(R.b48(t[k]) for t in tuples), dtype=np.uint8).copy() for k in range(5)]
    return cols


def _run(ctx, tuples):
    bits, st = ctx.p384_verify_batch(*_pack(tuples))
    return bits, st


def _want(tuples):
    return np.array([R.status(*t) for t in tuples], dtype=np.uint8)


@pytest.fixture(scope="module")
def mixed257():
    """257 tuples: valid ones beside tuples with one bit flipped in e, r, s, qx or qy - and their reference statuses, computed once"""
    ts = []
    for i in range(257):
        t = _valid()
        if i % 2:
            k = (2, 3, 4, 0, 1)[(i // 2) % 5]
            t[k] ^= 1 << _rng.randrange(380)
        ts.append(tuple(t))
    return ts, _want(ts)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batches_against_the_reference(ctx, mixed257, n):
    ts, want = mixed257
    bits, st = _run(ctx, ts[:n])
    assert (st == want[:n]).all(), np.nonzero(st != want[:n])
    assert (bits == (want[:n] == 0)).all()
    assert (want[:n] == 0).any() or n == 1


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_no_verdict_bit_at_or_above_n(ctx, mixed257, n):
    """all-valid batches through the _dev entry into DEVICE words pre-filled with ones, one guard word behind them: every bit below n
    set, none at or above n in the last word, the guard word (and a guard status byte) untouched"""
    import torch
    ts, want = mixed257
    all_valid = [t for t, w in zip(ts, want) if w == 0]
    batch = (all_valid * (n // len(all_valid) + 1))[:n]
    dev = [torch.from_numpy(c).cuda() for c in _pack(batch)]
    nw = (n + 63) // 64
    words = torch.full((nw + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda")
    ctx.p384_verify_batch_dev(n, *[t.data_ptr() for t in dev], words.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    w = [int(x) for x in words.cpu().numpy().view(np.uint64)]
    st = status.cpu().numpy()
    assert (st[:n] == 0).all() and st[n] == 9
    assert w[nw] == 2**64 - 1                                    # nothing written behind the last word
    assert all(x == 2**64 - 1 for x in w[:nw - 1])
    tail = n - 64 * (nw - 1)
    assert w[nw - 1] == (1 << tail) - 1                          # (tail = 64: all ones)


def test_exact_status_codes_of_the_gate(ctx):
    v = _valid()
    qx, qy, e, r, s = v
    k = 0
    while R.on_curve(qx, (qy + 1 + k) % P):
        k += 1
    cases = [
        ((qx, qy, e, r, R.HALF_N), None), ((qx, qy, e, r, R.HALF_N + 1), 2),
        ((qx, qy, e, 0, s), 3), ((qx, qy, e, r, 0), 3), ((qx, qy, e, N, s), 3), ((qx, qy, e, N - 1, s), None), ((qx, qy, e, r, N), 2),
        ((qx, qy, e, N, N), 2), ((qx, qy, e, 0, N), 3), ((qx, qy, e, 2**384 - 1, s), 3),
        ((P, qy, e, r, s), 4), ((qx, P, e, r, s), 4), ((2**384 - 1, qy, e, r, s), 4),
        ((qx, (qy + 1 + k) % P, e, r, s), 4), ((0, 0, e, r, s), 4),
        ((P, qy, e, r, R.HALF_N + 1), 2), ((P, qy, e, 0, s), 3),
        (tuple(v), 0),
    ]
    ts = [c[0] for c in cases]
    want = _want(ts)
    for (t, fixed), w in zip(cases, want):
        assert fixed is None or fixed == w, (t, fixed, w)       # the reference itself gives the code the issue names
    bits, st = _run(ctx, ts)
    assert (st == want).all(), (st, want)
    assert (bits == (want == 0)).all()


def test_exceptional_final_sums(ctx):
    """u1 G = u2 Q (the sum is a doubling), u1 G = -u2 Q (infinity), Q = G, Q = -G, u1 = 0"""
    ts = []
    # Q = d G.  u1 G = u2 Q <=> u1 = u2 d.  Choose r, s freely (low s), then e = u1 s = r d (mod n): u1 = r w d, u2 = r w.
    d = _rng.randrange(2, N)
    q = R.mul(d, R.G)
    for sign_ in (1, -1):
        s = _rng.randrange(1, R.HALF_N)
        w = pow(s, -1, N)
        # r must equal x(2 u1 G) mod n for "valid": take any r and let the device reject or accept as the reference says
        r = _rng.randrange(1, N)
        e = sign_ * r * d % N
        u1, u2 = e * w % N, r * w % N
        assert R.mul(u1, R.G) == (R.mul(u2, q) if sign_ == 1 else R.neg(R.mul(u2, q)))
        ts.append((q[0], q[1], e, r, s))
        if sign_ == 1:
            # ... and one that VERIFIES through the doubling: r = x(2 u1 G) mod n needs u1 = r w d: fixed point search over k: R = k G,
            # r = x(R); 2 u1 = k, u2 = u1 / d -> s = r / u2, e = u1 s
            while True:
                kk = _rng.randrange(1, N)
                r2 = R.mul(kk, R.G)[0] % N
                u1b = kk * pow(2, -1, N) % N
                u2b = u1b * pow(d, -1, N) % N
                s2 = r2 * pow(u2b, -1, N) % N
                if 0 < s2 <= R.HALF_N and r2:
                    break
            e2 = u1b * s2 % N
            ts.append((q[0], q[1], e2, r2, s2))
            assert R.status(*ts[-1]) == 0
    for qq in (R.G, R.neg(R.G)):
        for _ in range(2):
            dd = 1 if qq == R.G else N - 1
            e = _rng.randrange(2**384)
            sg = R.sign(dd, e, _rng.randrange(1, N))
            ts.append((qq[0], qq[1], e, sg[0], R.low_s(sg[1])))
            assert R.status(*ts[-1]) == 0
        # Q = +-G with u1 = +-u2: e = +-r
        r = _rng.randrange(1, N)
        ts.append((qq[0], qq[1], r, r, _rng.randrange(1, R.HALF_N)))
        ts.append((qq[0], qq[1], N - r, r, _rng.randrange(1, R.HALF_N)))
    # u1 = 0: e = 0 and e = n (e = 0 mod n); valid when r = x(u2 Q): R = k G, r = x(R), u2 = k / d, s = r / u2
    for e in (0, N):
        while True:
            kk = _rng.randrange(1, N)
            r = R.mul(kk, R.G)[0] % N
            s = r * pow(kk * pow(d, -1, N) % N, -1, N) % N
            if 0 < s <= R.HALF_N:
                break
        ts.append((q[0], q[1], e, r, s))
        assert R.status(*ts[-1]) == 0
        ts.append((q[0], q[1], e, r, s - 1 or 1))
    want = _want(ts)
    assert (want == 0).sum() >= 7 and (want == 1).sum() >= 4
    bits, st = _run(ctx, ts)
    assert (st == want).all(), (st, want)
    assert (bits == (want == 0)).all()


def test_second_acceptance_branch(ctx):
    """x(R) = n + k < p: r = x - n must verify, r = x - n + 1 must not"""
    ts = []
    k = 1                                    # (k = 0 would be r = 0)
    for _ in range(3):
        while R.lift_x(N + k) is None:
            k += 1
        Rp = R.lift_x(N + k)
        x = N + k
        k += 1
        s = _rng.randrange(1, R.HALF_N)
        e = _rng.randrange(2**384)
        r = x - N
        w = pow(s, -1, N)
        u1, u2 = e * w % N, r * w % N
        q = R.mul(pow(u2, -1, N), R.add(Rp, R.neg(R.mul(u1, R.G))))      # Q = u2^-1 (R - u1 G)
        assert R.on_curve(*q) and r + N < P
        ts.append((q[0], q[1], e, r, s))
        ts.append((q[0], q[1], e, r + 1, s))
    want = _want(ts)
    assert list(want) == [0, 1] * 3
    bits, st = _run(ctx, ts)
    assert (st == want).all(), (st, want)
    assert (bits == (want == 0)).all()


@pytest.mark.parametrize("sha3", [False, True])
def test_hash_then_verify_at_the_block_edges(ctx, sha3):
    n = 65
    lens = [0, 55, 56, 135, 136, 1856]
    hf = hashlib.sha3_256 if sha3 else hashlib.sha256
    msgs, ts = [], []
    for i in range(n):
        m = bytes(_rng.randrange(256) for _ in range(lens[i % len(lens)]))
        d, q = _KEYS[i % len(_KEYS)]
        e = R.hash_to_int(hf(m).digest())
        assert e < 2**256
        sg = R.sign(d, e, _rng.randrange(1, N))
        r, s = sg[0], R.low_s(sg[1])
        if i % 4 == 3:
            m = m + b"x" if i % 8 == 3 else m                 # another message, or another r
            r = r if i % 8 == 3 else r ^ 2
            e = R.hash_to_int(hf(m).digest())
        msgs.append(m)
        ts.append((q[0], q[1], e, r, s))
    want = _want(ts)
    assert (want == 0).sum() >= 40 and (want != 0).sum() >= 10
    arena = np.frombuffer(b"".join(msgs) + bytes(8), dtype=np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)
    qx, qy, _, r, s = _pack(ts)
    bits, st = ctx.hash_p384_verify_batch(arena, off, qx, qy, r, s, sha3=sha3)
    assert (st == want).all(), (st, want)
    assert (bits == (want == 0)).all()


def test_host_pointer_and_dev_calls_give_identical_bytes(ctx, mixed257):
    import torch
    ts, want = mixed257
    n = 193
    cols = _pack(ts[:n])
    bits, st = ctx.p384_verify_batch(*cols)
    dev = [torch.from_numpy(c).cuda() for c in cols]
    words = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    status = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    ctx.p384_verify_batch_dev(n, *[t.data_ptr() for t in dev], words.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == st).all() and (st == want[:n]).all()
    assert (fabgpu.unpack_bits(words.cpu().numpy().view(np.uint64), n) == bits).all()
    assert words.cpu().numpy().view(np.uint64).tobytes() == np.packbits(np.concatenate([bits, np.zeros(-n % 64, bool)]), bitorder="little").tobytes()
    # the hash-then-verify pair as well
    msgs = [bytes([i & 255]) * (i % 140) for i in range(n)]
    arena = np.frombuffer(b"".join(msgs) + bytes(64), dtype=np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)
    hb, hs = ctx.hash_p384_verify_batch(arena, off, cols[0], cols[1], cols[3], cols[4])
    ta, to = torch.from_numpy(arena).cuda(), torch.from_numpy(off.view(np.int32)).cuda()
    words.zero_()
    status.fill_(9)
    ctx.hash_p384_verify_batch_dev(n, ta.data_ptr(), ta.numel(), to.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[3].data_ptr(),
                                   dev[4].data_ptr(), words.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == hs).all()
    assert (fabgpu.unpack_bits(words.cpu().numpy().view(np.uint64), n) == hb).all()
    assert set(np.unique(hs)) <= {1, 2, 3, 4}          # none of these signatures is over these messages


# ---- the provider layer (option p384) ----
@pytest.fixture(scope="module")
def provider_cases():
    """(key, DER signature, digest, message, expected valid) for SHA-256 digests: valid ones beside changed digests, high S, r = n"""
    cases = []
    for i in range(40):
        d, q = _KEYS[i % len(_KEYS)]
        msg = b"p384 provider %d" % i
        dg = hashlib.sha256(msg).digest()
        sg = R.sign(d, R.hash_to_int(dg), _rng.randrange(1, N))
        r, s = sg[0], R.low_s(sg[1])
        kind = i % 5
        if kind == 1:
            dg = hashlib.sha256(msg + b"!").digest()
        elif kind == 2:
            r ^= 4
        elif kind == 3 and i % 2:
            s = N - s
        cases.append((q, R.der_sig(r, s), dg, msg, R.status(q[0], q[1], R.hash_to_int(dg), r, s)))
    return cases


def test_provider_refuses_while_the_option_is_off(provider_cases):
    csp = fabgpu.GPUCSP(device=0)
    try:
        text = fabgpu.load_hooks().fabgpu_test_p384_refusal_text().decode()
        assert text == "P-384 is served by bccsp/sw, not by the GPU provider"
        q, sig, dg, msg, _ = provider_cases[0]
        assert csp.get_option("p384") == 0
        assert csp.verify_batch_p384([q], [sig], [dg]) == [(False, text)]
        assert csp.identity_verify_batch_p384([q], [msg], [sig]) == ["could not determine the validity of the signature: " + text]
        with pytest.raises(fabgpu.BCCSPError, match="P-384 is served by bccsp/sw"):
            csp.verify_coalesced_p384(q, sig, dg)
        csp.set_option("p384", 1)
        assert csp.verify_batch_p384([q], [sig], [dg]) == [(True, None)]
    finally:
        csp.close()


def test_provider_batch_answers_and_texts(provider_cases):
    csp = fabgpu.GPUCSP(device=0, p384=1, hash_sha3=1)
    try:
        keys, sigs, dgs, msgs, want = zip(*provider_cases)
        got = csp.verify_batch_p384(keys, sigs, dgs)
        for (valid, err), w in zip(got, want):
            assert valid == (w == 0)
            if w == 2:
                assert err.startswith("Failed verifing with opts [<nil>]: Invalid S. Must be smaller than half the order [") and str(R.HALF_N) in err
            else:
                assert err is None
        assert any(w == 2 for w in want) and any(w == 1 for w in want) and sum(w == 0 for w in want) >= 16
        # identity.Verify: the message is hashed on the device in the MSP's family
        ident = csp.identity_verify_batch_p384(keys, msgs, sigs)
        for k, (e, w, c) in enumerate(zip(ident, want, provider_cases)):
            if k % 5 == 1:
                assert e is None                                 # (the signature IS over this message; only the digest of the case was changed)
            elif w == 0:
                assert e is None
            elif w == 2:
                assert e.startswith("could not determine the validity of the signature: Failed verifing with opts [<nil>]: Invalid S.")
            else:
                assert e == "The signature is invalid"
        # SHA3 family: signatures over SHA3-256 digests
        d, q = _KEYS[0]
        m3 = [b"sha3 family %d" % i for i in range(5)]
        s3 = []
        for i, m in enumerate(m3):
            sg = R.sign(d, R.hash_to_int(hashlib.sha3_256(m).digest()), _rng.randrange(1, N))
            s3.append(R.der_sig(sg[0], R.low_s(sg[1])))
        assert csp.identity_verify_batch_p384([q] * 5, m3, s3, hash_family="SHA3") == [None] * 5
        assert csp.identity_verify_batch_p384([q] * 5, m3, s3, hash_family="SHA2") == ["The signature is invalid"] * 5
        assert csp.identity_verify_batch_p384([q], m3[:1], s3[:1], hash_family="MD5") == ["hash familiy not recognized [MD5]"]
        # an off-curve key, an empty digest, a signature that is no DER
        bad = csp.verify_batch_p384([(q[0], q[1] ^ 1), q, q], [sigs[0], sigs[0], b"\x30\x03\x02\x01"], [dgs[0], b"", dgs[0]])
        assert bad[0] == (False, "public key is not on P-384: the GPU provider does not decide this tuple (use bccsp/sw)")
        assert bad[1] == (False, "Invalid digest. Cannot be empty.")
        assert bad[2][0] is False and bad[2][1].startswith("Failed verifing with opts [<nil>]: Failed unmashalling signature [")
    finally:
        csp.close()


def test_coalesced_entry_from_16_threads_equals_the_batch_entry(provider_cases):
    import threading
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        csp.coalescer_configure(window_us=2000, max_batch=64)
        keys, sigs, dgs, msgs, want = zip(*provider_cases)
        batch = csp.verify_batch_p384(keys, sigs, dgs)
        got = [None] * len(provider_cases)

        def worker(t):
            for i in range(t, len(provider_cases), 16):
                try:
                    got[i] = (csp.verify_coalesced_p384(keys[i], sigs[i], dgs[i]), None)
                except fabgpu.BCCSPError as x:
                    got[i] = (False, str(x))
        th = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert got == batch
        cs = csp.coalescer_stats()                       # (high-S items are decided on the caller's thread: they never queue)
        assert cs["calls"] == sum(1 for w in want if w != 2) and cs["launches"] < cs["calls"] and cs["largest_batch"] > 1
    finally:
        csp.close()


def test_audit_poisons_on_a_corrupted_valid(provider_cases):
    keys, sigs, dgs, msgs, want = zip(*provider_cases)
    bad = [i for i, w in enumerate(want) if w == 1][0]
    good = [i for i, w in enumerate(want) if w == 0][0]
    # without the audit the corruption goes through: the hook works
    csp = fabgpu.GPUCSP(device=0, p384=1)
    try:
        fabgpu.p384_corrupt(csp, 1)
        assert csp.verify_batch_p384([keys[bad]], [sigs[bad]], [dgs[bad]]) == [(True, None)]
        assert csp.verify_batch_p384([keys[bad]], [sigs[bad]], [dgs[bad]]) == [(False, None)]
        assert not csp.poisoned()
    finally:
        csp.close()
    csp = fabgpu.GPUCSP(device=0, p384=1, audit_permille=1000)
    try:
        assert csp.verify_batch_p384([keys[good]], [sigs[good]], [dgs[good]]) == [(True, None)]      # an honest "valid" passes the audit
        assert csp.identity_verify_batch_p384([keys[good]], [msgs[good]], [sigs[good]]) == [None]
        assert not csp.poisoned()
        fabgpu.p384_corrupt(csp, 1)
        with pytest.raises(fabgpu.PoisonedError):
            csp.verify_batch_p384([keys[bad]], [sigs[bad]], [dgs[bad]])
        assert csp.poisoned()
        with pytest.raises(fabgpu.PoisonedError):
            csp.verify_coalesced_p384(keys[good], sigs[good], dgs[good])
    finally:
        csp.close()
