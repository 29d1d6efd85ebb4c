#!/usr/bin/env python3
"""ECDSA P-384 verification on the device against two baselines, one process: fabgpu_p384_verify_batch_dev on HBM-resident inputs
against (a) the one-lane P-256 kernel (a context with FABGPU_FLAG_ONE_LANE_ONLY, fabgpu_p256_verify_batch_dev) on the same n and
(b) libcrypto's ECDSA_do_verify on P-384 on 16 threads over the same tuples.  n = 3 000 and 30 000 fresh-key tuples.

The P-384 tuples are 256 signatures made with Python integers (tests/p384_ref.py) over 32 keys, repeated to n - the kernel's control flow
does not depend on the operands, so a repeated tuple costs what a distinct one costs - with every 97th tuple's r changed afterwards;
the verdicts are checked against exactly that after the timed region.  After a clock warm-up, ROUNDS interleaved rounds (p384, p256,
p384, ...), each timed by events over back-to-back launches.  Writes profiles/p384_batch.json and prints the same JSON line."""
import ctypes
import ctypes.util
import json
import os
import random
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-mod_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fabgpu  # noqa: E402
import p384_ref as R  # noqa: E402

ROUNDS = int(os.environ.get("P384_ROUNDS", "6"))
SIZES = [int(x) for x in os.environ.get("P384_SIZES", "3000,30000").split(",")]
LAUNCHES = {"p384": 2, "p256": 10}
CPU_THREADS = 16
torch.cuda.set_device(0)
stream = torch.cuda.current_stream()
ctx = fabgpu.Context(device=0)
ctx1 = fabgpu.Context(device=0, flags=fabgpu.FLAG_ONE_LANE_ONLY)
fabgpu.load_hooks()

rng = random.Random(384)
keys = []
for _ in range(32):
    d = rng.randrange(1, R.N)
    keys.append((d, R.mul(d, R.G)))
base = []
for i in range(256):
    d, q = keys[i % 32]
    e = rng.randrange(2**256)
    r, s = R.sign(d, e, rng.randrange(1, R.N))
    base.append((q[0], q[1], e, r, R.low_s(s)))


def cpu_verify_seconds(tuples):
    """libcrypto ECDSA_do_verify(P-384) over the tuples on CPU_THREADS threads (ctypes drops the GIL in the calls): wall seconds"""
    C = ctypes.CDLL(ctypes.util.find_library("crypto"))
    vp = ctypes.c_void_p
    for f in ("EC_KEY_new_by_curve_name", "BN_bin2bn", "ECDSA_SIG_new", "BN_new"):
        getattr(C, f).restype = vp
    C.EC_KEY_set_public_key_affine_coordinates.argtypes = [vp, vp, vp]
    C.ECDSA_SIG_set0.argtypes = [vp, vp, vp]
    C.ECDSA_do_verify.argtypes = [ctypes.c_char_p, ctypes.c_int, vp, vp]
    C.BN_bin2bn.argtypes = [ctypes.c_char_p, ctypes.c_int, vp]
    NID_secp384r1 = 715
    items = []
    for qx, qy, e, r, s in tuples:
        k = C.EC_KEY_new_by_curve_name(NID_secp384r1)
        assert C.EC_KEY_set_public_key_affine_coordinates(k, C.BN_bin2bn(R.b48(qx), 48, None), C.BN_bin2bn(R.b48(qy), 48, None)) == 1
        sg = C.ECDSA_SIG_new()
        C.ECDSA_SIG_set0(sg, C.BN_bin2bn(R.b48(r), 48, None), C.BN_bin2bn(R.b48(s), 48, None))
        items.append((R.b48(e)[16:], k, sg))          # e < 2^256: the 32-byte digest itself
    n_ok = [0] * CPU_THREADS

    def work(t):
        for dg, k, sg in items[t::CPU_THREADS]:
            n_ok[t] += C.ECDSA_do_verify(dg, 32, sg, k) == 1
    th = [threading.Thread(target=work, args=(t,)) for t in range(CPU_THREADS)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    return time.perf_counter() - t0, sum(n_ok)


out = {"rounds": ROUNDS, "launches_per_round": LAUNCHES, "cpu_threads": CPU_THREADS}
for n in SIZES:
    tuples = [base[i % 256] for i in range(n)]
    truth = np.ones(n, bool)
    for i in range(0, n, 97):
        t = list(tuples[i])
        t[3] ^= 2
        tuples[i] = tuple(t)
        truth[i] = False
    cols = [torch.from_numpy(np.frombuffer(b"".join(R.b48(t[k]) for t in tuples), dtype=np.uint8).copy()).cuda() for k in range(5)]
    words = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    b = fabgpu.synth_batch(n, seed=384, invalid_permille=10)
    c256 = [torch.from_numpy(b[k]).cuda() for k in ("qx", "qy", "e", "r", "s")]
    words256 = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    status256 = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def p384():
        ctx.p384_verify_batch_dev(n, *[c.data_ptr() for c in cols], words.data_ptr(), status.data_ptr(), stream.cuda_stream)

    def p256():
        ctx1.p256_verify_batch_dev(n, *[c.data_ptr() for c in c256], words256.data_ptr(), status256.data_ptr(), stream.cuda_stream)
    calls = {"p384": p384, "p256": p256}
    t_end = time.time() + 2.0        # clock warm-up
    while time.time() < t_end:
        p384()
        p256()
        torch.cuda.synchronize()
    per = {f: [] for f in calls}
    for _ in range(ROUNDS):
        for f, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(LAUNCHES[f]):
                call()
            e1.record(stream)
            e1.synchronize()
            per[f].append(e0.elapsed_time(e1) / LAUNCHES[f])
    torch.cuda.synchronize()
    got = fabgpu.unpack_bits(words.cpu().numpy().view(np.uint64), n)
    assert (got == truth).all() and ((status.cpu().numpy() == 0) == truth).all(), n
    assert ((status256.cpu().numpy() == 0).sum()) > n * 0.9
    row = {f: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for f, v in per.items()}
    ratios = [a / c for a, c in zip(per["p384"], per["p256"])]
    row["p384_over_p256_one_lane_median"] = statistics.median(ratios)
    row["p384_over_p256_one_lane_min"], row["p384_over_p256_one_lane_max"] = min(ratios), max(ratios)
    row["p384_verifies_per_s"] = n / (row["p384"]["median_ms"] * 1e-3)
    cpu_s, cpu_ok = cpu_verify_seconds(tuples)
    assert cpu_ok == int(truth.sum()), (cpu_ok, int(truth.sum()))
    row["libcrypto_16_threads_ms"] = cpu_s * 1e3
    row["libcrypto_over_device"] = cpu_s * 1e3 / row["p384"]["median_ms"]
    out[str(n)] = row
ctx.close()
ctx1.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "p384_batch.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
