#!/usr/bin/env python3
"""SHA3-256 with 32 lanes on a message (FABGPU_FLAG_SHA3_COOP) against the one-lane kernels, one process: two contexts, flag on and flag
off, the same HBM-resident messages of 1 856 bytes (the size tools/bench_sha3.py uses), the _dev entry points on torch's stream.

  hash_only   n = 64 .. 8 192: fabgpu_sha3_256_batch_dev on both contexts, and the 32-lane kernel alone at every n through the test hook
              (above SHA3_COOP_MAX the flag-on context takes the mixed road, which is the one-lane kernel for messages of one size) -
              the `coop_kernel` column is what places SHA3_COOP_MAX: the largest power of two at which its median is not above the
              flag-off median;
  hash_verify n = 400, 3 000: fabgpu_sha3_256_p256_verify_batch_dev, fresh keys;
  mixed       30 000 messages, with and without one message of 1 MiB among them, on both contexts: the flag-on launch with the long
              message against the launches without it.

After a clock warm-up, ROUNDS interleaved rounds per leg (who goes first alternates), each timed by events over LAUNCHES back-to-back
calls; digests and verdicts of both contexts are checked against hashlib after the timed region.  Writes profiles/sha3_coop.json (or the
path given as the first argument) and prints the same JSON line."""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-mod_amd"))
import ctypes  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fabgpu  # noqa: E402

ROUNDS = int(os.environ.get("SHA3_COOP_ROUNDS", "10"))
LAUNCHES = 4
MSG = 1856
SIZES = [64, 256, 1024, 2048, 4096, 8192]
VERIFY_SIZES = [400, 3000]
MIXED_N, LONG = 30000, 1 << 20
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sha3_coop.json")

torch.cuda.set_device(0)
stream = torch.cuda.current_stream()
hooks = fabgpu.load_hooks()
hooks.fabgpu_test_sha3_coop_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p]
ctxs = {"coop": fabgpu.Context(device=0, flags=fabgpu.FLAG_SHA3_COOP), "one_lane": fabgpu.Context(device=0)}
rng = np.random.default_rng(1856)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def timed(calls):
    """calls: {name: f()} -> {name: [ms per call, one per round]}, interleaved, after a warm-up of two seconds"""
    t_end = time.time() + 2.0
    while time.time() < t_end:
        for f in calls.values():
            f()
        torch.cuda.synchronize()
    per = {k: [] for k in calls}
    names = list(calls)
    for i in range(ROUNDS):
        for k in (names if i % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(LAUNCHES):
                calls[k]()
            e1.record(stream)
            e1.synchronize()
            per[k].append(e0.elapsed_time(e1) / LAUNCHES)
    torch.cuda.synchronize()
    return per


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v}


def digests_of(arena, off):
    return np.frombuffer(b"".join(hashlib.sha3_256(arena[off[i]:off[i + 1]].tobytes()).digest() for i in range(len(off) - 1)), dtype=np.uint8)


out = {"rounds": ROUNDS, "launches_per_round": LAUNCHES, "message_bytes": MSG, "sha3_coop_max": 4096, "hash_only": {}, "hash_verify": {}, "mixed": {}}

# ---- hash only ----
for n in SIZES:
    off = (np.arange(n + 1, dtype=np.uint64) * MSG).astype(np.uint32)
    arena = rng.integers(0, 256, size=n * MSG, dtype=np.uint8)
    d_arena, d_off = up(arena), up(off)
    res = {k: torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for k in ("coop", "one_lane", "coop_kernel")}
    calls = {k: (lambda k=k: ctxs[k].sha3_256_batch_dev(n, d_arena.data_ptr(), arena.size, d_off.data_ptr(), res[k].data_ptr(), stream.cuda_stream))
             for k in ("coop", "one_lane")}

    def kernel_alone():
        rc = hooks.fabgpu_test_sha3_coop_batch_dev(ctxs["coop"]._h, n, d_arena.data_ptr(), arena.size, d_off.data_ptr(), res["coop_kernel"].data_ptr(),
                                                   stream.cuda_stream)
        assert rc == 0, rc
    calls["coop_kernel"] = kernel_alone
    per = timed(calls)
    want = digests_of(arena, off)
    for k, t in res.items():
        assert (t.cpu().numpy() == want).all(), (k, n)
    row = {k: summary(v) for k, v in per.items()}
    row["one_lane_over_coop_kernel_median"] = statistics.median([a / c for a, c in zip(per["one_lane"], per["coop_kernel"])])
    row["one_lane_over_coop_median"] = statistics.median([a / c for a, c in zip(per["one_lane"], per["coop"])])
    out["hash_only"][str(n)] = row

# ---- hash -> fresh-key verify ----
for n in VERIFY_SIZES:
    off = (np.arange(n + 1, dtype=np.uint64) * MSG).astype(np.uint32)
    arena = rng.integers(0, 256, size=n * MSG, dtype=np.uint8)
    dig = digests_of(arena, off).reshape(n, 32)
    b = fabgpu.synth_batch(n, seed=n, invalid_permille=0, e_in=dig)
    t = {k: up(v) for k, v in dict(arena=arena, off=off, qx=b["qx"], qy=b["qy"], r=b["r"], s=b["s"]).items()}
    res = {k: (torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda"), torch.ones(n, dtype=torch.uint8, device="cuda")) for k in ctxs}
    calls = {k: (lambda k=k: ctxs[k].sha3_256_p256_verify_batch_dev(n, t["arena"].data_ptr(), arena.size, t["off"].data_ptr(), t["qx"].data_ptr(),
                                                                     t["qy"].data_ptr(), t["r"].data_ptr(), t["s"].data_ptr(), res[k][0].data_ptr(),
                                                                     res[k][1].data_ptr(), stream.cuda_stream)) for k in ctxs}
    per = timed(calls)
    for k, (words, status) in res.items():
        assert (status.cpu().numpy() == 0).all() and fabgpu.unpack_bits(words.cpu().numpy().view(np.uint64), n).all(), (k, n)
    row = {k: summary(v) for k, v in per.items()}
    row["one_lane_over_coop_median"] = statistics.median([a / c for a, c in zip(per["one_lane"], per["coop"])])
    out["hash_verify"][str(n)] = row

# ---- the mixed road ----
lens = np.full(MIXED_N, MSG, dtype=np.uint64)
legs = {}
for name, long_at in (("plain", None), ("one_long", MIXED_N // 2 + 11)):
    ln = lens.copy()
    if long_at is not None:
        ln[long_at] = LONG
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)
    arena = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    legs[name] = dict(off=off, arena=arena, d_arena=up(arena), d_off=up(off), long_at=long_at,
                      res={k: torch.zeros(32 * MIXED_N, dtype=torch.uint8, device="cuda") for k in ctxs})
calls = {}
for name, leg in legs.items():
    for k in ctxs:
        calls["%s/%s" % (name, k)] = (lambda leg=leg, k=k: ctxs[k].sha3_256_batch_dev(MIXED_N, leg["d_arena"].data_ptr(), leg["arena"].size,
                                                                                       leg["d_off"].data_ptr(), leg["res"][k].data_ptr(), stream.cuda_stream))
rows_before = ctxs["coop"].sha3_coop_rows()
per = timed(calls)
assert ctxs["coop"].sha3_coop_rows() > rows_before and ctxs["one_lane"].sha3_coop_rows() == 0
for name, leg in legs.items():
    sample = sorted(set(range(0, MIXED_N, 997)) | ({leg["long_at"]} if leg["long_at"] is not None else set()))
    for k in ctxs:
        got = leg["res"][k].cpu().numpy().reshape(-1, 32)
        for i in sample:
            assert got[i].tobytes() == hashlib.sha3_256(leg["arena"][leg["off"][i]:leg["off"][i + 1]].tobytes()).digest(), (name, k, i)
        assert (got == leg["res"]["coop"].cpu().numpy().reshape(-1, 32)).all()
out["mixed"] = {k: summary(v) for k, v in per.items()}
out["mixed"]["n"], out["mixed"]["long_bytes"] = MIXED_N, LONG
out["mixed"]["one_long_coop_over_plain_coop_median"] = statistics.median([a / c for a, c in zip(per["one_long/coop"], per["plain/coop"])])
out["mixed"]["one_long_one_lane_over_plain_one_lane_median"] = statistics.median([a / c for a, c in zip(per["one_long/one_lane"], per["plain/one_lane"])])
out["mixed"]["one_long_one_lane_over_one_long_coop_median"] = statistics.median([a / c for a, c in zip(per["one_long/one_lane"], per["one_long/coop"])])
out["mixed"]["plain_one_lane_over_plain_coop_median"] = statistics.median([a / c for a, c in zip(per["plain/one_lane"], per["plain/coop"])])

for c in ctxs.values():
    c.close()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
