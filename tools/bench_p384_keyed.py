#!/usr/bin/env python3
"""Registered-key P-384 verification against the fresh-key launch, one process: fabgpu_p384_verify_batch_keyed_dev against
fabgpu_p384_verify_batch_dev on the same HBM-resident tuples, n = 3 000 and 30 000, signed by 16 distinct registered keys.

The tuples are 256 signatures made with Python integers (tests/p384_ref.py), repeated to n - the kernels' control flow does not depend
on the operands - with every 97th tuple's r changed afterwards; both launches' verdicts are checked against exactly that after the timed
region.  After a clock warm-up, ROUNDS interleaved rounds (keyed, fresh, keyed, ...), each timed by events over back-to-back launches.
Also recorded: the one-off build of the generator's comb (the warm call of a new context), and the wall time of registering a batch of
1 and of 16 keys (one device build each).  Writes profiles/p384_keyed.json and prints the same JSON line."""
import json
import os
import random
import statistics
import sys
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
LAUNCHES = 2
N_KEYS = 16
torch.cuda.set_device(0)
stream = torch.cuda.current_stream()
fabgpu.load_hooks()

rng = random.Random(384016)
keys = []
for _ in range(N_KEYS + 1):
    d = rng.randrange(1, R.N)
    keys.append((d, R.mul(d, R.G)))
base = []
for i in range(256):
    d, q = keys[i % N_KEYS]
    e = rng.randrange(2**256)
    r, s = R.sign(d, e, rng.randrange(1, R.N))
    base.append((i % N_KEYS, q[0], q[1], e, r, R.low_s(s)))

out = {"rounds": ROUNDS, "launches_per_round": LAUNCHES, "keys": N_KEYS}
ctx = fabgpu.Context(device=0)
ctx.p384_verify_batch_dev(0, None, None, None, None, None, None, None)          # the fresh-key road's warm call (not timed)
t0 = time.perf_counter()
ctx.p384_verify_batch_keyed_dev(0, None, None, None, None, None, None)          # the keyed road's: the generator's comb
out["generator_comb_build_ms"] = (time.perf_counter() - t0) * 1e3
pairs = [(R.b48(q[0]), R.b48(q[1])) for _d, q in keys]
t0 = time.perf_counter()
extra = fabgpu.p384_key_register_batch(ctx, pairs[N_KEYS:])                      # a batch of one (the first build sizes the builder's room)
out["register_1_key_first_ms"] = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
ids = fabgpu.p384_key_register_batch(ctx, pairs[:N_KEYS])
out["register_16_keys_ms"] = (time.perf_counter() - t0) * 1e3
assert ctx.p384_key_unregister(extra[0])
t0 = time.perf_counter()
again = ctx.p384_key_register(*pairs[N_KEYS])                                    # a batch of one once more: the room and a table are there
out["register_1_key_ms"] = (time.perf_counter() - t0) * 1e3
assert again == (1 << 12 | extra[0]) and ids == list(range(1, N_KEYS + 1))
out["key_table_stats"] = ctx.p384_key_table_stats()

for n in SIZES:
    tuples = [base[i % 256] for i in range(n)]
    truth = np.ones(n, bool)
    for i in range(0, n, 97):
        t = list(tuples[i])
        t[4] ^= 2
        tuples[i] = tuple(t)
        truth[i] = False
    cols = [torch.from_numpy(np.frombuffer(b"".join(R.b48(t[k]) for t in tuples), dtype=np.uint8).copy()).cuda() for k in range(1, 6)]
    kid = torch.from_numpy(np.array([ids[t[0]] for t in tuples], dtype=np.uint32).view(np.int32)).cuda()
    res = {f: (torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")) for f in ("keyed", "fresh")}

    def keyed():
        ctx.p384_verify_batch_keyed_dev(n, kid.data_ptr(), *[c.data_ptr() for c in cols[2:]], res["keyed"][0].data_ptr(), res["keyed"][1].data_ptr(),
                                        stream.cuda_stream)

    def fresh():
        ctx.p384_verify_batch_dev(n, *[c.data_ptr() for c in cols], res["fresh"][0].data_ptr(), res["fresh"][1].data_ptr(), stream.cuda_stream)
    calls = {"keyed": keyed, "fresh": fresh}
    t_end = time.time() + 2.0        # clock warm-up
    while time.time() < t_end:
        keyed()
        fresh()
        torch.cuda.synchronize()
    per = {f: [] for f in calls}
    for _ in range(ROUNDS):
        for f, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(LAUNCHES):
                call()
            e1.record(stream)
            e1.synchronize()
            per[f].append(e0.elapsed_time(e1) / LAUNCHES)
    torch.cuda.synchronize()
    for f, (words, status) in res.items():
        got = fabgpu.unpack_bits(words.cpu().numpy().view(np.uint64), n)
        assert (got == truth).all() and ((status.cpu().numpy() == 0) == truth).all(), (f, n)
    row = {f: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v} for f, v in per.items()}
    ratios = [a / c for a, c in zip(per["fresh"], per["keyed"])]
    row["fresh_over_keyed_median"] = statistics.median(ratios)
    row["fresh_over_keyed_min"], row["fresh_over_keyed_max"] = min(ratios), max(ratios)
    row["fresh_spread_ms"] = max(per["fresh"]) - min(per["fresh"])
    row["keyed_faster_by_more_than_the_fresh_spread"] = bool(row["fresh"]["min_ms"] - row["keyed"]["max_ms"] > row["fresh_spread_ms"])
    row["keyed_verifies_per_s"] = n / (row["keyed"]["median_ms"] * 1e-3)
    out[str(n)] = row
ctx.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "p384_keyed.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
