#!/usr/bin/env python3
"""Registered-key P-384 verification on eight lanes per signature (FABGPU_FLAG_P384_WIDE) against the one-lane keyed kernel, one process:
two contexts, flag on and flag off, 16 registered keys each, fabgpu_p384_verify_batch_keyed_dev on the same HBM-resident tuples,
n = 1 000, 4 000 and 8 192.  The flag-off figure is the comparator: the one-lane kernel, unchanged.

The tuples are 256 signatures made with Python integers (tests/p384_ref.py), repeated to n - the kernels' control flow does not depend
on the operands - with every 97th tuple's r changed afterwards; both contexts' verdicts are checked against exactly that after the timed
region.  After a clock warm-up, ROUNDS interleaved rounds (wide, one-lane, wide, ...; who goes first alternates), each timed by events
over back-to-back launches.  Writes profiles/p384_keyed_wide.json and prints the same JSON line."""
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

ROUNDS = int(os.environ.get("P384_ROUNDS", "8"))
SIZES = [int(x) for x in os.environ.get("P384_SIZES", "1000,4000,8192").split(",")]
LAUNCHES = 4
N_KEYS = 16
torch.cuda.set_device(0)
stream = torch.cuda.current_stream()
fabgpu.load_hooks()

rng = random.Random(384816)
keys = []
for _ in range(N_KEYS):
    d = rng.randrange(1, R.N)
    keys.append((d, R.mul(d, R.G)))
base = []
for i in range(256):
    d, q = keys[i % N_KEYS]
    e = rng.randrange(2**256)
    r, s = R.sign(d, e, rng.randrange(1, 2**40))
    base.append((i % N_KEYS, q[0], q[1], e, r, R.low_s(s)))

out = {"rounds": ROUNDS, "launches_per_round": LAUNCHES, "keys": N_KEYS}
pairs = [(R.b48(q[0]), R.b48(q[1])) for _d, q in keys]
ctxs = {"wide": fabgpu.Context(device=0, flags=fabgpu.FLAG_P384_WIDE), "one_lane": fabgpu.Context(device=0)}
ids = {f: fabgpu.p384_key_register_batch(c, pairs) for f, c in ctxs.items()}
assert ids["wide"] == ids["one_lane"] == list(range(N_KEYS))

for n in SIZES:
    tuples = [base[i % 256] for i in range(n)]
    truth = np.ones(n, bool)
    for i in range(0, n, 97):
        t = list(tuples[i])
        t[4] ^= 2
        tuples[i] = tuple(t)
        truth[i] = False
    cols = [torch.from_numpy(np.frombuffer(b"".join(R.b48(t[k]) for t in tuples), dtype=np.uint8).copy()).cuda() for k in range(3, 6)]
    kid = torch.from_numpy(np.array([ids["wide"][t[0]] for t in tuples], dtype=np.uint32).view(np.int32)).cuda()
    res = {f: (torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")) for f in ctxs}

    def call(f):
        ctxs[f].p384_verify_batch_keyed_dev(n, kid.data_ptr(), *[c.data_ptr() for c in cols], res[f][0].data_ptr(), res[f][1].data_ptr(), stream.cuda_stream)
    before = ctxs["wide"].p384_wide_rows()
    t_end = time.time() + 2.0        # clock warm-up
    while time.time() < t_end:
        for f in ctxs:
            call(f)
        torch.cuda.synchronize()
    per = {f: [] for f in ctxs}
    for i in range(ROUNDS):
        for f in (("wide", "one_lane") if i % 2 == 0 else ("one_lane", "wide")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(LAUNCHES):
                call(f)
            e1.record(stream)
            e1.synchronize()
            per[f].append(e0.elapsed_time(e1) / LAUNCHES)
    torch.cuda.synchronize()
    assert ctxs["wide"].p384_wide_rows() > before and ctxs["one_lane"].p384_wide_rows() == 0
    for f, (words, status) in res.items():
        got = fabgpu.unpack_bits(words.cpu().numpy().view(np.uint64), n)
        assert (got == truth).all() and ((status.cpu().numpy() == 0) == truth).all(), (f, n)
    row = {f: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v} for f, v in per.items()}
    ratios = [a / c for a, c in zip(per["one_lane"], per["wide"])]
    row["one_lane_over_wide_median"] = statistics.median(ratios)
    row["one_lane_over_wide_min"], row["one_lane_over_wide_max"] = min(ratios), max(ratios)
    row["wide_verifies_per_s"] = n / (row["wide"]["median_ms"] * 1e-3)
    out[str(n)] = row
for c in ctxs.values():
    c.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "p384_keyed_wide.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
