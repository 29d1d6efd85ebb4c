#!/usr/bin/env python3
"""Registered-key P-384 verification on 16-bit comb tables (FABGPU_FLAG_P384_KEY_TABLES_16BIT: 24 windows, 48 mixed additions) against
the same one-lane keyed kernel on 8-bit tables (48 windows, 96 additions), one process: two contexts, flag on and flag off, 16
registered keys each, fabgpu_p384_verify_batch_keyed_dev on the same HBM-resident tuples, n = 30 000 and 3 000.  The flag-off figure is
the baseline: the 8-bit kernel, unchanged.  The product counts of csrc/p384_tables16.h predict x 1.43 (1 750 against 1 220); no
threshold is set.

The tuples are 256 signatures made with Python integers (tests/p384_ref.py), repeated to n - the kernels' control flow does not depend
on the operands - with every 97th tuple's r changed afterwards; both contexts' verdicts are checked against exactly that after the timed
region, and the flag-on context's counter must show every row on 16-bit tables.  After a clock warm-up, ROUNDS interleaved rounds
(16-bit, 8-bit, 16-bit, ...; who goes first alternates), each timed by events over back-to-back launches.

Build times, host clock, each on a context of its own: the generator's tables at the warm call (flag on: 8-bit and 16-bit; flag off:
8-bit), one key and then 16 keys from the registration call to the first snapshot that shows their 16-bit tables (the test hook that
waits for the queued builds and publishes), beside the time the registration call itself took.

P384_PARENT_JSON: the output of tools/bench_p384_keyed.py run on the parent commit in the same session; its keyed figures are recorded
beside the flag-off ones.  Writes profiles/p384_keyed16.json and prints the same JSON line."""
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
SIZES = [int(x) for x in os.environ.get("P384_SIZES", "30000,3000").split(",")]
LAUNCHES = 4
N_KEYS = 16
PREDICTED = 1750 / 1220
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
pairs = [(R.b48(q[0]), R.b48(q[1])) for _d, q in keys]

out = {"rounds": ROUNDS, "launches_per_round": LAUNCHES, "keys": N_KEYS, "predicted_ratio_by_product_count": PREDICTED}


def ms(f, idle=True):
    if idle:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    v = f()
    return (time.perf_counter() - t0) * 1e3, v


def warm(c):
    c.p384_verify_batch_keyed_dev(0, None, None, None, None, None, None)          # the warm call: the generator's tables, no launch


# ---- build times ----
build = {}
c0 = fabgpu.Context(device=0)
build["generator_8bit_only_ms"] = ms(lambda: warm(c0))[0]
c0.close()
c1 = fabgpu.Context(device=0, flags=fabgpu.FLAG_P384_KEY_TABLES_16BIT)
build["generator_8bit_and_16bit_ms"] = ms(lambda: warm(c1))[0]
t_reg, _ = ms(lambda: c1.p384_key_register(*pairs[0]))
t_wait, n16 = ms(lambda: fabgpu.p384_tables16_wait(c1), idle=False)               # (straight behind the registration: the build is running)
assert n16 == 1
build["one_key"] = {"registration_call_ms": t_reg, "registration_to_snapshot_ms": t_reg + t_wait}
c1.close()

ctxs = {"tables16": fabgpu.Context(device=0, flags=fabgpu.FLAG_P384_KEY_TABLES_16BIT), "tables8": fabgpu.Context(device=0)}
for c in ctxs.values():
    warm(c)
ids = {}
t_reg, ids["tables16"] = ms(lambda: fabgpu.p384_key_register_batch(ctxs["tables16"], pairs))
t_wait, n16 = ms(lambda: fabgpu.p384_tables16_wait(ctxs["tables16"]), idle=False)
assert n16 == N_KEYS
build["sixteen_keys"] = {"registration_call_ms": t_reg, "registration_to_snapshot_ms": t_reg + t_wait}
build["sixteen_keys_8bit_only_registration_call_ms"], ids["tables8"] = ms(lambda: fabgpu.p384_key_register_batch(ctxs["tables8"], pairs))
assert ids["tables16"] == ids["tables8"] == list(range(N_KEYS))
out["build"] = build

for n in SIZES:
    tuples = [base[i % 256] for i in range(n)]
    truth = np.ones(n, bool)
    for i in range(0, n, 97):
        t = list(tuples[i])
        t[4] ^= 2
        tuples[i] = tuple(t)
        truth[i] = False
    cols = [torch.from_numpy(np.frombuffer(b"".join(R.b48(t[k]) for t in tuples), dtype=np.uint8).copy()).cuda() for k in range(3, 6)]
    kid = torch.from_numpy(np.array([ids["tables16"][t[0]] for t in tuples], dtype=np.uint32).view(np.int32)).cuda()
    res = {f: (torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")) for f in ctxs}

    def call(f):
        ctxs[f].p384_verify_batch_keyed_dev(n, kid.data_ptr(), *[c.data_ptr() for c in cols], res[f][0].data_ptr(), res[f][1].data_ptr(), stream.cuda_stream)
    t_end = time.time() + 2.0        # clock warm-up
    while time.time() < t_end:
        for f in ctxs:
            call(f)
        torch.cuda.synchronize()
    before = ctxs["tables16"].p384_tables16_rows()
    per = {f: [] for f in ctxs}
    for i in range(ROUNDS):
        for f in (("tables16", "tables8") if i % 2 == 0 else ("tables8", "tables16")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(LAUNCHES):
                call(f)
            e1.record(stream)
            e1.synchronize()
            per[f].append(e0.elapsed_time(e1) / LAUNCHES)
    torch.cuda.synchronize()
    assert ctxs["tables16"].p384_tables16_rows() - before == ROUNDS * LAUNCHES * n and ctxs["tables8"].p384_tables16_rows() == 0
    for f, (words, status) in res.items():
        got = fabgpu.unpack_bits(words.cpu().numpy().view(np.uint64), n)
        assert (got == truth).all() and ((status.cpu().numpy() == 0) == truth).all(), (f, n)
    row = {f: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v} for f, v in per.items()}
    ratios = [a / c for a, c in zip(per["tables8"], per["tables16"])]
    row["tables8_over_tables16_median"] = statistics.median(ratios)
    row["tables8_over_tables16_min"], row["tables8_over_tables16_max"] = min(ratios), max(ratios)
    row["tables16_faster_than_the_fastest_tables8_round"] = bool(row["tables16"]["median_ms"] < row["tables8"]["min_ms"])
    row["tables16_verifies_per_s"] = n / (row["tables16"]["median_ms"] * 1e-3)
    out[str(n)] = row
out["key_table_stats_tables16"] = ctxs["tables16"].p384_key_table_stats()
for c in ctxs.values():
    c.close()
parent = os.environ.get("P384_PARENT_JSON")
if parent:
    pj = json.load(open(parent))
    out["parent_commit_bench_p384_keyed"] = {k: (v["keyed"] if isinstance(v, dict) and "keyed" in v else v) for k, v in pj.items()}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "p384_keyed16.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
