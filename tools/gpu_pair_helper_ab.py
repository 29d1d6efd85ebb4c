#!/usr/bin/env python3
"""A/B of the LDS-table pair kernel's two forms in one process: helper waves (the default: a second wave per SIMD computes s^-1, u1, u2
and u1*G beside the u2*Q chain) against one wave per SIMD (FABGPU_FLAG_PAIR_SOLO).  Fresh-key tuples resident in HBM, 1 % invalid;
after a clock warm-up, ROUNDS interleaved rounds per size (helper, solo, helper, solo, ...), each round timed by HIP events over
back-to-back launches; verdicts checked against the generator's ground truth and between the forms.  One JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-mod_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fabgpu  # noqa: E402

ROUNDS = int(os.environ.get("AB_ROUNDS", "12"))
SIZES = [int(x) for x in os.environ.get("AB_SIZES", "20000,30000,32768").split(",")]   # (profiler passes: AB_SIZES=30000)
LAUNCHES = 20          # per round
torch.cuda.set_device(0)
stream = torch.cuda.current_stream()
forms = {"helper": fabgpu.Context(device=0, max_batch=32768, flags=fabgpu.FLAG_PAIR_TABLE_LDS),
         "solo": fabgpu.Context(device=0, max_batch=32768, flags=fabgpu.FLAG_PAIR_TABLE_LDS | fabgpu.FLAG_PAIR_SOLO)}
out = {"rounds": ROUNDS, "launches_per_round": LAUNCHES}
for n in SIZES:
    b = fabgpu.synth_batch(n, seed=20260921, invalid_permille=10)
    dev = {k: torch.from_numpy(b[k]).cuda() for k in ("qx", "qy", "e", "r", "s")}
    words = {m: torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda") for m in forms}
    status = {m: torch.zeros(n, dtype=torch.uint8, device="cuda") for m in forms}

    def verify(m):
        forms[m].p256_verify_batch_dev(n, dev["qx"].data_ptr(), dev["qy"].data_ptr(), dev["e"].data_ptr(), dev["r"].data_ptr(),
                                       dev["s"].data_ptr(), words[m].data_ptr(), status[m].data_ptr(), stream.cuda_stream)
    t_end = time.time() + 2.0        # clock warm-up: 2 s of back-to-back launches of both forms
    while time.time() < t_end:
        for m in forms:
            for _ in range(5):
                verify(m)
        torch.cuda.synchronize()
    per = {m: [] for m in forms}
    for _ in range(ROUNDS):
        for m in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(LAUNCHES):
                verify(m)
            e1.record(stream)
            e1.synchronize()
            per[m].append(e0.elapsed_time(e1) / LAUNCHES)
    truth = b["kind"] == 0
    for m in forms:
        got = fabgpu.unpack_bits(words[m].cpu().numpy().view(np.uint64), n)
        assert (got == truth).all(), (n, m)
    assert (status["helper"].cpu() == status["solo"].cpu()).all(), n
    row = {m: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for m, v in per.items()}
    ratios = [s / h for h, s in zip(per["helper"], per["solo"])]
    row["speedup_median"] = statistics.median(ratios)
    row["speedup_min"], row["speedup_max"] = min(ratios), max(ratios)
    row["helper_verifies_per_s"] = n / (row["helper"]["median_ms"] * 1e-3)
    out[str(n)] = row
for c in forms.values():
    c.close()
print(json.dumps(out))
