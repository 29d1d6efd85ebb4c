#!/usr/bin/env python3
"""A/B of the LDS-table pair kernel's two builds of its table of odd multiples in one process: a doubling with update and seven co-Z
additions (the default) against a doubling, a mixed and six general additions (FABGPU_FLAG_PAIR_TABLE_ADD), as tools/gpu_pair_odd_ab.py
does for the recodings.  A second context with the SAME flags as the general-addition form ("add_again") runs in every round too: the
ratio of the two is the round-to-round spread of the method itself.  Fresh-key tuples resident in HBM, 1 % invalid; after a clock
warm-up, ROUNDS interleaved rounds per size (coz, add, add_again, ...), each timed by HIP events over back-to-back launches; verdicts
checked against the generator's ground truth, verdict words and status bytes between the forms.  One JSON line (also written to the
file named as the first argument); "gain" says whether the bar holds at 30 000 tuples: the co-Z form faster in EVERY round and the
median gain at least three times the largest same-form spread of the run.  AB_EXTRA_FLAGS adds flag bits to every context
(FLAG_PAIR_SOLO: the one-wave forms)."""
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
LDS = fabgpu.FLAG_PAIR_TABLE_LDS | int(os.environ.get("AB_EXTRA_FLAGS", "0"), 0)
forms = {"coz": fabgpu.Context(device=0, max_batch=32768, flags=LDS),
         "add": fabgpu.Context(device=0, max_batch=32768, flags=LDS | fabgpu.FLAG_PAIR_TABLE_ADD),
         "add_again": fabgpu.Context(device=0, max_batch=32768, flags=LDS | fabgpu.FLAG_PAIR_TABLE_ADD)}
out = {"rounds": ROUNDS, "launches_per_round": LAUNCHES, "flags": LDS}
for n in SIZES:
    b = fabgpu.synth_batch(n, seed=20260921, invalid_permille=10)
    dev = {k: torch.from_numpy(b[k]).cuda() for k in ("qx", "qy", "e", "r", "s")}
    words = {m: torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda") for m in forms}
    status = {m: torch.zeros(n, dtype=torch.uint8, device="cuda") for m in forms}

    def verify(m):
        forms[m].p256_verify_batch_dev(n, dev["qx"].data_ptr(), dev["qy"].data_ptr(), dev["e"].data_ptr(), dev["r"].data_ptr(),
                                       dev["s"].data_ptr(), words[m].data_ptr(), status[m].data_ptr(), stream.cuda_stream)
    t_end = time.time() + 2.0        # clock warm-up: 2 s of back-to-back launches of every form
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
        assert (status[m].cpu() == status["add"].cpu()).all() and (words[m].cpu() == words["add"].cpu()).all(), (n, m)
    row = {m: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for m, v in per.items()}
    gains = [ad / cz - 1.0 for cz, ad in zip(per["coz"], per["add"])]                   # > 0: the co-Z form is faster
    noise = [abs(a / c - 1.0) for a, c in zip(per["add"], per["add_again"])]            # the same kernel against itself
    row["gain_per_round"] = gains
    row["gain_median"], row["gain_min"], row["gain_max"] = statistics.median(gains), min(gains), max(gains)
    row["spread_same_form_max"] = max(noise)
    row["spread_same_form_median"] = statistics.median(noise)
    row["every_round_faster"] = all(g > 0 for g in gains)
    row["gain"] = row["every_round_faster"] and row["gain_median"] >= 3.0 * row["spread_same_form_max"]
    row["coz_verifies_per_s"] = n / (row["coz"]["median_ms"] * 1e-3)
    out[str(n)] = row
for c in forms.values():
    c.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(json.dumps(out) + "\n")
