#!/usr/bin/env python3
"""SHA3-256 against SHA-256 on the device, same messages, one process: fabgpu_sha3_256_batch against fabgpu_sha256_batch and
fabgpu_sha3_256_p256_verify_batch against fabgpu_sha256_p256_verify_batch, through the _dev entry points on HBM-resident inputs.
Shapes: 300 000 x 1 856 B (BASELINE configs[3]) and 30 000 x 1 856 B, fresh keys.  After a clock warm-up, ROUNDS interleaved rounds per
shape (sha256, sha3, sha256, sha3, ...), each timed by events over back-to-back launches.  Every 97th message has a byte flipped on the
device after signing: the verdicts of both families are checked against exactly that after the timed region, and the digests of a
sample of rows against hashlib.  Writes profiles/sha3_batch.json (medians, min / max over rounds, ratios, the kernel names one
untimed pass of each call launched) and prints the same JSON line."""
import hashlib
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

ROUNDS = int(os.environ.get("SHA3_ROUNDS", "8"))
SIZES = [int(x) for x in os.environ.get("SHA3_SIZES", "300000,30000").split(",")]
MSG = 1856
LAUNCHES = {"hash": 10, "verify": 5}
torch.cuda.set_device(0)
stream = torch.cuda.current_stream()
ctx = fabgpu.Context(device=0)
fabgpu.load_hooks()
out = {"rounds": ROUNDS, "message_bytes": MSG, "launches_per_round": LAUNCHES}


def kernel_names(fn):
    """names of the kernels one call launches (an untimed pass under the profiler); None when the profiler is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sorted({e.key for e in prof.key_averages() if "fab" in e.key or "sha" in e.key.lower() or "p256" in e.key})
    except Exception as x:   # noqa: BLE001
        return "profiler unavailable: %r" % (x,)


for n in SIZES:
    g = torch.Generator(device="cuda").manual_seed(1856 + n)
    arena = torch.randint(0, 256, (n * MSG + 64,), dtype=torch.uint8, device="cuda", generator=g)
    off = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * MSG).to(torch.int32)
    dig = {f: torch.zeros((n, 32), dtype=torch.uint8, device="cuda") for f in ("sha256", "sha3")}
    hash_fn = {"sha256": ctx.sha256_batch_dev, "sha3": ctx.sha3_256_batch_dev}
    verify_fn = {"sha256": ctx.sha256_p256_verify_batch_dev, "sha3": ctx.sha3_256_p256_verify_batch_dev}

    def hash_(f):
        hash_fn[f](n, arena.data_ptr(), arena.numel(), off.data_ptr(), dig[f].data_ptr(), stream.cuda_stream)
    for f in dig:
        hash_(f)
    torch.cuda.synchronize()
    sample = list(range(0, n, max(1, n // 64)))
    host = arena.cpu().numpy()
    for i in sample:
        m = host[i * MSG:(i + 1) * MSG].tobytes()
        assert dig["sha256"][i].cpu().numpy().tobytes() == hashlib.sha256(m).digest(), (n, i)
        assert dig["sha3"][i].cpu().numpy().tobytes() == hashlib.sha3_256(m).digest(), (n, i)
    # one signature set per family over the same messages, every tuple valid ...
    sig = {}
    for f in dig:
        b = fabgpu.synth_batch(n, seed=20260921, invalid_permille=0, e_in=dig[f].cpu().numpy())
        sig[f] = {k: torch.from_numpy(b[k]).cuda() for k in ("qx", "qy", "r", "s")}
    # ... then every 97th message changes under them
    broken = torch.arange(0, n, 97, device="cuda")
    arena[broken * MSG + 1000] ^= 0x20
    truth = np.ones(n, bool)
    truth[broken.cpu().numpy()] = False
    words = {f: torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda") for f in dig}
    status = {f: torch.zeros(n, dtype=torch.uint8, device="cuda") for f in dig}

    def verify(f):
        s = sig[f]
        verify_fn[f](n, arena.data_ptr(), arena.numel(), off.data_ptr(), s["qx"].data_ptr(), s["qy"].data_ptr(), s["r"].data_ptr(), s["s"].data_ptr(),
                     words[f].data_ptr(), status[f].data_ptr(), stream.cuda_stream)
    calls = {"hash": hash_, "verify": verify}
    names = {"%s_%s" % (c, f): kernel_names(lambda c=c, f=f: calls[c](f)) for c in calls for f in dig}
    t_end = time.time() + 2.0        # clock warm-up
    while time.time() < t_end:
        for f in dig:
            hash_(f)
            verify(f)
        torch.cuda.synchronize()
    row = {"kernels": names}
    for c, call in calls.items():
        per = {f: [] for f in dig}
        for _ in range(ROUNDS):
            for f in dig:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(LAUNCHES[c]):
                    call(f)
                e1.record(stream)
                e1.synchronize()
                per[f].append(e0.elapsed_time(e1) / LAUNCHES[c])
        r = {f: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for f, v in per.items()}
        ratios = [b3 / b2 for b2, b3 in zip(per["sha256"], per["sha3"])]
        r["sha3_over_sha256_median"] = statistics.median(ratios)
        r["sha3_over_sha256_min"], r["sha3_over_sha256_max"] = min(ratios), max(ratios)
        if c == "hash":
            r["sha3_gb_per_s"] = n * MSG / (r["sha3"]["median_ms"] * 1e-3) / 1e9
            r["sha256_gb_per_s"] = n * MSG / (r["sha256"]["median_ms"] * 1e-3) / 1e9
        row[c] = r
    torch.cuda.synchronize()
    for f in dig:                    # verdicts, after the timed region
        got = fabgpu.unpack_bits(words[f].cpu().numpy().view(np.uint64), n)
        assert (got == truth).all(), (n, f, int((got != truth).sum()))
        assert ((status[f].cpu().numpy() == 0) == truth).all(), (n, f)
    out[str(n)] = row
    del arena, host
ctx.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "sha3_batch.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
