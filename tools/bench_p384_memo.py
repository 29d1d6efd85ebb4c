#!/usr/bin/env python3
"""The verdict memo of the block pass's P-384 tuples (provider option p384, FABGPU_PASS_SEED_MEMO), one process.  Writes
profiles/p384_memo.json and prints the same line.

The block is tools/bench_p384_block.py's: 1 000 transactions, a P-384 creator and three P-384 endorsers each (4 000 P-384 tuples), 16
distinct transactions laid out over the 1 000; every signer imported, so the stage runs keyed.
(a) The pass, seeding on against seeding off, rounds interleaved in one provider (who goes first alternates): the cost of seeding is
    the difference of the two medians, reported beside the spread of the off rounds.  Lean passes, after a clock warm-up; the seeded
    block is evicted outside the timed region.
(b) What a validator pool then asks: 4 000 bccsp.Verify questions from 16 threads (ctypes drops the GIL in the calls), once answered by
    fabgpu_csp_memo_lookup_p384 after a seeding pass, once - no memo: the behaviour before this table existed - by the same 4 000
    fabgpu_csp_verify_coalesced_p384 calls.  Wall time of each, same run."""
import ctypes
import hashlib
import json
import os
import random
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("fabric-mod_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import blockbuilder as bb  # noqa: E402
import fabgpu  # noqa: E402
import p384_blocks as pb  # noqa: E402
import p384_ref as ref  # noqa: E402

ROUNDS = int(os.environ.get("P384_ROUNDS", "8"))
N_TX = int(os.environ.get("P384_BLOCK_TX", "1000"))
THREADS = 16


def timed(csp, blk, seq, seed):
    t0 = time.perf_counter()
    out = fabgpu.preverify_block2(csp, blk, block_seq=seq, seed_memo=seed, lean=True)
    return (time.perf_counter() - t0) * 1e3, out


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v}


def from_threads(work):
    """work(t) on THREADS threads at once -> wall milliseconds"""
    th = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    return (time.perf_counter() - t0) * 1e3


rnd = random.Random(384100)
signers = pb.signers(6, 384100)
distinct = [pb.endorser_tx(rnd, signers[t % 2], rnd.sample(signers[2:], 3), ext_bytes=990) for t in range(16)]
blk = bb.block(1, [distinct[t % 16][0] for t in range(N_TX)])
tuples = [tu for t in range(N_TX) for tu in distinct[t % 16][1]]
n_tuples = len(tuples)
questions = [(ref.b48(who.q[0]), ref.b48(who.q[1]), sig, hashlib.sha256(msg).digest()) for _k, who, msg, sig in tuples]

out = {"rounds": ROUNDS, "tx": N_TX, "p384_tuples": n_tuples, "block_bytes": len(blk), "threads": THREADS}
csp = fabgpu.GPUCSP(devices=[0], p384=1)
for sg in signers:
    csp.key_import_p384(sg.q)
first = fabgpu.preverify_block2(csp, blk, block_seq=1, seed_memo=True)
assert (first["tx_flags"] == 0).all() and first["memo_seeded"] == n_tuples
assert fabgpu.memo_evict_block(csp, 1) == n_tuples
t_end = time.time() + 2.0
while time.time() < t_end:
    timed(csp, blk, 2, False)

# ---- (a) the pass, seeding on against off ----
per = {"off": [], "on": []}
for i in range(2 * ROUNDS):
    for name in (("off", "on") if i % 2 == 0 else ("on", "off")):
        ms, o = timed(csp, blk, 10 + i, name == "on")
        assert (o["tx_flags"] == 0).all() and o["memo_seeded"] == (n_tuples if name == "on" else 0)
        per[name].append(ms)
        if name == "on":
            assert fabgpu.memo_evict_block(csp, 10 + i) == n_tuples
st = csp.p384_pass_stats()
assert st["fresh_launches"] == 0
row = {"seed_off": summary(per["off"]), "seed_on": summary(per["on"])}
row["seeding_adds_ms"] = statistics.median(per["on"]) - statistics.median(per["off"])
row["seed_off_spread_ms"] = max(per["off"]) - min(per["off"])
out["pass_keyed"] = row

# ---- (b) 4 000 questions from 16 threads: the memo, and the coalesced entry without one ----
L, h = csp._L, csp._h
look, coal = [], []
for r_ in range(ROUNDS):
    _, o = timed(csp, blk, 500 + r_, True)
    hits = [0] * THREADS

    def ask_memo(t):
        st8 = ctypes.c_uint8(255)
        for qx, qy, sig, dg in questions[t::THREADS]:
            if L.fabgpu_csp_memo_lookup_p384(h, qx, qy, sig, len(sig), dg, 32, ctypes.byref(st8), None) == 0 and st8.value == 0:
                hits[t] += 1
    look.append(from_threads(ask_memo))
    assert sum(hits) == n_tuples
    assert fabgpu.memo_evict_block(csp, 500 + r_) == n_tuples
    valid = [0] * THREADS

    def ask_coalesced(t):
        v, fl = ctypes.c_int(0), ctypes.c_int(0)
        err = ctypes.create_string_buffer(64)
        for qx, qy, sig, dg in questions[t::THREADS]:
            if L.fabgpu_csp_verify_coalesced_p384(h, qx, qy, sig, len(sig), dg, 32, ctypes.byref(v), ctypes.byref(fl), err, 64) == 0 and v.value == 1:
                valid[t] += 1
    coal.append(from_threads(ask_coalesced))
    assert sum(valid) == n_tuples
out["lookups_16_threads"] = {"memo_lookup_p384": summary(look), "verify_coalesced_p384_no_memo": summary(coal),
                             "note": "Python threads around ctypes calls: the interpreter's share is in both figures"}
out["memo_stats"] = fabgpu.memo_stats_p384(csp)
csp.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "p384_memo.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
