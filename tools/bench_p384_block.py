#!/usr/bin/env python3
"""The block pass with its P-384 stage (provider option p384), one process.  Writes profiles/p384_block_pass.json and prints the same line.

(a) A 1 000-transaction block, a P-384 creator and three P-384 endorsers each (4 000 P-384 tuples): the pass with the stage on the
    fresh-key kernel (no key imported), then on the keyed kernel (fabgpu_csp_key_import_p384 of every signer); beside them libcrypto's
    P-384 verify over the same tuples on 16 threads, timed the way tools/bench_p384.py times it.  The block is 16 distinct transactions (64 signatures made with
    Python integers, tests/p384_ref.py) laid out over the 1 000 - the kernels' control flow does not depend on the operands.
(b) The 10 000-transaction all-P-256 block of the bench (tests/blockgen.py, as bench.py builds it) through ONE provider, option on
    against off, rounds interleaved (who goes first alternates): the option-on median against the option-off rounds' own spread, and the stage's counters (no launch).
Passes are the lean form a memo-less caller asks for (tx_flags only), after a clock warm-up.

--sha3: another measurement instead, written to profiles/p384_block_pass_sha3.json.  The 1 000-transaction block with a P-384 creator
    of a SHA2 MSP and three P-384 endorsers of an MSP of the SHA3 family (signatures over SHA3-256): the pass with that MSP registered
    SHA3 (fabgpu_csp_msp_hash_family: two described batches, 1 000 rows under SHA-256 and 3 000 under SHA3-256) against the same block
    with the MSP left SHA2 (one batch of 4 000 rows under SHA-256, the endorsements "not valid"), one provider, rounds interleaved (who
    goes first alternates), on the fresh-key kernel and then on the keyed one."""
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("fabric-mod_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import blockbuilder as bb  # noqa: E402
import blockgen  # noqa: E402
import fabgpu  # noqa: E402
import p384_blocks as pb  # noqa: E402

ROUNDS = int(os.environ.get("P384_ROUNDS", "8"))
N_TX = int(os.environ.get("P384_BLOCK_TX", "1000"))
N_TX_256 = int(os.environ.get("P256_BLOCK_TX", "10000"))
fabgpu.load_hooks()


def timed(csp, blk, seq):
    t0 = time.perf_counter()
    out = fabgpu.preverify_block2(csp, blk, block_seq=seq, lean=True)
    return (time.perf_counter() - t0) * 1e3, out


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v}


def cpu_verify_seconds(tuples):
    """libcrypto ECDSA_do_verify(P-384) over (qx, qy, digest32, r, s) on 16 threads (ctypes drops the GIL in the calls), as
    tools/bench_p384.py times it: wall seconds, and how many verified"""
    import ctypes
    import ctypes.util
    import threading

    import p384_ref as R
    C = ctypes.CDLL(ctypes.util.find_library("crypto"))
    vp = ctypes.c_void_p
    for f in ("EC_KEY_new_by_curve_name", "BN_bin2bn", "ECDSA_SIG_new", "BN_new"):
        getattr(C, f).restype = vp
    C.EC_KEY_set_public_key_affine_coordinates.argtypes = [vp, vp, vp]
    C.ECDSA_SIG_set0.argtypes = [vp, vp, vp]
    C.ECDSA_do_verify.argtypes = [ctypes.c_char_p, ctypes.c_int, vp, vp]
    C.BN_bin2bn.argtypes = [ctypes.c_char_p, ctypes.c_int, vp]
    items = []
    for qx, qy, dg, r, s in tuples:
        k = C.EC_KEY_new_by_curve_name(715)                   # NID_secp384r1
        assert C.EC_KEY_set_public_key_affine_coordinates(k, C.BN_bin2bn(R.b48(qx), 48, None), C.BN_bin2bn(R.b48(qy), 48, None)) == 1
        sg = C.ECDSA_SIG_new()
        C.ECDSA_SIG_set0(sg, C.BN_bin2bn(R.b48(r), 48, None), C.BN_bin2bn(R.b48(s), 48, None))
        items.append((dg, k, sg))
    n_ok = [0] * 16

    def work(t):
        for dg, k, sg in items[t::16]:
            n_ok[t] += C.ECDSA_do_verify(dg, 32, sg, k) == 1
    th = [threading.Thread(target=work, args=(t,)) for t in range(16)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    return time.perf_counter() - t0, sum(n_ok)


def sha3_mode():
    import p384_sha3_blocks as pb3
    rnd = random.Random(384103)
    creators = [pb3.Signer(rnd, "client%d.org1.example.com" % i, "Org1MSP", sha3=False) for i in range(2)]
    endorsers = [pb3.Signer(rnd, "peer%d.org3.example.com" % i, "Org3MSP", sha3=True) for i in range(4)]
    distinct = [pb.endorser_tx(rnd, creators[t % 2], rnd.sample(endorsers, 3), ext_bytes=990) for t in range(16)]
    blk = bb.block(1, [distinct[t % 16][0] for t in range(N_TX)])
    csp = fabgpu.GPUCSP(devices=[0], p384=1, hash_sha3=1)
    want = {"SHA3": fabgpu.TX_ALL_SIGNATURES_VALID, "SHA2": fabgpu.TX_BAD_ENDORSEMENT}
    res = {"rounds": ROUNDS, "tx": N_TX, "p384_tuples": 4 * N_TX, "sha3_tuples": 3 * N_TX, "block_bytes": len(blk)}
    for kernel in ("fresh", "keyed"):
        if kernel == "keyed":
            for sg in creators + endorsers:
                csp.key_import_p384(sg.q)
        for fam in ("SHA3", "SHA2"):                                # every path once, checked in full
            csp.msp_hash_family("Org3MSP", fam)
            first = fabgpu.preverify_block2(csp, blk, block_seq=1)
            assert (first["tx_flags"] == want[fam]).all() and len(first["tuple_status"]) == 4 * N_TX
        t_end = time.time() + 2.0
        while time.time() < t_end:
            timed(csp, blk, 2)
        per = {"SHA3": [], "SHA2": []}
        s0 = csp.p384_pass_stats()
        for i in range(2 * ROUNDS):
            for fam in (("SHA2", "SHA3") if i % 2 == 0 else ("SHA3", "SHA2")):     # (who goes first alternates)
                csp.msp_hash_family("Org3MSP", fam)
                ms, o = timed(csp, blk, 10 + i)
                assert (o["tx_flags"] == want[fam]).all()
                per[fam].append(ms)
        s1 = csp.p384_pass_stats()
        launches = s1[kernel + "_launches"] - s0[kernel + "_launches"]
        assert launches == 2 * ROUNDS * 3 and s1["sha3_rows"] - s0["sha3_rows"] == 2 * ROUNDS * 3 * N_TX       # two batches a SHA3 pass, one a SHA2 pass
        res[kernel] = {"msp_sha3_two_batches": summary(per["SHA3"]), "msp_left_sha2_one_batch": summary(per["SHA2"]),
                       "sha3_minus_sha2_median_ms": statistics.median(per["SHA3"]) - statistics.median(per["SHA2"])}
    res["stage_stats"] = csp.p384_pass_stats()
    csp.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "p384_block_pass_sha3.json"), "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res))


def wide_mode():
    """--wide: the 1 000-transaction P-384 block of (a), every signer imported, through ONE provider with the option p384_wide switched
    between the passes of a round (who goes first alternates): the keyed batch of 4 000 rows on eight lanes per signature against the
    one-lane keyed kernel.  Written to profiles/p384_block_pass_wide.json."""
    rnd = random.Random(384100)
    signers = pb.signers(6, 384100)
    distinct = [pb.endorser_tx(rnd, signers[t % 2], rnd.sample(signers[2:], 3), ext_bytes=990) for t in range(16)]
    blk = bb.block(1, [distinct[t % 16][0] for t in range(N_TX)])
    csp = fabgpu.GPUCSP(devices=[0], p384=1, p384_wide=1)
    for sg in signers:
        csp.key_import_p384(sg.q)
    for on in (1, 0):                                               # both forms once, checked in full
        csp.set_option("p384_wide", on)
        first = fabgpu.preverify_block2(csp, blk, block_seq=1)
        assert (first["tx_flags"] == 0).all() and (first["tuple_status"] == 0).all() and len(first["tuple_status"]) == 4 * N_TX
    t_end = time.time() + 2.0
    while time.time() < t_end:
        timed(csp, blk, 2)
    per = {"wide": [], "one_lane": []}
    s0 = csp.p384_pass_stats()
    for i in range(2 * ROUNDS):
        for name in (("one_lane", "wide") if i % 2 == 0 else ("wide", "one_lane")):
            csp.set_option("p384_wide", 1 if name == "wide" else 0)
            ms, o = timed(csp, blk, 10 + i)
            assert (o["tx_flags"] == 0).all()
            per[name].append(ms)
    s1 = csp.p384_pass_stats()
    assert s1["keyed_launches"] - s0["keyed_launches"] == 4 * ROUNDS and s1["wide_rows"] - s0["wide_rows"] == 2 * ROUNDS * 4 * N_TX
    res = {"rounds": 2 * ROUNDS, "tx": N_TX, "p384_tuples": 4 * N_TX, "block_bytes": len(blk), "pass_keyed_wide": summary(per["wide"]),
           "pass_keyed_one_lane": summary(per["one_lane"]), "stage_stats": s1}
    res["one_lane_minus_wide_median_ms"] = statistics.median(per["one_lane"]) - statistics.median(per["wide"])
    csp.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "p384_block_pass_wide.json"), "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res))


if "--sha3" in sys.argv[1:]:
    sha3_mode()
    sys.exit(0)
if "--wide" in sys.argv[1:]:
    wide_mode()
    sys.exit(0)

out = {"rounds": ROUNDS}
# ---- (a) the P-384 block ----
rnd = random.Random(384100)
signers = pb.signers(6, 384100)
distinct = [pb.endorser_tx(rnd, signers[t % 2], rnd.sample(signers[2:], 3), ext_bytes=990) for t in range(16)]
blk384 = bb.block(1, [distinct[t % 16][0] for t in range(N_TX)])
tuples = [tu for t in range(N_TX) for tu in distinct[t % 16][1]]
csp = fabgpu.GPUCSP(devices=[0], p384=1)
first = fabgpu.preverify_block2(csp, blk384, block_seq=1)
assert (first["tx_flags"] == 0).all() and (first["tuple_status"] == 0).all() and len(first["tuple_status"]) == 4 * N_TX
t_end = time.time() + 2.0
while time.time() < t_end:
    timed(csp, blk384, 2)
per = {"fresh": [], "keyed": []}
s0 = csp.p384_pass_stats()
for i in range(ROUNDS):
    ms, o = timed(csp, blk384, 10 + i)
    assert (o["tx_flags"] == 0).all()
    per["fresh"].append(ms)
s1 = csp.p384_pass_stats()
assert s1["fresh_launches"] - s0["fresh_launches"] == ROUNDS and s1["keyed_launches"] == 0
for sg in signers:
    csp.key_import_p384(sg.q)
timed(csp, blk384, 3)
for i in range(ROUNDS):
    ms, o = timed(csp, blk384, 100 + i)
    assert (o["tx_flags"] == 0).all()
    per["keyed"].append(ms)
s2 = csp.p384_pass_stats()
assert s2["keyed_launches"] - s1["keyed_launches"] == ROUNDS + 1 and s2["fresh_launches"] == s1["fresh_launches"]
csp.set_option("p384", 0)                                   # the same block with the stage off: walk, upload and the (empty) P-256 part alone
off_ms = []
for i in range(ROUNDS):
    ms, o = timed(csp, blk384, 200 + i)
    assert (o["tx_flags"] == fabgpu.TX_NEEDS_SW).all()
    off_ms.append(ms)
out["p384_block"] = {"tx": N_TX, "p384_tuples": 4 * N_TX, "block_bytes": len(blk384), "pass_stage_fresh": summary(per["fresh"]), "pass_stage_keyed": summary(per["keyed"]),
                     "pass_option_off_all_needs_sw": summary(off_ms), "stage_stats": s2}
out["p384_block"]["stage_adds_fresh_ms"] = statistics.median(per["fresh"]) - statistics.median(off_ms)
out["p384_block"]["stage_adds_keyed_ms"] = statistics.median(per["keyed"]) - statistics.median(off_ms)
csp.close()
cpu_s, cpu_ok = cpu_verify_seconds([(who.q[0], who.q[1], hashlib.sha256(msg).digest()) + pb.parse_der_sig(sig) for _k, who, msg, sig in tuples])
assert cpu_ok == 4 * N_TX
out["p384_block"]["libcrypto_16_threads_ms"] = cpu_s * 1e3

# ---- (b) the all-P-256 block, option on against off ----
blk256, _ = blockgen.endorser_block(N_TX_256, seed=1)
csp = fabgpu.GPUCSP(devices=[0])                             # ONE provider, the option switched between the passes of a round
csp._L.fabgpu_csp_identity_cache_limits(csp._h, 4096, 256, 1)
for k in range(3):
    timed(csp, blk256, 1 + k)
t_end = time.time() + 2.0
while time.time() < t_end:
    timed(csp, blk256, 5)
per = {"off": [], "on": []}
for i in range(2 * ROUNDS):
    for name in (("off", "on") if i % 2 == 0 else ("on", "off")):     # (who goes first alternates)
        csp.set_option("p384", 1 if name == "on" else 0)
        ms, o = timed(csp, blk256, 10 + i)
        assert (o["tx_flags"] == 0).all()
        per[name].append(ms)
row = {"tx": N_TX_256, "block_bytes": len(blk256), "option_off": summary(per["off"]), "option_on": summary(per["on"]), "stage_stats_option_on": csp.p384_pass_stats()}
row["option_on_median_inside_option_off_spread"] = bool(min(per["off"]) <= statistics.median(per["on"]) <= max(per["off"]))
row["no_stage_launch"] = row["stage_stats_option_on"] == dict.fromkeys(fabgpu.P384_PASS_STATS, 0)
out["p256_block_option_on_vs_off"] = row
csp.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "p384_block_pass.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
