#!/usr/bin/env python3
"""What the CPU audit of idemix pseudonym verdicts costs the validators (the sibling of tools/audit_cost.py): tools/go_call_replay.c on
a 10 000-transaction block whose every fifth creator is an idemix pseudonym (tools/make_bench_blocks.py idemix 10000 5), with the
issuer key registered (--idemix-ipk), at --audit-permille 0, 1, 10 and - for the time of ONE audit with warm code and tables, which a
block's two pseudonym audits at permille 1 do not show - 1000, `--runs` fresh processes each.  The same call prices the P-256 audit:
the all-ECDSA block of tools/audit_cost.py runs at the same settings beside it, and a setting's audit time is split between the kinds
by comparing the two blocks (see `figures` below).  With --parent-exe (a go_call_replay of the parent commit, its libfabgpu.so next to it; it
knows no --idemix-ipk, its idemix creators go to bccsp/idemix) the all-ECDSA block also runs through that build at permille 0: the
run-to-run spread the permille-0 figure of this build has to lie within.  Writes one JSON document (default
profiles/audit_cost_nym.json).  Needs a GPU.
    python tools/audit_cost_nym.py [--parent-exe PATH] [--runs 3] [--blocks 12] [--threads 16] [--out profiles/audit_cost_nym.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "fabric-mod_amd")]


def replay(exe, block, blocks, threads, permille=None, ipk=None):
    cmd = [exe] + ([] if permille is None else ["--audit-permille", str(permille)]) + ([] if ipk is None else ["--idemix-ipk", ipk]) + \
          [block, str(blocks), str(threads), "1", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not line:
        raise SystemExit("%s: rc %d: %s" % (" ".join(cmd), r.returncode, (r.stderr or r.stdout)[-400:]))
    return json.loads(line[-1])


def summarise(runs, blocks):
    v = [r["validators_ms_per_block_median"] for r in runs]
    e = {"validators_ms_per_block": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
    if "audit" in runs[0]:
        for k in ("digest_audits", "verdict_audits", "nym_audits", "skipped_nym", "mismatches", "poisoned", "audit_ns"):
            e[k] = [r["audit"].get(k, 0) for r in runs]
        e["audit_ms_per_block"] = [r["audit"]["audit_ms_per_block"] for r in runs]
        e["nym_memo_hits"] = [r.get("nym_memo_hits", 0) for r in runs]
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tx", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audit_cost_nym.json"))
    a = ap.parse_args()
    cache = os.path.join(ROOT, ".bench_blocks")
    os.makedirs(cache, exist_ok=True)
    iblock, eblock = os.path.join(cache, "idemix_%d_5.bin" % a.tx), os.path.join(cache, "friendly_%d.bin" % a.tx)
    if not os.path.exists(iblock):
        import make_bench_blocks
        open(iblock, "wb").write(make_bench_blocks.mixed_block("idemix", a.tx, 5))
    if not os.path.exists(eblock):
        import blockgen
        open(eblock, "wb").write(blockgen.endorser_block(a.tx, 1)[0])
    raw_ipk = bytes.fromhex(json.load(open(os.path.join(ROOT, "tests", "golden", "idemix_fixtures.json")))["msps"]["MSP1OU1"]["ipk"])
    exe = os.path.join(ROOT, "fabric-mod_amd", "lib", "go_call_replay")
    doc = {"what": "tools/go_call_replay.c, %d blocks of %d transactions, %d validator threads, %d fresh processes per setting; idemix block: every "
                   "fifth creator an idemix pseudonym, issuer key registered; validators_ms_per_block = the validators' CPU residue per block "
                   "(median over the blocks of a run)" % (a.blocks, a.tx, a.threads, a.runs), "idemix_block": {}, "ecdsa_block": {}}
    with tempfile.NamedTemporaryFile(suffix=".ipk") as kf:
        kf.write(raw_ipk)
        kf.flush()
        runs = {}
        for _ in range(a.runs):                                # interleaved, so that drift of the machine falls on every setting alike
            if a.parent_exe:
                runs.setdefault(("ecdsa", "parent"), []).append(replay(a.parent_exe, eblock, a.blocks, a.threads))
            for pm in (0, 1, 10, 1000):
                runs.setdefault(("ecdsa", pm), []).append(replay(exe, eblock, a.blocks, a.threads, pm))
            for pm in (0, 1, 10, 1000):
                runs.setdefault(("idemix", pm), []).append(replay(exe, iblock, a.blocks, a.threads, pm, kf.name))
    for (blk, pm), rs in runs.items():
        doc["%s_block" % blk]["parent_commit" if pm == "parent" else "audit_permille_%d" % pm] = summarise(rs, a.blocks)
    E, I = doc["ecdsa_block"], doc["idemix_block"]
    # The library has one clock for all kinds.  Both blocks have the same number of signatures and of digest audits; on the idemix block a
    # pseudonym audit stands where the all-ECDSA block has a creator's verdict audit.  So, per setting (how cold an audit's code and
    # tables are depends on the setting): a digest + verdict pair of the P-256 audit from the all-ECDSA block, and one pseudonym audit =
    # (audit time of the idemix block - audit time of the all-ECDSA block) / pseudonym audits + that pair's price (the digest audit's
    # share of the pair, a few microseconds of SHA-256, is counted to the verdict it goes with).
    figures = {}
    for pm in (1, 10, 1000):
        s, e = I["audit_permille_%d" % pm], E["audit_permille_%d" % pm]
        n_pairs = sum(e["digest_audits"]) + sum(e["verdict_audits"])
        us_pair = 2e-3 * sum(e["audit_ns"]) / n_pairs if n_pairs else None
        n_nym = sum(s["nym_audits"])
        figures["permille_%d" % pm] = {
            "nym_audits_per_block": n_nym / (a.runs * a.blocks),
            "p256_microseconds_per_digest_plus_verdict_audit": us_pair,
            "microseconds_per_pseudonym_audit": 1e-3 * (sum(s["audit_ns"]) - sum(e["audit_ns"])) / n_nym + us_pair if n_nym and us_pair else None,
            "audit_ms_per_block": statistics.median(s["audit_ms_per_block"]),
            "added_validators_ms_per_block_over_permille_0": s["median"] - I["audit_permille_0"]["median"],
            "p256_only_block_added_validators_ms_per_block": e["median"] - E["audit_permille_0"]["median"]}
    doc["figures"] = figures
    if a.parent_exe:
        p, z = E["parent_commit"], E["audit_permille_0"]
        doc["permille_0_within_parent_spread"] = {"parent_min": p["min"], "parent_max": p["max"], "permille_0_median": z["median"],
                                                  "within": p["min"] <= z["median"] <= p["max"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
