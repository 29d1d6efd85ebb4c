#!/usr/bin/env python3
"""What the provider's sampled CPU audit costs the validators: tools/go_call_replay.c on the 10 000-transaction block of the block-pass
benches at --audit-permille 0, 1 and 10, `--runs` fresh processes each, and - with --parent-exe, a go_call_replay built from the
commit before the audit existed (it links its own libfabgpu.so next to it) - the same block through that build, which gives the
run-to-run spread the permille-0 figure has to lie within.  Writes one JSON document (default profiles/audit_cost.json):
validators_ms_per_block of every run, the audit's own nanosecond counter and its audit counts.  Needs a GPU.
    python tools/audit_cost.py [--parent-exe PATH] [--runs 3] [--blocks 12] [--threads 16] [--out profiles/audit_cost.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def replay(exe, block, blocks, threads, permille=None):
    cmd = [exe] + ([] if permille is None else ["--audit-permille", str(permille)]) + [block, str(blocks), str(threads), "1", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not line:
        raise SystemExit("%s: rc %d: %s" % (" ".join(cmd), r.returncode, (r.stderr or r.stdout)[-400:]))
    return json.loads(line[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-exe")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tx", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audit_cost.json"))
    a = ap.parse_args()
    block = os.path.join(ROOT, ".bench_blocks", "friendly_%d.bin" % a.tx)
    if not os.path.exists(block):
        sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "fabric-mod_amd")]
        import blockgen
        os.makedirs(os.path.dirname(block), exist_ok=True)
        open(block, "wb").write(blockgen.endorser_block(a.tx, 1)[0])
    exe = os.path.join(ROOT, "fabric-mod_amd", "lib", "go_call_replay")
    doc = {"what": "tools/go_call_replay.c, %d blocks of %d transactions, %d validator threads, %d fresh processes per setting; "
                   "validators_ms_per_block = the validators' CPU residue per block (median over the blocks of a run)" % (a.blocks, a.tx, a.threads, a.runs),
           "settings": {}}

    def summarise(runs):
        v = [r["validators_ms_per_block_median"] for r in runs]
        e = {"validators_ms_per_block": v, "median": statistics.median(v), "min": min(v), "max": max(v),
             "ms_per_block_end_to_end": [r["ms_per_block_end_to_end"] for r in runs]}
        if "audit" in runs[0]:
            e["audit_ns_per_run"] = [r["audit"]["audit_ns"] for r in runs]
            e["audit_ms_per_block"] = [r["audit"]["audit_ms_per_block"] for r in runs]
            for k in ("digest_audits", "verdict_audits", "direct_audits", "mismatches", "skipped_nym", "poisoned"):
                e[k] = [r["audit"][k] for r in runs]
            n = sum(r["audit"]["digest_audits"] + r["audit"]["verdict_audits"] for r in runs)
            e["microseconds_per_audit_pair"] = 2e-3 * sum(e["audit_ns_per_run"]) / n if n else None
        return e
    # interleaved, so that drift of the machine falls on every setting alike
    runs = {"parent": [], "0": [], "1": [], "10": []}
    for _ in range(a.runs):
        if a.parent_exe:
            runs["parent"].append(replay(a.parent_exe, block, a.blocks, a.threads))
        for pm in (0, 1, 10):
            runs[str(pm)].append(replay(exe, block, a.blocks, a.threads, pm))
    if a.parent_exe:
        doc["settings"]["parent_commit"] = summarise(runs["parent"])
    for pm in (0, 1, 10):
        doc["settings"]["audit_permille_%d" % pm] = summarise(runs[str(pm)])
    if a.parent_exe:
        p, z = doc["settings"]["parent_commit"], doc["settings"]["audit_permille_0"]
        doc["permille_0_within_parent_spread"] = {"parent_min": p["min"], "parent_max": p["max"], "permille_0_median": z["median"],
                                                  "within": p["min"] <= z["median"] <= p["max"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
