#!/bin/bash
# The provider's CPU audit of idemix pseudonym signatures (audit_host.cpp audit_nym_verify: the one-lane FP256BN commitment compiled
# for the host, the two challenge hashes, behind the NymSignature gates) under AddressSanitizer and UndefinedBehaviorSanitizer, as a
# stand-alone program: the committed known answers and their message twins with oracle/idemix_oracle.py as the expectation, then a few
# thousand mutated signatures.  Host only, no GPU; run by hand (it is not a pytest test):
#   tools/fuzz/run_audit_nym.sh [mutants]
set -e
cd "$(dirname "$0")/../.."
CXX=${CXX:-/opt/rocm/lib/llvm/bin/clang++}
SRC=fabric-mod_amd/csrc
FLAGS="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -std=c++17 -I$SRC -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__"
OUT=${TMPDIR:-/tmp}
python3 - "$OUT/audit_nym_kats.txt" <<'PY'
import json, os, sys
ROOT = os.getcwd()
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import idemix_oracle as io
fx = json.load(open(os.path.join(ROOT, "tests", "golden", "idemix_fixtures.json")))["msps"]
be32 = lambda x: x.to_bytes(32, "big").hex()
rows = []
for v in json.load(open(os.path.join(ROOT, "tests", "golden", "idemix_nym_kats.json")))["vectors"]:
    ipk = io.IssuerPublicKey(bytes.fromhex(fx[v["msp"]]["ipk"]))
    sig = {k: bytes.fromhex(v[k]) for k in ("proof_c", "proof_s_sk", "proof_s_r_nym", "nonce")}
    nym, msg = (int(v["nym_x"], 16), int(v["nym_y"], 16)), bytes.fromhex(v["msg"])
    twin = bytes([msg[0] ^ 0x40]) + msg[1:] if msg else b"\x01"
    for m in (msg, twin):
        rows.append(" ".join([be32(ipk.h_sk[0]), be32(ipk.h_sk[1]), be32(ipk.h_rand[0]), be32(ipk.h_rand[1]), bytes(ipk.hash).hex(), be32(nym[0]), be32(nym[1]),
                              io.nym_signature_marshal(sig).hex(), m.hex() or "-", str(int(io.nym_verify(sig, nym, ipk, m) == io.NYM_VALID))]))
open(sys.argv[1], "w").write("\n".join(rows) + "\n")
PY
# (bccsp_host.cpp comes along for the host gates audit_host.cpp shares with it; the device entry points it names besides those of
# stubs.cpp are never called by this program and stay unresolved)
$CXX $FLAGS tools/fuzz/audit_nym_main.cpp $SRC/audit_host.cpp $SRC/bccsp_host.cpp $SRC/block_prepass.cpp $SRC/idemix_host.cpp tools/fuzz/stubs.cpp -o "$OUT/audit_nym_main" -lpthread \
    -Wl,--unresolved-symbols=ignore-all
"$OUT/audit_nym_main" "$OUT/audit_nym_kats.txt" "${1:-3000}"
