#!/bin/bash
# The provider's CPU audit (audit_host.cpp: SHA-256 and the one-lane P-256 verification compiled for the host, behind the host gates)
# under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: the committed vectors - edge cases, DER encodings
# across digest lengths 1 / 32 / 40, RFC 6979, the reference's certificates - with the restated bccsp/sw as the expectation, then a
# few thousand mutated DER signatures.  Host only, no GPU; run by hand (it is not a pytest test):
#   tools/fuzz/run_audit.sh [mutants]
set -e
cd "$(dirname "$0")/../.."
CXX=${CXX:-/opt/rocm/lib/llvm/bin/clang++}
SRC=fabric-mod_amd/csrc
FLAGS="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -std=c++17 -I$SRC -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__"
OUT=${TMPDIR:-/tmp}
python3 - "$OUT/audit_kats.txt" <<'PY'
import hashlib, json, os, sys
ROOT = os.getcwd()
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bccsp_sw_oracle as po
G = os.path.join(ROOT, "tests", "golden")
load = lambda n: json.load(open(os.path.join(G, n)))
def want(qx, qy, sig, dg):
    if not po.on_curve(qx, qy):
        return False                                   # KeyImport refuses the key: it never reaches Verify
    try:
        return po.csp_verify((qx, qy), sig, dg)
    except po.BCCSPError:
        return False
rows = []
def add(qx, qy, sig, dg):
    if qx >> 256 or qy >> 256:
        return
    rows.append("%064x %064x %s %s %d" % (qx, qy, sig.hex() or "-", dg.hex() or "-", want(qx, qy, sig, dg)))
for v in load("edge_kats.json")["vectors"]:
    add(int(v["qx"], 16), int(v["qy"], 16), po.marshal_ecdsa_signature(int(v["r"], 16), int(v["s"], 16)), bytes.fromhex(v["e"]))
d = 1 + 5 * 7919
qx, qy = po.pt_mul(d, (po.GX, po.GY))
for v in load("der_kats.json")["vectors"]:
    for dg in (b"\x07", b"\x01" * 32, b"\xff" * 40):
        add(qx, qy, bytes.fromhex(v["der"]), dg)
for k, dg in enumerate((b"\x07", b"\x01" * 32, b"\xff" * 40)):
    add(qx, qy, po.marshal_ecdsa_signature(*po.sign_raw(d, dg, 0x5EED + k)), dg)
f = load("rfc6979_p256_sha256.json")
for v in f["vectors"]:
    r, s = int(v["r"], 16), int(v["s"], 16)
    for s_ in (s, po.N - s):
        add(int(f["qx"], 16), int(f["qy"], 16), po.marshal_ecdsa_signature(r, s_), hashlib.sha256(v["message"].encode()).digest())
for v in load("ref_cert_kats.json")["vectors"]:
    add(int(v["qx"], 16), int(v["qy"], 16), bytes.fromhex(v["sig_der"]), bytes.fromhex(v["e"]))
open(sys.argv[1], "w").write("\n".join(rows) + "\n")
PY
$CXX $FLAGS tools/fuzz/audit_kats.cpp $SRC/audit_host.cpp $SRC/bccsp_host.cpp $SRC/block_prepass.cpp $SRC/idemix_host.cpp tools/fuzz/stubs.cpp -o "$OUT/audit_kats" -lpthread
"$OUT/audit_kats" "$OUT/audit_kats.txt" "${1:-5000}"
