// The provider's CPU audit (fabric-mod_amd/csrc/audit_host.h) under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone:
//   audit_kats <vectors file> [mutants]
// The vectors file is flat text, one vector per line:  qx qy signature digest expect  (hex, hex, hex DER, hex, 0 / 1), written by
// tools/fuzz/run_audit.sh from the committed fixtures with the restated bccsp/sw as the expectation.  Every vector must get its
// expectation; then `mutants` (default 5 000) mutated DER signatures - bit flips, random bytes, long-form length bytes, truncation,
// each in an exact-size heap block - go through audit_p256_verify: nothing may be read out of bounds, and a mutant that is accepted
// must be one the host's unmarshaller takes.  The SHA-256 is run over every length 0 .. 300 from exact-size blocks.  Host only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "audit_host.h"
#include "bccsp_host.h"
using namespace fab::bccsp;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> b(s.size() / 2);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return b;
}
struct Vec {
    std::vector<uint8_t> qx, qy, sig, dg;
    bool expect;
};
// the call on exact-size heap copies: a read past either end is the sanitizer's to catch
static bool run(const Vec& v, const std::vector<uint8_t>& sig) {
    uint8_t* s = (uint8_t*)malloc(sig.size() ? sig.size() : 1);
    uint8_t* d = (uint8_t*)malloc(v.dg.size() ? v.dg.size() : 1);
    if (!sig.empty()) memcpy(s, sig.data(), sig.size());
    if (!v.dg.empty()) memcpy(d, v.dg.data(), v.dg.size());
    const bool ok = audit_p256_verify(v.qx.data(), v.qy.data(), s, sig.size(), d, v.dg.size());
    free(s);
    free(d);
    return ok;
}
int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: audit_kats <vectors file> [mutants]\n"); return 2; }
    const long mutants = argc > 2 ? atol(argv[2]) : 5000;
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<Vec> vs;
    static char a[4096], b[4096], c[4096], d[4096];
    int e;
    while (fscanf(f, "%4095s %4095s %4095s %4095s %d", a, b, c, d, &e) == 5) {
        Vec v{unhex(a), unhex(b), unhex(strcmp(c, "-") ? c : ""), unhex(strcmp(d, "-") ? d : ""), e != 0};
        if (v.qx.size() != 32 || v.qy.size() != 32) { printf("bad key length in the vectors file\n"); return 2; }
        vs.push_back(v);
    }
    fclose(f);
    size_t accepted = 0;
    for (size_t i = 0; i < vs.size(); i++) {
        const bool got = run(vs[i], vs[i].sig);
        if (got != vs[i].expect) { printf("VECTOR %zu: audit says %d, expected %d\n", i, (int)got, (int)vs[i].expect); return 1; }
        accepted += got;
    }
    std::vector<const Vec*> good;
    for (const Vec& v : vs)
        if (v.expect) good.push_back(&v);
    if (good.empty()) { printf("no accepted vector to mutate\n"); return 2; }
    std::mt19937_64 rng(17);
    size_t mut_accepted = 0;
    for (long it = 0; it < mutants; it++) {
        const Vec& v = *good[rng() % good.size()];
        std::vector<uint8_t> s = v.sig;
        const int k = 1 + rng() % 4;
        for (int j = 0; j < k && !s.empty(); j++) {
            const size_t pos = rng() % s.size();
            switch (rng() % 5) {
                case 0: s[pos] ^= (uint8_t)(1u << (rng() % 8)); break;
                case 1: s[pos] = (uint8_t)rng(); break;
                case 2: s[pos] = (uint8_t)(0x80 | (rng() % 5)); break;   // long-form / indefinite lengths
                case 3: s.resize(s.size() - rng() % (s.size() < 8 ? s.size() : 8)); break;
                default: s.insert(s.begin() + pos, (uint8_t)rng()); break;
            }
        }
        if (run(v, s)) {
            BigInt R, S;
            if (!UnmarshalECDSASignature(s.data(), s.size(), R, S).ok() || !IsLowS(S)) { printf("MUTANT %ld accepted although the gates refuse it\n", it); return 1; }
            mut_accepted++;
        }
    }
    for (size_t n = 0; n <= 300; n++) {                       // SHA-256 over exact-size blocks: the padding never reads past the message
        uint8_t* m = (uint8_t*)malloc(n ? n : 1);
        for (size_t i = 0; i < n; i++) m[i] = (uint8_t)(i * 131 + n);
        uint8_t out[32], again[32];
        audit_sha256(m, n, out);
        audit_sha256(m, n, again);
        free(m);
        if (memcmp(out, again, 32) != 0) { printf("SHA-256 not deterministic at length %zu\n", n); return 1; }
    }
    printf("audit_kats: %zu vectors as expected (%zu accepted), %ld mutated signatures (%zu still accepted), SHA-256 lengths 0..300: no finding\n", vs.size(),
           accepted, mutants, mut_accepted);
    return 0;
}
