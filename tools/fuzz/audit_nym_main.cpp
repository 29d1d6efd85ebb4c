// The CPU audit's pseudonym-signature verification (fabric-mod_amd/csrc/audit_host.h audit_nym_verify) under AddressSanitizer and
// UndefinedBehaviorSanitizer, stand-alone:
//   audit_nym_main <vectors file> [mutants]
// The vectors file is flat text, one vector per line:  hsk_x hsk_y hrand_x hrand_y ipk_hash nym_x nym_y signature message expect
// (hex; "-" for an empty byte string; 0 / 1), written by tools/fuzz/run_audit_nym.sh from the committed known answers
// (tests/golden/idemix_nym_kats.json, each with a twin whose message has one bit flipped) with oracle/idemix_oracle.py as the
// expectation.  Every vector must get its expectation; then `mutants` (default 3 000) mutated signatures - bit flips, random bytes,
// length bytes, truncation, insertion, each in an exact-size heap block beside an exact-size message - go through audit_nym_verify:
// nothing may be read out of bounds, and a mutant that is accepted must still unmarshal to four 32-byte fields.  Host only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "audit_host.h"
#include "idemix_host.h"
using namespace fab::bccsp;

static std::vector<uint8_t> unhex(const std::string& s) {
    if (s == "-") return {};
    std::vector<uint8_t> b(s.size() / 2);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return b;
}
struct Vec {
    std::vector<uint8_t> f[7], sig, msg;       // hsk_x hsk_y hrand_x hrand_y ipk_hash nym_x nym_y
    bool expect;
};
// the call on exact-size heap copies: a read past either end is the sanitizer's to catch
static bool run(const Vec& v, const std::vector<uint8_t>& sig) {
    uint8_t* s = (uint8_t*)malloc(sig.size() ? sig.size() : 1);
    uint8_t* m = (uint8_t*)malloc(v.msg.size() ? v.msg.size() : 1);
    uint8_t* k[7];
    for (int i = 0; i < 7; i++) {
        k[i] = (uint8_t*)malloc(32);
        memcpy(k[i], v.f[i].data(), 32);
    }
    if (!sig.empty()) memcpy(s, sig.data(), sig.size());
    if (!v.msg.empty()) memcpy(m, v.msg.data(), v.msg.size());
    const bool ok = audit_nym_verify(k[0], k[1], k[2], k[3], k[4], k[5], k[6], s, sig.size(), m, v.msg.size());
    for (int i = 0; i < 7; i++) free(k[i]);
    free(s);
    free(m);
    return ok;
}
int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: audit_nym_main <vectors file> [mutants]\n"); return 2; }
    const long mutants = argc > 2 ? atol(argv[2]) : 3000;
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<Vec> vs;
    static char w[9][20000];
    int e;
    while (fscanf(f, "%19999s %19999s %19999s %19999s %19999s %19999s %19999s %19999s %19999s %d", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], &e) == 10) {
        Vec v;
        for (int i = 0; i < 7; i++) {
            v.f[i] = unhex(w[i]);
            if (v.f[i].size() != 32) { printf("a field of the vectors file is not 32 bytes\n"); return 2; }
        }
        v.sig = unhex(w[7]);
        v.msg = unhex(w[8]);
        v.expect = e != 0;
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
    std::mt19937_64 rng(23);
    size_t mut_accepted = 0;
    for (long it = 0; it < mutants; it++) {
        const Vec& v = *good[rng() % good.size()];
        std::vector<uint8_t> s = v.sig;
        const int k = 1 + rng() % 3;
        for (int j = 0; j < k && !s.empty(); j++) {
            const size_t pos = rng() % s.size();
            const size_t field = 34 * (size_t)(rng() % 4);                   // where a field of the unmutated signature starts: tag, length, 32 bytes
            switch (rng() % 6) {
                case 0: s[pos] ^= (uint8_t)(1u << (rng() % 8)); break;
                case 1: s[pos] = (uint8_t)rng(); break;
                case 2: if (field + 1 < s.size()) s[field + 1] = (uint8_t)rng(); break;     // a length byte
                case 3: s.resize(s.size() - rng() % (s.size() < 40 ? s.size() : 40)); break;
                case 4: if (field < s.size()) s[field] = (uint8_t)rng(); break;             // a tag
                default: s.insert(s.begin() + pos, (uint8_t)rng()); break;
            }
        }
        if (run(v, s)) {
            NymSignatureFields sf;
            if (!UnmarshalNymSignature(s.data(), s.size(), sf) || sf.len[0] != 32 || sf.len[1] != 32 || sf.len[2] != 32 || sf.len[3] != 32) {
                printf("MUTANT %ld accepted although the gates refuse it\n", it);
                return 1;
            }
            mut_accepted++;
        }
    }
    printf("audit_nym_main: %zu vectors as expected (%zu accepted), %ld mutated signatures (%zu still accepted): no finding\n", vs.size(), accepted, mutants, mut_accepted);
    return 0;
}
