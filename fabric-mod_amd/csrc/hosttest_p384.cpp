// Stand-alone host program over the host compilation of p384.h (its own main; built by the Makefile as ../lib/hosttest_p384, and as
// ../lib/hosttest_p384_san with -fsanitize=address,undefined by `make sanitize-p384`).  It reads the tuples of a vector file - one tuple
// per line: qx qy e r s status, hex, as tests/test_p384_host.py writes them from tests/golden/p384_kats.json - and runs each through
// the verification core; then a fixed set of edge operands through the field, scalar and point primitives, where the sanitizers look
// for out-of-range shifts, signed overflow and stray array indices.  Exit status 0: every status as expected.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "p384.h"

using namespace fab::p384;

static bool hex48(const char* h, uint8_t* out) {
    const size_t n = strlen(h);
    if (n == 0 || n > 96) return false;
    char buf[97];
    memset(buf, '0', 96);
    memcpy(buf + 96 - n, h, n);
    buf[96] = 0;
    for (int i = 0; i < 48; i++) {
        unsigned v;
        if (sscanf(buf + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}

int main(int argc, char** argv) {
    std::vector<uint32_t> gtab(P384_GTAB_WORDS);
    build_gtab(gtab.data());
    int bad = 0, n = 0;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        char a[5][128];
        int want;
        while (fscanf(f, "%127s %127s %127s %127s %127s %d", a[0], a[1], a[2], a[3], a[4], &want) == 6) {
            uint8_t b[5][48];
            bool ok = true;
            for (int k = 0; k < 5; k++) ok = ok && hex48(a[k], b[k]);
            if (!ok) {
                fprintf(stderr, "line %d: bad hex\n", n + 1);
                return 2;
            }
            const uint32_t st = verify_host(gtab.data(), b[0], b[1], b[2], b[3], b[4]);
            if ((int)st != want) {
                fprintf(stderr, "tuple %d: status %u, expected %d\n", n, st, want);
                bad++;
            }
            n++;
        }
        fclose(f);
    }
    // edge operands through every primitive (results are folded into one word so that nothing is optimised away)
    const u384 P = FAB_P384_P, N = FAB_P384_N, one = FAB_P384_ONE_MONT;
    u384 pm1, nm1, allones, t, acc = zero384();
    u384 unit = zero384();
    unit.w[0] = 1;
    sub384(pm1, P, unit);
    sub384(nm1, N, unit);
    for (int i = 0; i < 12; i++) allones.w[i] = 0xFFFFFFFFu;
    const u384 ops[5] = {zero384(), unit, pm1, nm1, one};
    for (const u384& x : ops)
        for (const u384& y : ops) {
            fp_mul(t, x, y); add384(acc, acc, t);
            fp_add(t, x, y); add384(acc, acc, t);
            fp_sub(t, x, y); add384(acc, acc, t);
            if (lt384(x, N) && lt384(y, N)) { fn_mul(t, x, y); add384(acc, acc, t); }
        }
    fn_reduce_once(t, allones); add384(acc, acc, t);
    fn_inv(t, nm1); add384(acc, acc, t);
    fn_inv(t, zero384()); add384(acc, acc, t);
    jac G, D, S, I = pt_infinity();
    G.X = FAB_P384_GX_MONT; G.Y = FAB_P384_GY_MONT; G.Z = one;
    pt_dbl(D, G);
    pt_add<false>(S, D, G);
    pt_add<true>(S, S, G);
    pt_add<false>(S, G, G);                       // P + P
    bad += eq384(S.X, D.X) && eq384(S.Y, D.Y) && eq384(S.Z, D.Z) ? 0 : 1;
    jac NG = G;
    fp_sub(NG.Y, zero384(), G.Y);
    pt_add<true>(S, G, NG);                       // P + (-P)
    bad += is_zero(S.Z) ? 0 : 1;
    pt_add<false>(S, I, G);
    bad += eq384(S.X, G.X) ? 0 : 1;
    pt_add<false>(S, G, I);
    bad += eq384(S.X, G.X) ? 0 : 1;
    pt_dbl(S, I);
    bad += is_zero(S.Z) ? 0 : 1;
    uint8_t e48[48], dg[64];
    for (int i = 0; i < 64; i++) dg[i] = (uint8_t)(i + 1);
    const size_t lens[4] = {20, 32, 48, 64};
    for (size_t len : lens) {
        hash_to_int(dg, len, e48);
        bad += e48[47] == (len > 48 ? 48 : (uint8_t)len) ? 0 : 1;
    }
    printf("hosttest_p384: %d tuples, %d failures (fold %08x)\n", n, bad, acc.w[0]);
    return bad ? 1 : 0;
}
