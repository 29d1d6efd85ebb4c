// Stand-alone host program over p256_odd4.h (u2_fold_odd, odd_digit4): the host compilation of the recoding the LDS-table pair kernels
// run.  Reads scalars from the file named on the command line (or stdin), one per line as 64 hex digits, and answers one line each:
//     <k as folded, 64 hex digits> <64 digits, window 0 first: sign and entry, e.g. +3 -0>
// Each digit is computed twice, by odd_digit4 and by the top-down walk the device loop uses (odd_walk4_next); a difference ends the program.
// tests/test_pair_odd_windows_host.py checks every answer against Python integers; `make sanitize-pair-odd` builds and runs this program
// with -fsanitize=address,undefined over its own cases.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "p256_odd4.h"

using namespace fab;

static bool parse(u256& r, const char* s) {
    if (strlen(s) < 64) return false;
    for (int w = 0; w < 8; w++) {
        uint32_t v = 0;
        for (int c = 0; c < 8; c++) {
            const char ch = s[(7 - w) * 8 + c];
            uint32_t d;
            if (ch >= '0' && ch <= '9') d = (uint32_t)(ch - '0');
            else if (ch >= 'a' && ch <= 'f') d = (uint32_t)(ch - 'a' + 10);
            else if (ch >= 'A' && ch <= 'F') d = (uint32_t)(ch - 'A' + 10);
            else return false;
            v = (v << 4) | d;
        }
        r.w[w] = v;
    }
    return true;
}

static void answer(const u256& u2) {
    u256 k;
    u2_fold_odd(k, u2);
    for (int w = 7; w >= 0; w--) printf("%08x", k.w[w]);
    uint32_t kw[9];
    for (int w = 0; w < 8; w++) kw[w] = k.w[w];
    kw[8] = 0;
    odd_digit walked[ODD4_WINDOWS];
    odd_walk4 wk;
    odd_walk4_start(wk, k);
    for (int i = ODD4_WINDOWS - 1; i >= 0; i--) walked[i] = odd_walk4_next(wk);
    for (int i = 0; i < ODD4_WINDOWS; i++) {
        const odd_digit d = odd_digit4(kw, i);
        if (d.entry != walked[i].entry || d.neg != walked[i].neg) {   // the device's walk and the indexed form must be one recoding
            printf(" walk differs at %d\n", i);
            exit(3);
        }
        printf(" %c%u", d.neg ? '-' : '+', d.entry);
    }
    printf("\n");
}

int main(int argc, char** argv) {
    FILE* in = stdin;
    if (argc > 1 && strcmp(argv[1], "self") == 0) {
        // the program's own cases (the sanitizer run): small, large and all-ones scalars
        const char* own[] = {"0000000000000000000000000000000000000000000000000000000000000001",
                             "0000000000000000000000000000000000000000000000000000000000000002",
                             "ffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc63254f",
                             "ffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632550",
                             "8000000000000000000000000000000000000000000000000000000000000000",
                             "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff"};
        for (const char* s : own) {
            u256 v;
            if (!parse(v, s)) return 2;
            answer(v);
        }
        return 0;
    }
    if (argc > 1 && !(in = fopen(argv[1], "r"))) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    char line[256];
    while (fgets(line, sizeof line, in)) {
        u256 v;
        if (!parse(v, line)) {
            fprintf(stderr, "bad line: %s", line);
            return 2;
        }
        answer(v);
    }
    if (in != stdin) fclose(in);
    return 0;
}
