// Stand-alone host program over the host compilation of p384_wide.h (its own main; built by the Makefile as ../lib/hosttest_p384_wide,
// and as ../lib/hosttest_p384_wide_san with -fsanitize=address,undefined by `make sanitize-p384-wide`).
// It reads cases from stdin - one per line: qx qy e r s key_ok, hex and 0 / 1, as tests/test_p384_wide_host.py writes them from
// tests/p384_wide_cases.py - builds the comb table of every distinct key once, and prints per case the status of verify_core_keyed
// (one chain of 96 additions) and of verify_core_keyed_split (the eight partial sums and the tree of p384_wide_kernels.hip), side by
// side: "<one-lane> <split>".  key_ok 0: the row names no live key - it runs on the generator's comb, as the kernels' rows do.
// Exit status 0: every line was read and both columns agree; 1: a disagreement; 2: bad input.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "p384_wide.h"

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

// a table in 16-byte aligned memory
struct Table {
    std::vector<uint32_t> raw;
    uint32_t* p;
    Table() : raw(CombTab384::TABLE_WORDS + 4), p(raw.data() + ((16 - ((uintptr_t)raw.data() & 15)) & 15) / 4) {}
    Table(const Table&) = delete;
};

int main() {
    Table g;
    build_gcomb384(g.p);
    std::map<std::string, Table> tabs;
    int n = 0, differ = 0;
    char a[5][128];
    int key_ok;
    while (scanf("%127s %127s %127s %127s %127s %d", a[0], a[1], a[2], a[3], a[4], &key_ok) == 6) {
        uint8_t b[5][48];
        bool ok = true;
        for (int k = 0; k < 5; k++) ok = ok && hex48(a[k], b[k]);
        if (!ok) {
            fprintf(stderr, "case %d: bad hex\n", n);
            return 2;
        }
        const uint32_t* q = g.p;
        if (key_ok) {
            std::string name((const char*)b[0], 48);
            name.append((const char*)b[1], 48);
            auto it = tabs.find(name);
            if (it == tabs.end()) {
                it = tabs.try_emplace(name).first;
                if (!build_comb384_be(it->second.p, b[0], b[1])) {
                    fprintf(stderr, "case %d: the key is not a point of the curve\n", n);
                    return 2;
                }
            }
            q = it->second.p;
        }
        const uint32_t one = verify_keyed_host(g.p, q, b[2], b[3], b[4], key_ok != 0);
        const uint32_t split = verify_keyed_split_host(g.p, q, b[2], b[3], b[4], key_ok != 0);
        printf("%u %u\n", one, split);
        differ += one != split ? 1 : 0;
        n++;
    }
    if (!feof(stdin)) {
        fprintf(stderr, "case %d: malformed line\n", n);
        return 2;
    }
    fprintf(stderr, "hosttest_p384_wide: %d cases, %d disagreements (%zu keys)\n", n, differ, tabs.size());
    return differ ? 1 : 0;
}
