// Stand-alone host program over the host compilation of p384_tables.h (its own main; built by the Makefile as
// ../lib/hosttest_p384_keyed, and as ../lib/hosttest_p384_keyed_san with -fsanitize=address,undefined by `make sanitize-p384-keyed`).
// It reads the tuples of a vector file - one per line: qx qy e r s status, hex, as tests/test_p384_keyed_host.py writes them from
// tests/golden/p384_kats.json and its exceptional rows - builds the comb table of every distinct key once, and runs each tuple
// through the keyed verification core (a key off the curve gets no table: its rows run on the generator's with key_ok = false, as the
// kernel's rows without a live key do).  Then the builder's invariants on the generator's table.  Exit status 0: all as expected.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "p384_tables.h"

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

int main(int argc, char** argv) {
    Table g;
    build_gcomb384(g.p);
    int bad = 0, n = 0;
    std::map<std::string, Table> tabs;
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
            const uint32_t* q = g.p;
            const bool key_ok = pubkey_on_curve(b[0], b[1]);
            if (key_ok) {
                std::string name((const char*)b[0], 48);
                name.append((const char*)b[1], 48);
                auto it = tabs.find(name);
                if (it == tabs.end()) {
                    it = tabs.try_emplace(name).first;
                    if (!build_comb384_be(it->second.p, b[0], b[1])) bad++;
                }
                q = it->second.p;
            }
            const uint32_t st = verify_keyed_host(g.p, q, b[2], b[3], b[4], key_ok);
            if ((int)st != want) {
                fprintf(stderr, "tuple %d: status %u, expected %d\n", n, st, want);
                bad++;
            }
            n++;
        }
        fclose(f);
    }
    // the generator's table: entry 0 of every window zero, every other entry a point of the curve, T[0][j] = j G as build_gtab makes
    // them, and T[w + 1][1] = 256 T[w][1] by eight doublings
    std::vector<uint32_t> gtab(P384_GTAB_WORDS);
    build_gtab(gtab.data());
    const CombPtr384 gc{g.p};
    const u384 one = FAB_P384_ONE_MONT;
    for (uint32_t w = 0; w < (uint32_t)CombTab384::WINDOWS; w++) {
        for (int k = 0; k < CombTab384::ENTRY_WORDS; k++) bad += g.p[CombTab384::index(w, 0) + (size_t)k] ? 1 : 0;
        for (uint32_t d = 1; d < CombTab384::DIGITS; d++) {
            jac e;
            gc.load(e, w, d);
            bad += on_curve(e.X, e.Y) ? 0 : 1;
        }
        if (w + 1 < (uint32_t)CombTab384::WINDOWS) {
            jac a, nx, t;
            gc.load(a, w, 1);
            gc.load(nx, w + 1, 1);
            for (int k = 0; k < 8; k++) {
                pt_dbl(t, a);
                a = t;
            }
            u384 zz, zzz, x, y;                  // a == nx: X = x Z^2, Y = y Z^3
            fp_sqr(zz, a.Z);
            fp_mul(zzz, zz, a.Z);
            fp_mul(x, nx.X, zz);
            fp_mul(y, nx.Y, zzz);
            bad += eq384(x, a.X) && eq384(y, a.Y) && eq384(nx.Z, one) ? 0 : 1;
        }
    }
    for (uint32_t j = 1; j <= (uint32_t)P384_TAB_ENTRIES; j++) {
        jac a, b;
        gc.load(a, 0, j);
        GTabPtr{gtab.data()}.load(b, j);
        bad += eq384(a.X, b.X) && eq384(a.Y, b.Y) ? 0 : 1;
    }
    // the low byte of every window, in order
    u384 u;
    for (int i = 0; i < 12; i++) u.w[i] = 0x03020100u + 0x04040404u * (uint32_t)i;
    for (uint32_t w = 0; w < 48; w++) bad += take_low_byte(u) == w ? 0 : 1;
    bad += is_zero(u) ? 0 : 1;
    printf("hosttest_p384_keyed: %d tuples, %d failures (%zu keys)\n", n, bad, tabs.size());
    return bad ? 1 : 0;
}
