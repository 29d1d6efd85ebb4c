// Stand-alone host program over the host compilation of p384_tables16.h (its own main; built by the Makefile as
// ../lib/hosttest_p384_tables16, and as ../lib/hosttest_p384_tables16_san with -fsanitize=address,undefined by
// `make sanitize-p384-tables16`).  It reads commands from stdin, one per line, as tests/test_p384_tables16_host.py writes them:
//   V qx qy e r s key_ok   one tuple through verify_core_keyed twice - on the 8-bit tables (48 windows) and through the 24-window
//                          instantiation (CombOnDemand384x16 over the same tables); prints "<48-window status> <24-window status>".
//                          key_ok 0: the row names no live key and runs on the generator's comb.
//   T qx qy w d            entry d of window w of the key's 16-bit table as build_comb384x16 stores it (the window is built whole, once);
//                          prints "x y" as plain integers in hex, "0 0" for the all-zero entry.
// All numbers are hex.  Without input (an empty stdin) the program runs cases of its own: windows 0 and 23 of the generator's table
// against the on-demand comb and the copies of the 8-bit entries.
// Exit status 0: every line was read (and, for V, both columns agree; for the own cases, everything matched); 1: a disagreement;
// 2: bad input.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "p384_tables16.h"

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

// words in 16-byte aligned memory
struct Words {
    std::vector<uint32_t> raw;
    uint32_t* p;
    explicit Words(size_t n) : raw(n + 4), p(raw.data() + ((16 - ((uintptr_t)raw.data() & 15)) & 15) / 4) {}
    Words(const Words&) = delete;
};

static void print_plain(const uint32_t* mont12) {
    u384 m, v;
    for (int k = 0; k < 12; k++) m.w[k] = mont12[k];
    fp_from_mont(v, m);
    uint8_t be[48];
    to_be48(be, v);
    for (int i = 0; i < 48; i++) printf("%02x", be[i]);
}

static int own_cases(const uint32_t* g8) {
    int bad = 0;
    const CombOnDemand384x16 od{g8};
    Words win(CombTab384x16::WINDOW_WORDS);
    const uint32_t ws[2] = {0, 23};
    const uint32_t ds[] = {1, 2, 0x00FF, 0x0100, 0x0101, 0x7FFF, 0x8000, 0xFF00, 0xFFFF};
    for (uint32_t w : ws) {
        build_comb384x16(g8, w, w + 1, win.p);
        for (int k = 0; k < CombTab384x16::ENTRY_WORDS; k++) bad += win.p[k] != 0;
        for (uint32_t d : ds) {
            jac t;
            od.load(t, w, d);
            const uint32_t* e = win.p + (size_t)d * CombTab384x16::ENTRY_WORDS;
            for (int k = 0; k < 12; k++) bad += (e[k] != t.X.w[k]) + (e[12 + k] != t.Y.w[k]);
        }
    }
    fprintf(stderr, "hosttest_p384_tables16: own cases, %d words differ\n", bad);
    return bad ? 1 : 0;
}

int main() {
    Words g(CombTab384::TABLE_WORDS);
    build_gcomb384(g.p);
    std::map<std::string, Words> tabs;
    std::map<std::pair<std::string, uint32_t>, Words> wins;
    auto table_of = [&](const uint8_t* qx, const uint8_t* qy) -> const uint32_t* {
        std::string name((const char*)qx, 48);
        name.append((const char*)qy, 48);
        auto it = tabs.find(name);
        if (it == tabs.end()) {
            it = tabs.try_emplace(name, CombTab384::TABLE_WORDS).first;
            if (!build_comb384_be(it->second.p, qx, qy)) return nullptr;
        }
        return it->second.p;
    };
    int n = 0, differ = 0;
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        char a[5][128];
        uint8_t b[5][48];
        if (cmd[0] == 'V' && cmd[1] == 0) {
            int key_ok;
            if (scanf("%127s %127s %127s %127s %127s %d", a[0], a[1], a[2], a[3], a[4], &key_ok) != 6) return 2;
            bool ok = true;
            for (int k = 0; k < 5; k++) ok = ok && hex48(a[k], b[k]);
            const uint32_t* q = !ok ? nullptr : key_ok ? table_of(b[0], b[1]) : g.p;
            if (!q) {
                fprintf(stderr, "line %d: bad hex, or the key is not a point of the curve\n", n);
                return 2;
            }
            const uint32_t s48 = verify_keyed_host(g.p, q, b[2], b[3], b[4], key_ok != 0);
            const uint32_t s24 = verify_keyed16_host(g.p, q, b[2], b[3], b[4], key_ok != 0);
            printf("%u %u\n", s48, s24);
            differ += s48 != s24 ? 1 : 0;
        } else if (cmd[0] == 'T' && cmd[1] == 0) {
            unsigned w, d;
            if (scanf("%127s %127s %x %x", a[0], a[1], &w, &d) != 4 || w >= (unsigned)CombTab384x16::WINDOWS || d >= CombTab384x16::DIGITS) return 2;
            const uint32_t* q = hex48(a[0], b[0]) && hex48(a[1], b[1]) ? table_of(b[0], b[1]) : nullptr;
            if (!q) {
                fprintf(stderr, "line %d: bad hex, or the key is not a point of the curve\n", n);
                return 2;
            }
            std::string name((const char*)b[0], 48);
            name.append((const char*)b[1], 48);
            auto it = wins.find({name, w});
            if (it == wins.end()) {
                it = wins.try_emplace({name, w}, CombTab384x16::WINDOW_WORDS).first;
                build_comb384x16(q, w, w + 1, it->second.p);
            }
            const uint32_t* e = it->second.p + (size_t)d * CombTab384x16::ENTRY_WORDS;
            bool zero = true;
            for (int k = 0; k < CombTab384x16::ENTRY_WORDS; k++) zero = zero && e[k] == 0;
            if (zero) {
                printf("0 0\n");
            } else {
                print_plain(e);
                printf(" ");
                print_plain(e + 12);
                printf("\n");
            }
        } else {
            fprintf(stderr, "line %d: unknown command\n", n);
            return 2;
        }
        n++;
    }
    if (!feof(stdin)) return 2;
    if (n == 0) return own_cases(g.p);
    fprintf(stderr, "hosttest_p384_tables16: %d lines, %d disagreements (%zu keys, %zu windows)\n", n, differ, tabs.size(), wins.size());
    return differ ? 1 : 0;
}
