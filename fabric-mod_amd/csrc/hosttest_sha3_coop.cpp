// Stand-alone host program over the array instantiation of sha3_coop.h (its own main; built by the Makefile as ../lib/hosttest_sha3_coop,
// and as ../lib/hosttest_sha3_coop_san with -fsanitize=address,undefined by `make sanitize-sha3-coop`).
// The 32-lanes-per-message SHA3-256 of the kernels, with a 32-entry array where they have a half-wavefront, against the one-lane host
// sha3_256 of sha3_256.h over the concatenated message.
// Cases on stdin, one per line:  buffer-hex sa la sb lb  ("-" for an empty buffer): the message is  buffer[sa, sa + la) || buffer[sb, sb + lb),
// as tests/test_sha3_coop_host.py writes them.  Per case it prints the array model's digest and the one-lane digest, side by side.
// With the argument `self` it runs its own grid instead: every length around the block boundaries at the four byte phases, and prefixes
// that put the seam at the ends and in the middle of a block.  Exit status 1 when any pair of digests differs.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "sha3_coop.h"

using namespace fab;

static int n_cases = 0, n_differ = 0;

static void hex32(const uint8_t* d, char* out) {
    for (int i = 0; i < 32; i++) sprintf(out + 2 * i, "%02x", d[i]);
}

static void run_case(const std::vector<uint8_t>& buf, uint32_t sa, uint32_t la, uint32_t sb, uint32_t lb, bool print) {
    uint8_t coop[32], one[32];
    // (the buffer is copied to its exact size: a read outside it is the sanitizer's to see)
    std::vector<uint8_t> exact(buf);
    sha3_256_coop_host(exact.data(), exact.size(), sa, la, sb, lb, coop);
    std::vector<uint8_t> msg;
    msg.insert(msg.end(), exact.begin() + sa, exact.begin() + sa + la);
    msg.insert(msg.end(), exact.begin() + sb, exact.begin() + sb + lb);
    sha3_256_host(msg.data(), msg.size(), one);
    n_cases++;
    const bool differ = memcmp(coop, one, 32) != 0;
    if (differ) n_differ++;
    if (print || differ) {
        char a[65], b[65];
        hex32(coop, a);
        hex32(one, b);
        printf("%s %s%s\n", a, b, differ ? " DIFFER" : "");
    }
}

static void self_grid() {
    std::vector<uint8_t> buf(5000);
    uint32_t x = 0x9E3779B9u;
    for (auto& b : buf) {
        x = x * 1664525u + 1013904223u;
        b = (uint8_t)(x >> 24);
    }
    std::vector<uint32_t> lens;
    for (uint32_t v : {0u, 1u, 7u, 8u, 9u}) lens.push_back(v);
    for (uint32_t blocks = 1; blocks <= 3; blocks++)
        for (uint32_t v = blocks * 136 - 2; v <= blocks * 136 + 2; v++) lens.push_back(v);
    lens.push_back(14 * 136 - 1);
    lens.push_back(14 * 136);
    lens.push_back(14 * 136 + 1);
    for (uint32_t len : lens)
        for (uint32_t phase = 0; phase < 4; phase++) run_case(buf, 0, 0, 8 + phase, len, false);
    for (uint32_t pl : {0u, 1u, 135u, 136u, 137u, 300u})
        for (uint32_t len : lens)
            for (uint32_t phase = 0; phase < 4; phase++) run_case(buf, 3001 + phase, pl, 9 + (phase ^ 1u), len, false);
    // the last message ends on the buffer's last byte, the buffer's size at every residue mod 4
    for (uint32_t cut = 0; cut < 4; cut++) {
        std::vector<uint8_t> b2(buf.begin(), buf.begin() + 700 + cut);
        run_case(b2, 0, 0, 300, (uint32_t)b2.size() - 300, false);
        run_case(b2, 2, 137, 301, (uint32_t)b2.size() - 301, false);
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "self")) {
        self_grid();
    } else {
        std::string line;
        int c;
        auto flush = [&]() {
            if (line.empty()) return true;
            std::vector<char> hex(line.size() + 1);
            unsigned sa, la, sb, lb;
            if (sscanf(line.c_str(), "%s %u %u %u %u", hex.data(), &sa, &la, &sb, &lb) != 5) {
                fprintf(stderr, "hosttest_sha3_coop: malformed case: %.60s\n", line.c_str());
                return false;
            }
            std::vector<uint8_t> buf;
            if (strcmp(hex.data(), "-") != 0) {
                const size_t hl = strlen(hex.data());
                if (hl % 2) return false;
                for (size_t i = 0; i < hl; i += 2) {
                    unsigned v;
                    if (sscanf(hex.data() + i, "%2x", &v) != 1) return false;
                    buf.push_back((uint8_t)v);
                }
            }
            if ((uint64_t)sa + la > buf.size() || (uint64_t)sb + lb > buf.size()) {
                fprintf(stderr, "hosttest_sha3_coop: a span leaves its buffer\n");
                return false;
            }
            run_case(buf, sa, la, sb, lb, true);
            line.clear();
            return true;
        };
        while ((c = getchar()) != EOF) {
            if (c == '\n') {
                if (!flush()) return 2;
            } else {
                line.push_back((char)c);
            }
        }
        if (!flush()) return 2;
    }
    fprintf(stderr, "hosttest_sha3_coop: %d cases, %d disagreements\n", n_cases, n_differ);
    return n_differ ? 1 : 0;
}
