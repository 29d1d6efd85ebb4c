// Stand-alone host program over DescribedPlan (described_plan.h; its own main; built by the Makefile as ../lib/hosttest_described_plan,
// and as ../lib/hosttest_described_plan_san with -fsanitize=address,undefined by `make sanitize-described-plan`).  The plan is a pure
// function of offsets, so it runs here without a context and without a device, in the order the entry points feed it: rows, pseudonym
// rows, prefixes, gathered pieces, close, rebase.
//
// A script on stdin, one description per line, numbers in decimal or 0x hex; one answer line per description on stdout.
//     PLACE SPANS PREFIX_IN_TAIL TAIL TAIL_BASE TAIL_LEN N M NN NG  off...  pre_off...  nym_off...  gather_spans...
//         PLACE           arena | own      where the tail lies on the device (DescribedPlan::Tail)
//         SPANS           0 | 1            off / pre_off hold pairs (N and M pairs) or consecutive offsets (N + 1, and M + 1 if M != 0)
//         PREFIX_IN_TAIL  0 | 1            may_be_tail of the prefix rows (no entry point passes 1)
//         TAIL            0 | 1            the batch has a tail pointer
//         nym_off: NN pairs; gather_spans: NG x 3 pairs
//     -> refused RC
//     -> ok LO HI TAIL_USED GATHER_TOTAL | rebased off | rebased pre_off | rebased nym_off | rebased gather_spans
// tests/test_described_plan_host.py writes such scripts from a model of its own and compares every number.  Each array lives in a heap
// buffer of exactly its length, so that a read or write past its end is the sanitizer's to see.
// With the argument `self`: the program's own cases, one of each refusal and closing rule, each with the answer it must get.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "described_plan.h"

using fab::DescribedPlan;

namespace {
bool take(std::istringstream& ss, std::vector<uint32_t>& v, size_t k) {
    v.resize(k);
    v.shrink_to_fit();
    for (size_t i = 0; i < k; i++) {
        std::string t;
        if (!(ss >> t)) return false;
        v[i] = (uint32_t)std::stoull(t, nullptr, 0);
    }
    return true;
}
void show(std::string& out, const DescribedPlan& p, const std::vector<uint32_t>& src, bool pairs) {
    std::vector<uint32_t> dst(src.size());
    p.rebase(dst.data(), src.data(), src.size(), pairs);
    out += " |";
    for (uint32_t v : dst) out += " " + std::to_string(v);
}
// one description -> its answer line; false: the line is malformed
bool answer(const std::string& line, std::string& out) {
    std::istringstream ss(line);
    std::string place, t;
    unsigned long long f[9];
    if (!(ss >> place)) return false;
    for (auto& x : f) {
        if (!(ss >> t)) return false;
        x = std::stoull(t, nullptr, 0);
    }
    const bool spans = f[0] != 0, prefix_in_tail = f[1] != 0;
    const size_t n = f[5], m = f[6], nn = f[7], ng = f[8];
    std::vector<uint32_t> off, pre, nym, gat;
    if (!take(ss, off, spans ? 2 * n : n + 1) || !take(ss, pre, m ? (spans ? 2 * m : m + 1) : 0) || !take(ss, nym, 2 * nn) || !take(ss, gat, 6 * ng)) return false;
    DescribedPlan p(place == "arena" ? DescribedPlan::IN_ARENA : DescribedPlan::OWN_BUFFER, spans, f[2] ? &line : nullptr, (uint32_t)f[3], (uint32_t)f[4]);
    p.see_rows(off.data(), n, true);
    if (spans) p.see_rows(nym.data(), nn, true);
    p.see_rows(pre.data(), m, prefix_in_tail);
    p.see_gather(gat.data(), 3 * ng);
    if (p.close() != FABGPU_OK) {
        out = "refused " + std::to_string(p.rc);
        return true;
    }
    out = "ok " + std::to_string(p.lo) + " " + std::to_string(p.hi) + " " + std::to_string(p.tail_used ? 1 : 0) + " " + std::to_string(p.gather_total);
    show(out, p, off, spans);
    show(out, p, pre, spans);
    show(out, p, nym, true);
    show(out, p, gat, true);
    return true;
}

// ---- the cases made here: one of each refusal and of each closing rule, with the answer it must get ----
const char* const OWN_CASES[][2] = {
    {"own 1 0 0 0 0 2 0 0 0  7 7 10 20", "ok 10 20 0 0 | 0 0 0 10 | | |"},                                  // an empty span carries no address
    {"own 1 0 0 0 0 2 0 0 0  10 20 9 8", "refused -1"},                                                      // reversed
    {"own 1 0 1 1024 100 2 0 0 0  1000 1024 1024 1030", "ok 1000 1024 1 0 | 0 24 1024 1030 | | |"},          // up to and from tail_base
    {"own 1 0 1 1024 100 1 0 0 0  1000 1025", "refused -1"},                                                 // straddles
    {"own 1 0 1 1024 100 1 0 0 0  1100 1125", "refused -1"},                                                 // leaves the tail
    {"own 1 0 1 1024 100 1 1 0 0  0 5 1024 1030", "refused -1"},                                             // a prefix in the tail
    {"own 1 1 1 1024 100 1 1 0 0  0 5 1024 1030", "ok 0 5 1 0 | 0 5 | 1024 1030 | |"},                       // ... where the policy allows it
    {"own 0 0 0 0 0 4 2 0 0  40 40 50 60 60 30 30 35", "ok 30 60 0 0 | 10 10 20 30 30 | 0 0 5 | |"},         // consecutive, empty ends
    {"own 0 0 0 0 0 2 0 0 0  40 50 49", "refused -1"},
    {"own 1 0 1 1000 100 1 0 0 0  0 5", "refused -1"},                                                       // tail_base not a multiple of 64
    {"own 0 0 1 1024 100 1 0 0 0  0 5", "refused -1"},                                                       // a tail without the spans flag
    {"own 1 0 1 0xFFFFFF00 0xF0 1 0 0 0  0xFFFFFF00 0xFFFFFFF0", "ok 0 0 1 0 | 4294967040 4294967280 | | |"},
    {"own 1 0 1 0xFFFFFF00 0xF1 1 0 0 0  3 4", "refused -1"},
    {"arena 1 0 1 1024 100 1 0 0 1  0 5 1000 1025 0 0 0 0", "refused -1"},                                   // a gathered piece past tail_base
    {"arena 1 0 0 0 0 1 0 0 1  0 5 0 0x7FFFFFF0 0 0 0 0", "ok 0 2147483632 0 2147483632 | 0 5 | | | 0 2147483632 0 0 0 0"},
    {"arena 1 0 0 0 0 1 0 0 1  0 5 0 0x7FFFFFF0 9 10 0 0", "refused -5"},
    {"arena 1 0 1 1024 100 2 0 1 0  500 600 1024 1030 700 800", "ok 0 800 1 0 | 500 600 1024 1030 | | 700 800 |"},   // in the arena: lo = 0
    {"own 1 0 1 1024 100 2 0 0 0  500 600 1024 1030", "ok 500 600 1 0 | 0 100 1024 1030 | | |"},             // a buffer of its own: tail spans stay
};
}  // namespace

// stdin: the script.  With the argument "self": the cases above; exit status 0 and "0 failures" if every one answered as it must.
int main(int argc, char** argv) {
    std::string line, out;
    if (argc > 1 && std::string(argv[1]) == "self") {
        int bad = 0;
        for (const auto& c : OWN_CASES)
            if (!answer(c[0], out) || out != c[1]) {
                fprintf(stderr, "FAILED: %s\n  got  %s\n  want %s\n", c[0], out.c_str(), c[1]);
                bad++;
            }
        printf("hosttest_described_plan: %zu cases\n%d failures\n", sizeof(OWN_CASES) / sizeof(OWN_CASES[0]), bad);
        return bad ? 1 : 0;
    }
    size_t ln = 0;
    while (std::getline(std::cin, line)) {
        ln++;
        if (line.find_first_not_of(" \t") == std::string::npos || line[line.find_first_not_of(" \t")] == '#') continue;
        if (!answer(line, out)) {
            fprintf(stderr, "line %zu: malformed\n", ln);
            return 2;
        }
        puts(out.c_str());
    }
    return 0;
}
