// Stand-alone host program over MspFamilyTable and ParseHashFamily (msp_family.h; its own main; built by the Makefile as
// ../lib/hosttest_msp_family, and as ../lib/hosttest_msp_family_san with -fsanitize=address,undefined by `make sanitize-msp-family`).
// The registry is a pure function of strings, so it runs here without a provider and without a device.
//
// With a file name: the file is a script, one command per line, strings in hex ("-": empty); one answer line per command on stdout.
//     sha3 0|1            -> ok                       (whether the provider serves the family: the hash_sha3 option)
//     set MSPID FAMILY    -> ok | refused TEXT        (what fabgpu_csp_msp_hash_family does: parse, then the table)
//     get MSPID           -> SHA2 | SHA3
//     count               -> count N                  (MSPs set SHA3)
// tests/test_msp_family_host.py writes such scripts and checks every answer.  Each looked-up mspid lives in a heap buffer of exactly its
// length, so that a read past its end is the sanitizer's to see.
// Without arguments: the same cases made here and, last, lookups from four threads while a fifth sets and resets families.  Exit status
// 0 and "0 failures": everything answered as it must.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "msp_family.h"

using fab::MspFamilyTable;
using fab::ParseHashFamily;

namespace {

bool unhex(const std::string& s, std::string& out) {
    out.clear();
    if (s == "-") return true;
    if (s.size() % 2) return false;
    auto nib = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
    for (size_t i = 0; i < s.size(); i += 2) {
        const int a = nib(s[i]), b = nib(s[i + 1]);
        if (a < 0 || b < 0) return false;
        out.push_back((char)(a << 4 | b));
    }
    return true;
}
// exactly these bytes on the heap, nothing behind them
bool sha3_exact(const MspFamilyTable& t, const std::string& mspid) {
    uint8_t* p = (uint8_t*)malloc(mspid.size() ? mspid.size() : 1);
    if (!mspid.empty()) memcpy(p, mspid.data(), mspid.size());
    const bool r = t.Sha3(p, mspid.size());
    free(p);
    return r;
}
// what the C entry does with (mspid, family): "" or the refusal
std::string set_family(MspFamilyTable& t, bool served, const std::string& mspid, const char* family) {
    bool sha3 = false;
    std::string err;
    if (!ParseHashFamily(family, served, &sha3, &err)) return err;
    return t.Set(mspid, sha3) ? "" : "invalid mspid";
}

int run_script(const char* path) {
    std::ifstream in(path);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    MspFamilyTable t;
    bool served = false;
    std::string line;
    size_t ln = 0;
    while (std::getline(in, line)) {
        ln++;
        std::istringstream ss(line);
        std::string cmd, a, b, id, fam;
        if (!(ss >> cmd) || cmd[0] == '#') continue;
        if (cmd == "sha3") {
            int v = 0;
            ss >> v;
            served = v != 0;
            puts("ok");
        } else if (cmd == "set") {
            ss >> a >> b;
            if (ss.fail() || !unhex(a, id) || !unhex(b, fam)) {
                fprintf(stderr, "line %zu: malformed\n", ln);
                return 2;
            }
            const std::string e = set_family(t, served, id, fam.c_str());
            if (e.empty()) puts("ok");
            else printf("refused %s\n", e.c_str());
        } else if (cmd == "get") {
            ss >> a;
            if (ss.fail() || !unhex(a, id)) {
                fprintf(stderr, "line %zu: malformed\n", ln);
                return 2;
            }
            puts(sha3_exact(t, id) ? "SHA3" : "SHA2");
        } else if (cmd == "count") {
            printf("count %zu\n", t.CountSha3());
        } else {
            fprintf(stderr, "line %zu: unknown command %s\n", ln, cmd.c_str());
            return 2;
        }
    }
    return 0;
}

int g_bad = 0;
void expect(bool ok, const char* what, size_t i = 0) {
    if (ok) return;
    fprintf(stderr, "FAILED: %s (%zu)\n", what, i);
    g_bad++;
}

int own_cases() {
    {   // defaults, set / get, back to the default
        MspFamilyTable t;
        expect(!t.AnySha3() && !sha3_exact(t, "Org1MSP") && !sha3_exact(t, ""), "every MSP is SHA2 until set");
        expect(set_family(t, true, "Org1MSP", "SHA3").empty() && sha3_exact(t, "Org1MSP") && t.CountSha3() == 1, "set SHA3");
        expect(!sha3_exact(t, "Org1MS") && !sha3_exact(t, "Org1MSPx") && !sha3_exact(t, "org1msp"), "neighbouring names stay SHA2");
        expect(set_family(t, true, "Org1MSP", "SHA3").empty() && t.CountSha3() == 1, "set twice");
        expect(set_family(t, true, "Org1MSP", "SHA2").empty() && !sha3_exact(t, "Org1MSP") && !t.AnySha3(), "set back");
        expect(set_family(t, false, "Org2MSP", "SHA2").empty() && !t.AnySha3(), "SHA2 needs no option");
    }
    {   // the refusals
        MspFamilyTable t;
        expect(set_family(t, true, "Org1MSP", "SHA1") == "hash familiy not recognized [SHA1]", "an unknown family");
        expect(set_family(t, true, "Org1MSP", "") == "hash familiy not recognized []", "an empty family");
        expect(set_family(t, true, "Org1MSP", nullptr) == "hash familiy not recognized []", "no family");
        expect(set_family(t, true, "Org1MSP", "sha3") == "hash familiy not recognized [sha3]", "families are case-sensitive");
        expect(set_family(t, false, "Org1MSP", "SHA3") == "failed computing digest: SHA3 is served by bccsp/sw, not by the GPU provider", "SHA3 with the option off");
        expect(set_family(t, true, "", "SHA3") == "invalid mspid", "an empty mspid");
        expect(set_family(t, true, std::string(MspFamilyTable::kMaxMspId + 1, 'a'), "SHA3") == "invalid mspid", "an overlong mspid");
        expect(set_family(t, true, std::string(MspFamilyTable::kMaxMspId, 'a'), "SHA3").empty(), "the longest mspid");
        expect(t.CountSha3() == 1, "nothing refused was stored");
    }
    {   // many MSPs, names with a zero byte inside
        MspFamilyTable t;
        const size_t N = 5000;
        auto name = [](size_t i) { return "Org" + std::to_string(i) + std::string(1, '\0') + "MSP"; };
        for (size_t i = 0; i < N; i += 2) expect(set_family(t, true, name(i), "SHA3").empty(), "set", i);
        expect(t.CountSha3() == N / 2, "count");
        for (size_t i = 0; i < N; i++) expect(sha3_exact(t, name(i)) == (i % 2 == 0), "get", i);
        for (size_t i = 0; i < N; i += 4) expect(set_family(t, true, name(i), "SHA2").empty(), "reset", i);
        for (size_t i = 0; i < N; i++) expect(sha3_exact(t, name(i)) == (i % 4 == 2), "get after reset", i);
    }
    {   // readers beside a writer: a fixed MSP answers the same throughout, a toggled one answers either
        MspFamilyTable t;
        t.Set("FixedSHA3", true);
        std::atomic<bool> stop{false};
        std::atomic<int> wrong{0};
        std::vector<std::thread> readers;
        for (int r = 0; r < 4; r++)
            readers.emplace_back([&] {
                while (!stop.load(std::memory_order_relaxed)) {
                    if (!sha3_exact(t, "FixedSHA3") || sha3_exact(t, "FixedSHA2")) wrong.fetch_add(1);
                    (void)sha3_exact(t, "Toggled7");
                }
            });
        std::thread writer([&] {
            for (int k = 0; k < 20000; k++) t.Set("Toggled" + std::to_string(k % 16), (k / 16) % 2 == 0);
            stop.store(true);
        });
        writer.join();
        for (auto& th : readers) th.join();
        expect(wrong.load() == 0, "readers beside a writer");
    }
    printf("%d failures\n", g_bad);
    return g_bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) { return argc > 1 ? run_script(argv[1]) : own_cases(); }
