// Stand-alone host program over IdentityToP384 (block_prepass.cpp; its own main; built by the Makefile as ../lib/hosttest_p384_ident, and
// as ../lib/hosttest_p384_ident_san with -fsanitize=address,undefined by `make sanitize-p384-ident`).  The decoder reads identities out
// of UNVALIDATED blocks: it runs here over one P-384 identity - the file named on the command line (tests/test_p384_identity_host.py
// writes one), or one made here around P-384's generator - over every proper prefix of it and over every single-bit flip of it, each in
// a heap buffer of exactly its length, so that a read past the end is the sanitizer's to see.  Exit status 0: the identity decodes to
// an on-curve key, no prefix decodes, and every flipped input either is refused or yields 96 bytes (never a crash, never a key from
// outside the buffer: the key bytes of an accepted flip are found in the flipped certificate again).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "block_prepass.h"
#include "p384_tables.h"

using fab::bccsp::IdentityToP384;
using fab::bccsp::PemToDer;

namespace {
typedef std::vector<uint8_t> Bytes;
Bytes tlv(uint8_t tag, const Bytes& body) {
    Bytes o(1, tag);
    const size_t n = body.size();
    if (n < 128) {
        o.push_back((uint8_t)n);
    } else if (n < 256) {
        o.push_back(0x81);
        o.push_back((uint8_t)n);
    } else {
        o.push_back(0x82);
        o.push_back((uint8_t)(n >> 8));
        o.push_back((uint8_t)n);
    }
    o.insert(o.end(), body.begin(), body.end());
    return o;
}
Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes o;
    for (const Bytes& p : parts) o.insert(o.end(), p.begin(), p.end());
    return o;
}
Bytes name(const char* cn) {   // Name: one RDN with a commonName
    const Bytes oid_cn = {0x55, 0x04, 0x03};
    return tlv(0x30, tlv(0x31, tlv(0x30, cat({tlv(0x06, oid_cn), tlv(0x0C, Bytes(cn, cn + strlen(cn)))}))));
}
std::string base64(const Bytes& b) {
    static const char T[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    std::string o;
    size_t col = 0;
    for (size_t i = 0; i < b.size(); i += 3) {
        const uint32_t v = (uint32_t)b[i] << 16 | (i + 1 < b.size() ? (uint32_t)b[i + 1] << 8 : 0) | (i + 2 < b.size() ? b[i + 2] : 0);
        const char q[4] = {T[v >> 18], T[(v >> 12) & 63], i + 1 < b.size() ? T[(v >> 6) & 63] : '=', i + 2 < b.size() ? T[v & 63] : '='};
        o.append(q, 4);
        if ((col += 4) == 64) {
            o.push_back('\n');
            col = 0;
        }
    }
    if (col) o.push_back('\n');
    return o;
}
// msp.SerializedIdentity{1 mspid, 2 id_bytes = PEM of a certificate whose SubjectPublicKeyInfo carries P-384's generator}
Bytes generator_identity() {
    uint8_t g[96];
    fab::p384::generator_be(g, g + 48);
    const Bytes oid_ec = {0x2A, 0x86, 0x48, 0xCE, 0x3D, 0x02, 0x01}, oid_384 = {0x2B, 0x81, 0x04, 0x00, 0x22};
    const Bytes oid_sig = {0x2A, 0x86, 0x48, 0xCE, 0x3D, 0x04, 0x03, 0x03};   // ecdsa-with-SHA384
    Bytes point = {0x00, 0x04};
    point.insert(point.end(), g, g + 96);
    const Bytes spki = tlv(0x30, cat({tlv(0x30, cat({tlv(0x06, oid_ec), tlv(0x06, oid_384)})), tlv(0x03, point)}));
    const Bytes sigalg = tlv(0x30, tlv(0x06, oid_sig));
    const char* when = "250101000000Z";
    const Bytes validity = tlv(0x30, cat({tlv(0x17, Bytes(when, when + 13)), tlv(0x17, Bytes(when, when + 13))}));
    const Bytes tbs = tlv(0x30, cat({tlv(0xA0, tlv(0x02, Bytes(1, 2))), tlv(0x02, Bytes(16, 0x5A)), sigalg, name("ca.org1.example.com, a certificate authority of the tests"),
                                     validity, name("peer0.org1.example.com, an endorsing peer of the tests"), spki}));
    Bytes sig(1, 0);
    sig.resize(1 + 102, 0x33);                                          // (the pass never checks chains: arbitrary bytes)
    const Bytes cert = tlv(0x30, cat({tbs, sigalg, tlv(0x03, sig)}));
    const std::string pem = "-----BEGIN CERTIFICATE-----\n" + base64(cert) + "-----END CERTIFICATE-----\n";
    const char* msp = "Org1MSP";
    Bytes id = {0x0A, 7};
    id.insert(id.end(), msp, msp + 7);
    id.push_back(0x12);
    size_t n = pem.size();                                              // (varint length: two bytes for 128 .. 16383)
    id.push_back((uint8_t)(0x80 | (n & 0x7F)));
    id.push_back((uint8_t)(n >> 7));
    id.insert(id.end(), pem.begin(), pem.end());
    return id;
}
// the decoder over exactly these bytes, in a heap buffer of exactly their length
bool decode(const uint8_t* p, size_t n, uint8_t* qxy) {
    uint8_t* buf = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(buf, p, n);
    const bool ok = IdentityToP384(buf, n, qxy, qxy + 48);
    free(buf);
    return ok;
}
}  // namespace

int main(int argc, char** argv) {
    Bytes id;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        uint8_t chunk[4096];
        size_t k;
        while ((k = fread(chunk, 1, sizeof(chunk), f)) > 0) id.insert(id.end(), chunk, chunk + k);
        fclose(f);
    } else {
        id = generator_identity();
    }
    uint8_t key[96], q[96];
    if (!decode(id.data(), id.size(), key) || !fab::p384::pubkey_on_curve(key, key + 48)) {
        fprintf(stderr, "the identity itself does not decode to an on-curve P-384 key\n");
        return 1;
    }
    int bad = 0;
    size_t inputs = 1, accepted_flips = 0;
    for (size_t n = 0; n < id.size(); n++, inputs++)
        if (decode(id.data(), n, q)) {
            fprintf(stderr, "prefix of %zu bytes decodes\n", n);
            bad++;
        }
    Bytes m = id;
    for (size_t bit = 0; bit < 8 * id.size(); bit++, inputs++) {
        m[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
        if (decode(m.data(), m.size(), q)) {
            accepted_flips++;
            // what it answers must be the point the flipped certificate holds: X || Y contiguous in its DER
            const uint8_t* idb = nullptr;
            Bytes der;
            bool found = false;
            for (size_t at = 0; at + 27 <= m.size() && !idb; at++)
                if (memcmp(&m[at], "-----BEGIN CERTIFICATE-----", 27) == 0) idb = &m[at];
            if (idb && PemToDer(idb, (size_t)(m.data() + m.size() - idb), der))
                for (size_t at = 0; at + 96 <= der.size() && !found; at++) found = memcmp(&der[at], q, 96) == 0;
            if (!found) {
                fprintf(stderr, "flip of bit %zu: the key answered is not in the certificate\n", bit);
                bad++;
            }
        }
        m[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
    }
    printf("hosttest_p384_ident: %zu inputs (identity of %zu bytes, %zu prefixes, %zu bit flips of which %zu still decode), %d failures\n", inputs, id.size(),
           id.size(), 8 * id.size(), accepted_flips, bad);
    return bad ? 1 : 0;
}
