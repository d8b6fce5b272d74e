// gl_transcript.hpp — what the 64-bit field's prover and verifier share on the host (goldilocks_prover.cpp, goldilocks_verifier.cpp): Fq3's
// product, SHA-256, the coin and the transcript seed.  Free of the device runtime: it needs coin.hpp's keccak256 only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "goldilocks_prover.hpp"

namespace ssh {
namespace gl {

// ---- the coin (goldilocks.py Coin over coin.PublicCoin's Solidity shape: solidity.rs:54-118 with H = Keccak-256 or SHA-256)
struct Coin {
    Digest digest;
    uint64_t counter = 0;
    bool sha;
    Coin(const Digest &seed, bool sha_) : digest(seed), sha(sha_) {}
    Digest h(const std::vector<uint8_t> &m) const { return sha ? sha256(m.data(), m.size()) : keccak256(m.data(), m.size()); }
    void reseed_with_bytes(const uint8_t *data, size_t len) {
        std::vector<uint8_t> m(digest.begin(), digest.end());                  // be32(digest + 1)
        for (int i = 31; i >= 0; --i) { if (++m[i] != 0) break; }
        m.insert(m.end(), data, data + len);
        digest = h(m);
        counter = 0;
    }
    void reseed_with_digest(const Digest &d) { reseed_with_bytes(d.data(), 32); }
    void reseed_with_fq3s(const uint64_t *vals, size_t n3) {                   // little-endian 8-byte coordinates
        std::vector<uint8_t> b(8 * n3);
        for (size_t i = 0; i < n3; ++i) for (int k = 0; k < 8; ++k) b[8 * i + k] = (uint8_t)(vals[i] >> (8 * k));
        reseed_with_bytes(b.data(), b.size());
    }
    void reseed_with_int(uint64_t v) {
        uint8_t b[8];
        for (int k = 0; k < 8; ++k) b[k] = (uint8_t)(v >> (8 * (7 - k)));
        reseed_with_bytes(b, 8);
    }
    Digest draw_bytes() {
        std::vector<uint8_t> m(digest.begin(), digest.end());
        uint8_t c[32] = {0};
        for (int k = 0; k < 8; ++k) c[31 - k] = (uint8_t)(counter >> (8 * k));
        m.insert(m.end(), c, c + 32);
        ++counter;
        return h(m);
    }
    uint64_t draw_felt() {                                                     // the first of the draw's four big-endian words below p
        for (;;) {
            const Digest d = draw_bytes();
            for (int k = 0; k < 4; ++k) {
                uint64_t v = 0;
                for (int j = 0; j < 8; ++j) v = (v << 8) | d[8 * k + j];
                if (v < 0xFFFFFFFF00000001ull) return v;
            }
        }
    }
    Fq3 draw_fq3() { Fq3 r; r[0] = draw_felt(); r[1] = draw_felt(); r[2] = draw_felt(); return r; }
    std::vector<uint64_t> draw_queries(size_t max_n, uint64_t domain) {
        std::vector<uint64_t> vals;
        while (vals.size() < max_n) {
            const Digest d = draw_bytes();
            for (int k = 0; k < 4 && vals.size() < max_n; ++k) {
                uint64_t v = 0;
                for (int j = 0; j < 8; ++j) v = (v << 8) | d[8 * k + j];
                vals.push_back(v % domain);
            }
        }
        std::sort(vals.begin(), vals.end());
        vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
        return vals;
    }
};

}  // namespace gl
}  // namespace ssh
