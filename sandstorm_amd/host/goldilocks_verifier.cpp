// goldilocks_verifier.cpp — see goldilocks_verifier.hpp.  sandstorm_amd/goldilocks.py _verify is the specification: the checks below
// come in its order and refuse in its words.
#include "goldilocks_verifier.hpp"

#include <algorithm>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>

#include "gl_transcript.hpp"

namespace ssh {
namespace gl {

namespace {
[[noreturn]] void refuse(const std::string &what) { throw std::runtime_error(what); }
void need(bool cond, const std::string &what) { if (!cond) refuse(what); }
std::string u(uint64_t v) { return std::to_string(v); }
}  // namespace

// ---- the blob
Proof parse_proof_blob(const uint64_t *blob, uint64_t len) {
    static constexpr uint64_t MAX_VALUES = 1ull << 20, MAX_LAYERS = 64, MAX_POSITIONS = 1ull << 16, MAX_WIDTH = 64, MAX_DEPTH = 64;
    auto bad = [](const std::string &what) -> void { throw std::runtime_error("proof blob: " + what); };
    if (!blob) bad("NULL blob");
    if (len < 4) bad("blob of " + u(len) + " words is shorter than its header of 4");
    uint64_t at = 0;
    auto want = [&](uint64_t words, const std::string &what) {
        if (words > len - at) bad("truncated in " + what + ": " + u(words) + " words wanted at word " + u(at) + " of " + u(len));
    };
    Proof p;
    p.trace_len = blob[0]; p.pow_nonce = blob[1];
    if (blob[2] > 1) bad("the extension flag is " + u(blob[2]));
    p.has_ext = blob[2] == 1;
    const uint64_t n_layers = blob[3];
    if (n_layers > MAX_LAYERS) bad("layer count " + u(n_layers) + " out of range");
    at = 4;
    auto digest = [&](const std::string &what) { want(4, what); Digest d; memcpy(d.data(), blob + at, 32); at += 4; return d; };
    p.base_root = digest("the base root"); p.ext_root = digest("the extension root"); p.comp_root = digest("the composition root");
    auto values = [&](std::vector<uint64_t> &out, const std::string &what) {
        want(1, what + "' count");
        const uint64_t cnt = blob[at++];
        if (cnt > MAX_VALUES) bad(what + "' count " + u(cnt) + " out of range");
        want(3 * cnt, what);
        out.assign(blob + at, blob + at + 3 * cnt);
        at += 3 * cnt;
    };
    values(p.ood_trace, "the out-of-domain trace values");
    want(18, "the out-of-domain composition values");
    p.ood_comp.assign(blob + at, blob + at + 18);
    at += 18;
    values(p.remainder, "the remainder's coefficients");
    for (uint64_t k = 0; k < n_layers; ++k) {
        FriLayer fl;
        fl.root = digest("FRI layer " + u(k) + "'s root");
        want(1, "FRI layer " + u(k) + "'s length");
        if (blob[at] > 64) bad("FRI layer " + u(k) + "'s log length " + u(blob[at]) + " out of range");
        fl.log_len = (uint32_t)blob[at++];
        p.fri_layers.push_back(fl);
    }
    auto opening = [&](const std::string &what) {
        want(3, what + "'s header");
        const uint64_t npos = blob[at], width = blob[at + 1], depth = blob[at + 2];
        at += 3;
        if (npos > MAX_POSITIONS) bad(what + ": position count " + u(npos) + " out of range");
        if (width > MAX_WIDTH) bad(what + ": row width " + u(width) + " out of range");
        if (depth > MAX_DEPTH) bad(what + ": path depth " + u(depth) + " out of range");
        Opening o;
        o.width = (uint32_t)width; o.depth = (uint32_t)depth;
        want(npos * width, what + "'s rows");
        o.rows.assign(blob + at, blob + at + npos * width);
        at += npos * width;
        want(npos * depth * 4, what + "'s paths");
        o.paths.resize(npos * depth * 32);
        if (!o.paths.empty()) memcpy(o.paths.data(), blob + at, o.paths.size());
        at += npos * depth * 4;
        return o;
    };
    p.base = opening("the base opening");
    if (p.has_ext) p.ext = opening("the extension opening");
    p.comp = opening("the composition opening");
    for (uint64_t k = 0; k < n_layers; ++k) p.fri_layers[k].opening = opening("FRI layer " + u(k) + "'s opening");
    if (at != len) bad(u(len - at) + " words left over");
    return p;
}

// ---- the checks
namespace {
Digest tree_hash(const std::vector<uint8_t> &m, bool sha) { return sha ? sha256(m.data(), m.size()) : blake2s256(m.data(), m.size()); }

void check_opening(const Opening &o, uint32_t width, const std::vector<uint64_t> &positions, uint32_t depth, const Digest &root, const std::string &what, bool sha) {
    need(o.width == width && o.depth == depth && o.rows.size() == positions.size() * (size_t)width && o.paths.size() == positions.size() * (size_t)depth * 32, what + ": shape");
    for (size_t q = 0; q < positions.size(); ++q) {
        std::vector<uint8_t> leaf(8 * (size_t)width);
        for (uint32_t c = 0; c < width; ++c) for (int k = 0; k < 8; ++k) leaf[8 * c + k] = (uint8_t)(o.rows[q * width + c] >> (8 * k));
        Digest node = tree_hash(leaf, sha);
        for (uint32_t lvl = 0; lvl < depth; ++lvl) {
            const uint8_t *sib = o.paths.data() + (q * depth + lvl) * 32;
            std::vector<uint8_t> m;
            if (((positions[q] >> lvl) & 1) == 0) { m.assign(node.begin(), node.end()); m.insert(m.end(), sib, sib + 32); }
            else { m.assign(sib, sib + 32); m.insert(m.end(), node.begin(), node.end()); }
            node = tree_hash(m, sha);
        }
        need(node == root, what + ": authentication path does not reach the root");
    }
}

bool verify_pow(const Digest &digest, uint32_t bits, uint64_t nonce) {
    if (!bits) return true;
    std::vector<uint8_t> m;
    const uint64_t magic = 0x0123456789ABCDEDull;
    for (int k = 7; k >= 0; --k) m.push_back((uint8_t)(magic >> (8 * k)));
    m.insert(m.end(), digest.begin(), digest.end());
    m.push_back((uint8_t)bits);
    const Digest prefix = keccak256(m.data(), m.size());
    std::vector<uint8_t> m2(prefix.begin(), prefix.end());
    for (int k = 7; k >= 0; --k) m2.push_back((uint8_t)(nonce >> (8 * k)));
    const Digest h = keccak256(m2.data(), m2.size());
    uint64_t v = 0;
    for (int j = 0; j < 8; ++j) v = (v << 8) | h[j];
    return (v >> (64 - bits)) == 0;
}
uint32_t log2_of(uint64_t v) { uint32_t l = 0; while ((1ull << l) < v) ++l; return l; }
}  // namespace

std::vector<uint64_t> verify(const PlainAir &air, const Options &opt, uint32_t hash_option, const Digest &seed, const Proof &proof, uint32_t required_security_bits) {
    need(opt.log_blowup >= 1 && opt.log_blowup <= 4, "options: log_blowup must be 1, 2, 3 or 4 (LDE blowup 2, 4, 8 or 16), not " + u(opt.log_blowup));
    need(opt.num_queries >= 1 && opt.num_queries <= 256 && (opt.fold == 2 || opt.fold == 4 || opt.fold == 8 || opt.fold == 16) && opt.max_remainder >= 1 &&
             opt.max_remainder <= (1u << 16) && opt.grinding <= 40, "options out of range");
    const uint64_t n = proof.trace_len;
    need(n >= 16 && n <= (1ull << (32 - opt.log_blowup)) && (n & (n - 1)) == 0, "trace length");
    need(n == air.n(), "trace length: the proof's is " + u(n) + ", the AIR handle was made for " + u(air.n()));
    const uint32_t log_n = log2_of(n), lb = opt.log_blowup;
    const uint32_t log_N = std::max(1u, log_n + lb);
    const uint32_t sec = std::min(std::min(opt.num_queries * lb + opt.grinding, 192 - log_N), 128u);
    need(sec >= required_security_bits, "the proof's options conjecture " + u(sec) + " bits of security, " + u(required_security_bits) + " required");
    const uint64_t N = n << lb;
    const auto &mask = air.mask();
    need(proof.has_ext, "roots: 32 bytes each");
    need(proof.ood_trace.size() == 3 * mask.size(), "out-of-domain trace values: not a uint64 array of the expected shape");
    need(proof.ood_comp.size() == 18, "out-of-domain composition values: not a uint64 array of the expected shape");
    need(hash_option <= 1, "options: hash");
    const bool sha = opt.sha256;
    Coin coin(transcript_seed(seed, opt, n, air.statement_digest()), sha);
    coin.reseed_with_digest(proof.base_root);
    std::vector<Fq3> challenges;
    for (int i = 0; i < 3; ++i) challenges.push_back(coin.draw_fq3());
    coin.reseed_with_digest(proof.ext_root);
    const Fq3 alpha = coin.draw_fq3();
    coin.reseed_with_digest(proof.comp_root);
    const Fq3 z = coin.draw_fq3(), zc = mul3(z, z);
    std::map<std::pair<uint32_t, uint32_t>, Fq3> ood_t;
    for (size_t j = 0; j < mask.size(); ++j) ood_t[mask[j]] = Fq3{proof.ood_trace[3 * j], proof.ood_trace[3 * j + 1], proof.ood_trace[3 * j + 2]};
    std::vector<Fq3> ood_c;
    for (int k = 0; k < 6; ++k) ood_c.push_back(Fq3{proof.ood_comp[3 * k], proof.ood_comp[3 * k + 1], proof.ood_comp[3 * k + 2]});
    for (uint64_t v : proof.ood_trace) need(v < GL_P, "out-of-domain values: range");
    for (uint64_t v : proof.ood_comp) need(v < GL_P, "out-of-domain values: range");
    // the AIR identity at z: sum_k alpha^k C_k(z) multiplier_k(z) = H0(z^2) + z H1(z^2), H_h = sum_t X^t comp[3 h + t]
    const Fq3 lhs = air.evaluate(challenges, alpha, z, [&](uint32_t c, uint32_t o) { return ood_t.at({c, o}); });
    const Fq3 Xk[3] = {Fq3{1, 0, 0}, Fq3{0, 1, 0}, Fq3{0, 0, 1}};
    Fq3 H[2] = {Fq3{0, 0, 0}, Fq3{0, 0, 0}};
    for (int h = 0; h < 2; ++h) for (int t = 0; t < 3; ++t) H[h] = add3(H[h], mul3(Xk[t], ood_c[3 * h + t]));
    need(lhs == add3(H[0], mul3(z, H[1])), "the out-of-domain values do not satisfy the AIR");
    {
        std::vector<uint64_t> all(proof.ood_trace);
        all.insert(all.end(), proof.ood_comp.begin(), proof.ood_comp.end());
        coin.reseed_with_fq3s(all.data(), all.size());
    }
    const Fq3 gamma = coin.draw_fq3();
    std::vector<Fq3> coefs;
    {
        Fq3 cur{1, 0, 0};
        for (size_t i = 0; i < mask.size() + 6; ++i) { coefs.push_back(cur); cur = mul3(cur, gamma); }
    }
    // FRI transcript
    uint64_t n_layers = 0, rem_len = N;
    while (rem_len > ((uint64_t)opt.max_remainder << lb)) {
        need(rem_len % opt.fold == 0, "options: layer length " + u(rem_len) + " is not a multiple of the folding factor");
        rem_len /= opt.fold;
        ++n_layers;
    }
    need(proof.fri_layers.size() == n_layers, "number of FRI layers");
    std::vector<Fq3> fri_alphas;
    uint32_t ll = log_n + lb;
    const uint32_t log_fold = log2_of(opt.fold);
    for (const FriLayer &fl : proof.fri_layers) {
        need(fl.log_len == ll, "FRI layer length");
        coin.reseed_with_digest(fl.root);
        fri_alphas.push_back(coin.draw_fq3());
        ll -= log_fold;
    }
    const std::vector<uint64_t> &rem = proof.remainder;
    {
        bool ok = rem.size() == 3 * rem_len;
        for (size_t i = 3 * (rem_len >> lb); ok && i < rem.size(); ++i) ok = rem[i] == 0;
        for (size_t i = 0; ok && i < rem.size(); ++i) ok = rem[i] < GL_P;
        need(ok, "FRI remainder: shape / degree");
    }
    coin.reseed_with_fq3s(rem.data(), rem.size());
    need(verify_pow(coin.digest, opt.grinding, proof.pow_nonce), "proof of work");
    coin.reseed_with_int(proof.pow_nonce);
    const std::vector<uint64_t> positions = coin.draw_queries(opt.num_queries, N);
    // trace / composition openings, DEEP value at every query
    check_opening(proof.base, 5, positions, log_n + lb, proof.base_root, "base trace", sha);
    check_opening(proof.ext, 3, positions, log_n + lb, proof.ext_root, "extension trace", sha);
    check_opening(proof.comp, 6, positions, log_n + lb, proof.comp_root, "composition trace", sha);
    const uint64_t wN = fp_root_of_unity(log_n + lb), g = fp_root_of_unity(log_n), OFFSET = 7;
    std::map<uint64_t, Fq3> carried;
    for (size_t q = 0; q < positions.size(); ++q) {
        const uint64_t x = fp_mul(OFFSET, fp_pow(wN, positions[q]));
        uint64_t row[8];
        for (int c = 0; c < 5; ++c) row[c] = proof.base.rows[q * 5 + c];
        for (int c = 0; c < 3; ++c) row[5 + c] = proof.ext.rows[q * 3 + c];
        Fq3 acc{0, 0, 0};
        for (size_t j = 0; j < mask.size(); ++j) {
            const Fq3 den = sub3(f3(x), scale3(z, fp_pow(g, mask[j].second % n)));
            acc = add3(acc, mul3(mul3(coefs[j], sub3(f3(row[mask[j].first]), ood_t.at(mask[j]))), inv3(den)));
        }
        const Fq3 dinv = inv3(sub3(f3(x), zc));
        for (int k = 0; k < 6; ++k) acc = add3(acc, mul3(mul3(coefs[mask.size() + k], sub3(f3(proof.comp.rows[q * 6 + k]), ood_c[k])), dinv));
        carried[positions[q]] = acc;
    }
    // FRI: layer rows open, contain the value carried from the layer below, and fold to the next
    std::vector<uint64_t> pos = positions;
    ll = log_n + lb;
    uint64_t off = OFFSET;
    for (size_t li = 0; li < proof.fri_layers.size(); ++li) {
        const FriLayer &fl = proof.fri_layers[li];
        const uint64_t rows = (1ull << ll) / opt.fold;
        std::vector<uint64_t> folded;
        for (uint64_t p : pos) folded.push_back(p % rows);
        std::sort(folded.begin(), folded.end());
        folded.erase(std::unique(folded.begin(), folded.end()), folded.end());
        check_opening(fl.opening, 3 * opt.fold, folded, ll - log_fold, fl.root, "FRI layer " + u(li), sha);
        const uint64_t wL = fp_root_of_unity(ll), wf_inv = fp_inv(fp_root_of_unity(log_fold)), fold_inv = fp_inv(opt.fold);
        std::map<uint64_t, Fq3> nxt;
        for (size_t qi = 0; qi < folded.size(); ++qi) {
            const uint64_t j = folded[qi];
            std::vector<Fq3> vals;
            for (uint32_t k = 0; k < opt.fold; ++k) { const uint64_t *r = fl.opening.rows.data() + qi * 3 * opt.fold + 3 * k; vals.push_back(Fq3{r[0], r[1], r[2]}); }
            for (uint64_t p : pos)
                if (p % rows == j) need(vals[p / rows] == carried.at(p), "FRI layer " + u(li) + " does not continue the layer below at position " + u(p));
            // interpolant of the row over x_j <w_fold>, evaluated at alpha: coefficient t = (1/fold) x_j^-t sum_m v_m w_fold^(-t m)
            const uint64_t xj_inv = fp_inv(fp_mul(off, fp_pow(wL, j)));
            Fq3 acc{0, 0, 0};
            for (uint32_t t = opt.fold; t-- > 0;) {
                Fq3 s{0, 0, 0};
                for (uint32_t m = 0; m < opt.fold; ++m) s = add3(s, scale3(vals[m], fp_pow(wf_inv, (uint64_t)t * m)));
                const Fq3 coef = scale3(s, fp_mul(fp_pow(xj_inv, t), fold_inv));
                acc = add3(mul3(acc, fri_alphas[li]), coef);
            }
            nxt[j] = acc;
        }
        carried = nxt; pos = folded; ll -= log_fold; off = fp_pow(off, opt.fold);
    }
    // the remainder polynomial at the last positions
    const uint64_t wL = fp_root_of_unity(ll);
    for (uint64_t p : pos) {
        const uint64_t x = fp_mul(off, fp_pow(wL, p));
        Fq3 acc{0, 0, 0};
        for (size_t k = rem.size() / 3; k-- > 0;) acc = add3(scale3(acc, x), Fq3{rem[3 * k], rem[3 * k + 1], rem[3 * k + 2]});
        need(acc == carried.at(p), "the remainder does not continue the last FRI layer at position " + u(p));
    }
    return positions;
}

}  // namespace gl
}  // namespace ssh
