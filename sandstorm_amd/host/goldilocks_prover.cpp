// goldilocks_prover.cpp — the 64-bit field's claim (cli/src/main.rs:103-133: p = 2^64 - 2^32 + 1, challenges in Fq3) in the C++ host:
// the mirror of sandstorm_amd/goldilocks.py's Prover, stage by stage and array for array (tests hold the two to each other: the
// same proof arrays from the same statement).  PARITY UNPINNED, as the Python module's header says: the reference instantiates this
// claim from un-vendored parts; Options.hash = "sha256" takes the parts it NAMES (MatrixMerkleTreeImpl<Sha256HashFn> trees, a coin
// with SHA-256 inside), "blake2s" this library's own choice.  Every stage is a HIP kernel behind the C ABI (the *_gl64* entry
// points); what the layout decides - the extension columns, the lowered composition program for the drawn challenges - comes
// from the caller through two callbacks, as the 252-bit Prover takes its extension builder.
#include "goldilocks_prover.hpp"
#include "gl_transcript.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace ssh {
namespace gl {

static void ok(ss_status s) {
    if (s != SS_OK) throw std::runtime_error(ss_last_error());
}

// ---- the field on the host (a handful of values per proof)
static const uint64_t P = 0xFFFFFFFF00000001ull;
static uint64_t mulm(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % P); }
static uint64_t addm(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a + b) % P); }
static uint64_t powm(uint64_t a, uint64_t e) { uint64_t r = 1; for (; e; e >>= 1) { if (e & 1) r = mulm(r, a); a = mulm(a, a); } return r; }
static uint64_t invm(uint64_t a) { return powm(a, P - 2); }
static Fq3 pow3(Fq3 a, uint64_t e) { Fq3 r{1, 0, 0}; for (; e; e >>= 1) { if (e & 1) r = mul3(r, a); a = mul3(a, a); } return r; }
// (mul3, SHA-256, the coin and the transcript seed: gl_transcript.cpp, shared with the verifier)

namespace {
struct Dev {                                                // a device buffer of the context's pool
    ss_ctx *ctx;
    void *p = nullptr;
    Dev(ss_ctx *c, size_t bytes) : ctx(c) { ok(ss_dev_alloc(c, bytes ? bytes : 8, &p)); }
    ~Dev() { if (p) ss_dev_free(ctx, p); }
    Dev(const Dev &) = delete;
    Dev &operator=(const Dev &) = delete;
    uint64_t *u64() const { return (uint64_t *)p; }
    uint8_t *u8() const { return (uint8_t *)p; }
};
using DevP = std::unique_ptr<Dev>;
struct Commitment { DevP nodes; Digest root; };
}  // namespace

std::vector<ConstraintFailure> check_trace(ss_ctx *ctx, const CheckBlob &check, const std::vector<const uint64_t *> &cols, uint32_t log_n) {
    const size_t n_checks = check.domains.size();
    if (!n_checks || check.names.size() != n_checks || check.domain_names.size() != n_checks) throw std::runtime_error("check program: one domain and two names per check");
    ss_air_program prog;
    memset(&prog, 0, sizeof prog);
    static const uint64_t no_consts[3] = {0, 0, 0};
    static const uint32_t no_desc[2] = {0, 0};
    prog.code = check.code.data(); prog.n_instr = (uint32_t)(check.code.size() / 2);
    prog.consts = check.consts.empty() ? no_consts : check.consts.data(); prog.n_consts = (uint32_t)(check.consts.size() / 3);
    prog.d_tables = check.d_tables; prog.table_desc = check.table_desc.empty() ? no_desc : check.table_desc.data();
    prog.n_tables = (uint32_t)(check.table_desc.size() / 2);
    prog.n_slots = check.n_slots;
    std::vector<uint64_t> first(n_checks, 0);
    std::vector<uint32_t> count(n_checks, 0);
    ok(ss_check_constraints_gl64x3(ctx, &prog, cols.data(), (uint32_t)cols.size(), log_n, check.domains.data(), (uint32_t)n_checks, first.data(), count.data()));
    std::vector<ConstraintFailure> bad;
    for (size_t k = 0; k < n_checks; ++k)
        if (count[k]) bad.push_back(ConstraintFailure{(uint32_t)k, check.names[k], check.domain_names[k], first[k], count[k]});
    return bad;
}
std::string describe_failures(const std::vector<ConstraintFailure> &f) {
    if (f.empty()) return "the trace satisfies the AIR";
    const ConstraintFailure &a = f.front();
    return "trace does not satisfy the AIR: " + std::to_string(f.size()) + (f.size() == 1 ? " constraint fails" : " constraints fail") + "; first: #" +
           std::to_string(a.index) + " " + a.name + " (" + a.domain + ") at row " + std::to_string(a.first_row) + ", " + std::to_string(a.count) +
           (a.count == 1 ? " row" : " rows");
}

FriShape fri_shape(const Options &opt, uint64_t n_lde) {
    const std::string nums = " (LDE domain " + std::to_string(n_lde) + ", folding factor " + std::to_string(opt.fold) + ", max remainder " +
                             std::to_string(opt.max_remainder) + ", log blowup " + std::to_string(opt.log_blowup) + ")";
    if (opt.fold != 2 && opt.fold != 4 && opt.fold != 8 && opt.fold != 16)
        throw std::runtime_error("FRI geometry refused: the FRI folding factor must be 2, 4, 8 or 16" + nums);
    if (opt.max_remainder < 1 || opt.max_remainder > (1u << 16)) throw std::runtime_error("FRI geometry refused: the max remainder must be 1 .. 65536" + nums);
    if (opt.log_blowup > 4) throw std::runtime_error("FRI geometry refused: the log blowup must be at most 4" + nums);
    FriShape s{0, n_lde};
    for (; s.last_len > ((uint64_t)opt.max_remainder << opt.log_blowup); s.last_len /= opt.fold) {
        if (s.last_len % opt.fold) throw std::runtime_error("FRI geometry refused: a FRI layer's length is not a multiple of the folding factor" + nums);
        ++s.layers;
    }
    return s;
}
void check_log_blowup(uint32_t log_blowup) {
    if (log_blowup < 1 || log_blowup > 4)
        throw std::runtime_error("log_blowup refused: the log blowup must be 1, 2, 3 or 4 (LDE blowup 2, 4, 8 or 16), not " + std::to_string(log_blowup));
}

Proof prove(ss_ctx *ctx, const Options &opt, const Digest &seed, const Digest &statement_digest, const std::vector<const uint64_t *> &base_cols,
            uint64_t n, const std::vector<std::pair<uint32_t, uint32_t>> &mask, uint32_t num_challenges, uint32_t num_ext,
            const ExtensionBuilder &build_extension, const ProgramBuilder &build_program, const CheckBuilder &build_check) {
    if (!n || (n & (n - 1))) throw std::runtime_error("trace length: a power of two");
    check_log_blowup(opt.log_blowup);
    uint32_t log_n = 0;
    while ((1ull << log_n) < n) ++log_n;
    const uint32_t lb = opt.log_blowup;
    const uint64_t N = n << lb, OFFSET = 7;
    const uint32_t n_layers = fri_shape(opt, N).layers;     // refused here, not at step 7 after every commitment
    const int row_hash = opt.sha256 ? SS_HASH_SHA256 : SS_HASH_BLAKE2S, tree = opt.sha256 ? SS_TREE_SHA256 : SS_TREE_BLAKE2S;
    Coin coin(transcript_seed(seed, opt, n, statement_digest), opt.sha256);
    Proof proof;
    proof.trace_len = n;

    auto commit = [&](const std::vector<const uint64_t *> &segs, uint32_t seg_len, uint64_t rows) {
        Dev dig(ctx, 32 * rows);
        Commitment c;
        c.nodes.reset(new Dev(ctx, 64 * rows));
        ok(ss_hash_rows_gl64(ctx, row_hash, segs.data(), (uint32_t)segs.size(), seg_len, rows, dig.u8()));
        uint8_t root[33];
        ok(ss_merkle_build(ctx, tree, 0, SS_LEAF_DIGEST, dig.p, rows, c.nodes->u8(), nullptr, root));
        memcpy(c.root.data(), root, 32);
        return c;
    };
    auto open = [&](const std::vector<const uint64_t *> &segs, uint32_t seg_len, const Commitment &c, uint64_t rows, const std::vector<uint64_t> &positions) {
        Opening o;
        o.width = (uint32_t)segs.size() * seg_len;
        o.rows.assign(positions.size() * o.width, 0);
        ok(ss_gather_rows_gl64(ctx, segs.data(), (uint32_t)segs.size(), seg_len, rows, positions.data(), (uint32_t)positions.size(), o.rows.data()));
        uint32_t depth = 0;
        while ((1ull << depth) < rows) ++depth;
        o.depth = depth;
        o.paths.assign(positions.size() * depth * 32, 0);
        ok(ss_merkle_open(ctx, c.nodes->u8(), nullptr, rows, positions.data(), (uint32_t)positions.size(), o.paths.data(), nullptr));
        return o;
    };
    std::vector<DevP> keep;                                 // every column of the proof lives to its end
    auto extend = [&](const std::vector<const uint64_t *> &cols, std::vector<const uint64_t *> *ev, std::vector<const uint64_t *> *co) {
        std::vector<uint64_t *> e, c;
        for (size_t i = 0; i < cols.size(); ++i) {
            keep.emplace_back(new Dev(ctx, 8 * N)); e.push_back(keep.back()->u64());
            keep.emplace_back(new Dev(ctx, 8 * n)); c.push_back(keep.back()->u64());
        }
        if (!cols.empty()) ok(ss_lde_gl64(ctx, cols.data(), (uint32_t)cols.size(), log_n, lb, OFFSET, e.data(), c.data()));
        ev->insert(ev->end(), e.begin(), e.end());
        co->insert(co->end(), c.begin(), c.end());
    };
    // 1-2. base and extension traces
    std::vector<const uint64_t *> trace_ev, trace_co;
    extend(base_cols, &trace_ev, &trace_co);
    const size_t nbase = base_cols.size();
    Commitment base_com = commit(std::vector<const uint64_t *>(trace_ev.begin(), trace_ev.begin() + nbase), 1, N);
    proof.base_root = base_com.root;
    coin.reseed_with_digest(proof.base_root);
    std::vector<Fq3> challenges;
    for (uint32_t i = 0; i < num_challenges; ++i) challenges.push_back(coin.draw_fq3());
    Commitment ext_com;
    if (num_ext) {
        const std::vector<const uint64_t *> ext_cols = build_extension(challenges);
        if (ext_cols.size() != num_ext) throw std::runtime_error("the extension builder returned another number of coordinate columns");
        if (build_check) {                                  // the caller's base columns and the fresh extension columns, with this proof's challenges
            std::vector<const uint64_t *> all(base_cols.begin(), base_cols.end());
            all.insert(all.end(), ext_cols.begin(), ext_cols.end());
            const std::vector<ConstraintFailure> bad = check_trace(ctx, build_check(challenges), all, log_n);
            if (!bad.empty()) throw std::runtime_error(describe_failures(bad));
        }
        extend(ext_cols, &trace_ev, &trace_co);
        ext_com = commit(std::vector<const uint64_t *>(trace_ev.begin() + nbase, trace_ev.end()), 1, N);
        proof.has_ext = true;
        proof.ext_root = ext_com.root;
        coin.reseed_with_digest(proof.ext_root);
    } else if (build_check) {                               // an AIR without an extension trace: the base columns alone
        const std::vector<ConstraintFailure> bad = check_trace(ctx, build_check(challenges), base_cols, log_n);
        if (!bad.empty()) throw std::runtime_error(describe_failures(bad));
    }
    // 3-4. composition: the lowered program over the 2n-point coset, then H = H0(x^2) + x H1(x^2) as six coordinate columns
    const Fq3 alpha = coin.draw_fq3();
    const ProgramData pd = build_program(challenges, alpha);
    ss_air_program prog;
    memset(&prog, 0, sizeof prog);
    static const uint64_t no_consts[3] = {0, 0, 0};
    static const uint32_t no_desc[2] = {0, 0};
    prog.code = pd.code.data(); prog.n_instr = (uint32_t)(pd.code.size() / 2);
    prog.consts = pd.consts.empty() ? no_consts : pd.consts.data(); prog.n_consts = (uint32_t)(pd.consts.size() / 3);
    prog.d_tables = pd.d_tables; prog.table_desc = pd.table_desc.empty() ? no_desc : pd.table_desc.data(); prog.n_tables = (uint32_t)(pd.table_desc.size() / 2);
    prog.n_slots = pd.n_slots;
    std::vector<const uint64_t *> comp_co, comp_ev;
    {
        // The constraints have degree 2: whatever the blowup they are evaluated on the 2n-point coset OFFSET * <w_2n> only - every
        // 2^(lb-1)-th row of the LDE, the LDE itself at lb = 1 and copied out as columns of their own above it (freed with this block's
        // first half, before the composition commitment); the program's tables are those of that coset
        const uint64_t n2 = 2 * n;
        Dev q(ctx, 24 * n2);
        {
            std::vector<DevP> ce_buf;
            std::vector<const uint64_t *> ce_cols = trace_ev;
            if (lb > 1) {
                std::vector<uint64_t *> ce_out;
                for (size_t c = 0; c < trace_ev.size(); ++c) {
                    ce_buf.emplace_back(new Dev(ctx, 8 * n2));
                    ce_out.push_back(ce_buf.back()->u64());
                    ce_cols[c] = ce_buf.back()->u64();
                }
                ok(ss_subsample_rows_gl64(ctx, trace_ev.data(), (uint32_t)trace_ev.size(), n2, lb - 1, ce_out.data()));
            }
            ok(ss_eval_quotient_gl64x3(ctx, &prog, ce_cols.data(), (uint32_t)ce_cols.size(), log_n, 1, OFFSET, q.u64()));
        }
        // de-interleave the three coordinates, interpolate each over the coset (bit-reversed coefficients: the even ones first)
        std::vector<uint64_t *> qc;
        std::vector<DevP> qbuf;
        for (int t = 0; t < 3; ++t) {
            qbuf.emplace_back(new Dev(ctx, 8 * n2));
            qc.push_back(qbuf.back()->u64());
            ok(ss_dev_copy_2d(ctx, qc[t], 8, q.u8() + 8 * t, 24, 8, n2));
        }
        ok(ss_ntt_gl64(ctx, qc.data(), 3, log_n + 1, SS_NTT_INVERSE, OFFSET, SS_ORDER_NATURAL, SS_ORDER_BITREV));
        for (int half = 0; half < 2; ++half)
            for (int t = 0; t < 3; ++t) {
                keep.emplace_back(new Dev(ctx, 8 * n));
                ok(ss_dev_copy(ctx, keep.back()->p, qc[t] + half * n, 8 * n));
                comp_co.push_back(keep.back()->u64());
            }
        for (const uint64_t *c : comp_co) {                 // zero-padded to N in bit-reversed order, then the forward transform
            keep.emplace_back(new Dev(ctx, 8 * N));
            uint64_t *padded = keep.back()->u64();
            ok(ss_dev_zero(ctx, padded, 8 * N));
            ok(ss_dev_copy_2d(ctx, padded, 8u << lb, c, 8, 8, n));
            ok(ss_ntt_gl64(ctx, &padded, 1, log_n + lb, SS_NTT_FORWARD, OFFSET, SS_ORDER_BITREV, SS_ORDER_NATURAL));
            comp_ev.push_back(padded);
        }
    }
    Commitment comp_com = commit(comp_ev, 1, N);
    proof.comp_root = comp_com.root;
    coin.reseed_with_digest(proof.comp_root);
    // 5. out-of-domain evaluations
    const Fq3 z = coin.draw_fq3(), zc = pow3(z, 2);
    std::vector<uint32_t> mc, mo;
    for (auto &c : mask) { mc.push_back(c.first); mo.push_back(c.second); }
    proof.ood_trace.assign(3 * mask.size(), 0);
    ok(ss_ood_eval_gl64x3(ctx, trace_co.data(), (uint32_t)trace_co.size(), log_n, mc.data(), mo.data(), (uint32_t)mask.size(), z.data(), proof.ood_trace.data()));
    const uint32_t six[6] = {0, 1, 2, 3, 4, 5}, zeros[6] = {0, 0, 0, 0, 0, 0};
    proof.ood_comp.assign(18, 0);
    ok(ss_ood_eval_gl64x3(ctx, comp_co.data(), 6, log_n, six, zeros, 6, zc.data(), proof.ood_comp.data()));
    {
        std::vector<uint64_t> all(proof.ood_trace);
        all.insert(all.end(), proof.ood_comp.begin(), proof.ood_comp.end());
        coin.reseed_with_fq3s(all.data(), all.size());
    }
    // 6. DEEP composition
    const Fq3 gamma = coin.draw_fq3();
    std::vector<uint64_t> coefs;
    {
        Fq3 cur{1, 0, 0};
        for (size_t i = 0; i < mask.size() + 6; ++i) { coefs.insert(coefs.end(), cur.begin(), cur.end()); cur = mul3(cur, gamma); }
    }
    DevP layer(new Dev(ctx, 24 * N));
    ok(ss_deep_compose_gl64x3(ctx, trace_ev.data(), (uint32_t)trace_ev.size(), comp_ev.data(), 6, log_n, lb, OFFSET, mc.data(), mo.data(), (uint32_t)mask.size(),
                              proof.ood_trace.data(), coefs.data(), proof.ood_comp.data(), coefs.data() + 3 * mask.size(), z.data(), zc.data(), layer->u64()));
    // 7. FRI
    uint32_t log_fold = 0;
    while ((1u << log_fold) < opt.fold) ++log_fold;
    struct Layer { DevP evals; Commitment com; uint64_t rows; std::vector<const uint64_t *> segs; };
    std::vector<Layer> layers;
    uint32_t ll = log_n + lb;
    uint64_t off = OFFSET;
    for (uint32_t i = 0; i < n_layers; ++i) {
        Layer L;
        L.rows = (1ull << ll) / opt.fold;
        for (uint32_t k = 0; k < opt.fold; ++k) L.segs.push_back(layer->u64() + 3 * k * L.rows);
        L.com = commit(L.segs, 3, L.rows);
        coin.reseed_with_digest(L.com.root);
        const Fq3 a = coin.draw_fq3();
        DevP next(new Dev(ctx, 24 * L.rows));
        ok(ss_fri_fold_gl64x3(ctx, layer->u64(), ll, opt.fold, a.data(), off, 0, next->u64()));
        FriLayer fl;
        fl.root = L.com.root; fl.log_len = ll;
        proof.fri_layers.push_back(fl);
        L.evals = std::move(layer);
        layers.push_back(std::move(L));
        layer = std::move(next);
        ll -= log_fold;
        off = powm(off, opt.fold);
    }
    // remainder: interpolate the last layer (tiny) on the host
    {
        const uint64_t L = 1ull << ll;
        std::vector<uint64_t> last(3 * L);
        ok(ss_download(ctx, last.data(), layer->p, 24 * L));
        const uint64_t winv = invm(powm(7, (P - 1) >> ll)), oinv = invm(off), linv = invm(L % P);
        proof.remainder.assign(3 * L, 0);
        for (int t = 0; t < 3; ++t)
            for (uint64_t k = 0; k < L; ++k) {               // coefficient k = (1/L) sum_j v_j (w^-k)^j * off^-k
                uint64_t acc = 0, cur = 1;
                const uint64_t wk = powm(winv, k);
                for (uint64_t j = 0; j < L; ++j) { acc = addm(acc, mulm(last[3 * j + t], cur)); cur = mulm(cur, wk); }
                proof.remainder[3 * k + t] = mulm(mulm(acc, linv), powm(oinv, k));
            }
        for (uint64_t k = L >> lb; k < L; ++k)
            for (int t = 0; t < 3; ++t)
                if (proof.remainder[3 * k + t]) throw std::runtime_error("the FRI remainder is not of low degree: the DEEP composition is not the polynomial it must be");
        coin.reseed_with_fq3s(proof.remainder.data(), proof.remainder.size());
    }
    // 8. proof of work, queries, openings
    proof.pow_nonce = 0;
    if (opt.grinding) ok(ss_pow_grind(ctx, SS_COIN_SOLIDITY, coin.digest.data(), opt.grinding, &proof.pow_nonce));
    coin.reseed_with_int(proof.pow_nonce);
    const std::vector<uint64_t> positions = coin.draw_queries(opt.num_queries, N);
    proof.base = open(std::vector<const uint64_t *>(trace_ev.begin(), trace_ev.begin() + nbase), 1, base_com, N, positions);
    if (num_ext) proof.ext = open(std::vector<const uint64_t *>(trace_ev.begin() + nbase, trace_ev.end()), 1, ext_com, N, positions);
    proof.comp = open(comp_ev, 1, comp_com, N, positions);
    std::vector<uint64_t> pos = positions;
    for (size_t i = 0; i < layers.size(); ++i) {
        for (uint64_t &p : pos) p %= layers[i].rows;
        std::sort(pos.begin(), pos.end());
        pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
        proof.fri_layers[i].opening = open(layers[i].segs, 3, layers[i].com, layers[i].rows, pos);
    }
    ok(ss_ctx_sync(ctx));
    return proof;
}

}  // namespace gl
}  // namespace ssh
