// air_plain.hpp — the `plain` layout's AIR over the 64-bit field p = 2^64 - 2^32 + 1 with challenges in Fq3, in the C++ host: the
// mirror of sandstorm_amd/layouts/plain.py (cells, the 47 constraints in the reference's order, Hints, Tables, composition(),
// check_program(), mask()) and of air_program.py's lowering with ext=True.  The composition program it lowers is the Python
// lowering's code word for code word, constants in the same order, the same slot count and table descriptions:
// ss_eval_quotient_gl64x3 picks its compiled kernel by the FNV-1a hash of the code words (tools/gen_quotient_gl.py), so anything else
// would silently run the interpreter.  Everything a statement or a transcript decides - hints, challenges, alpha^k, g^(n-k) - is a
// constant interned by SYMBOL, never by value.  Free of the device runtime except PlainAir's optional table upload.
#pragma once
#include <cstdint>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "goldilocks_prover.hpp"

namespace ssh {
namespace gl {

// ---- Fq3 = Fp[X] / (X^3 - 2) on the host
static constexpr uint64_t GL_P = 0xFFFFFFFF00000001ull;
uint64_t fp_mul(uint64_t a, uint64_t b);
uint64_t fp_add(uint64_t a, uint64_t b);
uint64_t fp_sub(uint64_t a, uint64_t b);
uint64_t fp_pow(uint64_t a, uint64_t e);
uint64_t fp_inv(uint64_t a);                                 // 0 -> 0
uint64_t fp_root_of_unity(uint32_t log_n);                   // 7^((p-1) >> log_n)
Fq3 add3(const Fq3 &a, const Fq3 &b);
Fq3 sub3(const Fq3 &a, const Fq3 &b);
Fq3 scale3(const Fq3 &a, uint64_t s);
Fq3 inv3(const Fq3 &a);                                      // 0 -> 0
Fq3 pow3x(Fq3 a, uint64_t e);
inline Fq3 f3(uint64_t v) { return Fq3{v % GL_P, 0, 0}; }

// ---- the expression graph of air_program.py over Fq3: hash-consed; commutative operands ordered by a hash of the node's STRUCTURE
// (air_program.Expr._skey: the CRC-32 of the node's Python repr), so the DAG is the one Python builds
enum class XKind { X, Const, Const3, Sym, Trace, Table, Add, Sub, Mul, Inv };
struct XNode {
    XKind kind;
    int a = -1, b = -1;             // children
    uint64_t v = 0;                 // Const: the value; Const3: index into const3s(); Sym: index into symbols(); Trace: column; Table: index
    uint32_t off = 0;               // Trace: row offset
    uint32_t skey = 0;
};
class XGraph {
public:
    int x();
    int constant(uint64_t v);
    int constant3(const Fq3 &v);
    int sym(const std::string &name);
    int trace(uint32_t col, uint32_t row_offset);
    int table(uint32_t index);
    int add(int a, int b);
    int sub(int a, int b);
    int mul(int a, int b);
    int inv(int a);
    const std::vector<XNode> &nodes() const { return nodes_; }
    const std::vector<Fq3> &const3s() const { return const3s_; }
    const std::vector<std::string> &symbols() const { return symbols_; }
    int symbol_index(const std::string &name) const { auto it = sym_ix_.find(name); return it == sym_ix_.end() ? -1 : it->second; }
    bool leaf(int n) const { return nodes_[n].kind <= XKind::Table; }
private:
    int intern(XNode n, const std::string &repr);
    std::vector<XNode> nodes_;
    std::vector<Fq3> const3s_;
    std::vector<std::string> symbols_;
    std::map<std::string, int> sym_ix_;
    std::map<std::string, int> pool_;       // by the node's repr over child IDS: structural identity
};

// a lowered program whose constant table is filled per proof: a constant is a value, or a symbol's index
struct XConst { bool is_symbol; Fq3 value; int symbol; };
struct XProgram {
    std::vector<uint32_t> code;
    std::vector<XConst> consts;
    uint32_t n_slots = 0;
};
// air_program._lower_roots(roots, ext=True, checks): OUT after the single root, or CHECK k after each root
XProgram lower_ext(const XGraph &g, const std::vector<int> &roots, bool checks);
// air_program.evaluate_ext
Fq3 evaluate_ext(const XGraph &g, int root, const Fq3 &x, const std::function<Fq3(uint32_t, uint32_t)> &trace_at,
                 const std::function<Fq3(uint32_t)> &table_at, const std::vector<Fq3> &symbol_values);

// ---- the layout
struct PlainStatement {                                      // layouts/plain.py PublicInput
    uint64_t n_steps = 0, rc_min = 0, rc_max = 0;
    uint64_t program[2] = {0, 0}, execution[2] = {0, 0};     // the memory segments (begin, stop)
    std::vector<std::pair<uint64_t, uint64_t>> public_memory;
};
struct TableSpec { uint64_t p, e; bool inverse; };
struct PlainConstraint { std::string name, domain; std::vector<std::pair<uint64_t, uint64_t>> num, den; int numerator; };

class PlainAir {
public:
    // ctx may be NULL: a host-only handle (verification, dumping programs); otherwise the tables go up once, here
    PlainAir(ss_ctx *ctx, const PlainStatement &st);
    ~PlainAir();
    PlainAir(const PlainAir &) = delete;
    PlainAir &operator=(const PlainAir &) = delete;

    uint64_t n() const { return n_; }
    uint32_t log_n() const { return log_n_; }
    const std::vector<std::pair<uint32_t, uint32_t>> &mask() const { return mask_; }
    const Digest &statement_digest() const { return digest_; }
    const PlainStatement &statement() const { return st_; }
    const std::vector<PlainConstraint> &constraints() const { return constraints_; }
    const std::vector<TableSpec> &table_specs() const { return specs_; }
    const std::vector<uint64_t> &table_values() const { return table_values_; }
    const std::vector<uint32_t> &table_desc() const { return table_desc_; }
    const uint64_t *device_tables() const { return d_tables_; }
    ss_ctx *ctx() const { return ctx_; }

    Fq3 public_memory_quotient(const Fq3 &z, const Fq3 &alpha) const;
    // the composition program for these challenges and this coefficient: only the constant table is made here
    ProgramData program(const std::vector<Fq3> &challenges, const Fq3 &alpha) const;
    CheckBlob check_program(const std::vector<Fq3> &challenges) const;
    // the composition at an Fq3 point from the out-of-domain values (the verifier's side of the AIR identity)
    Fq3 evaluate(const std::vector<Fq3> &challenges, const Fq3 &alpha, const Fq3 &z, const std::function<Fq3(uint32_t, uint32_t)> &trace_at) const;
    Fq3 table_value_at(const TableSpec &spec, const Fq3 &x) const;

private:
    std::vector<Fq3> symbol_values(const std::vector<Fq3> &challenges, const Fq3 *alpha) const;
    std::vector<uint64_t> fill_consts(const XProgram &p, const std::vector<Fq3> &sv) const;
    ss_ctx *ctx_;
    PlainStatement st_;
    uint64_t n_, g_;
    uint32_t log_n_;
    XGraph graph_;
    int root_ = -1;
    std::vector<PlainConstraint> constraints_;
    std::vector<TableSpec> specs_;
    std::vector<uint64_t> table_values_;
    std::vector<uint32_t> table_desc_;
    uint64_t *d_tables_ = nullptr;
    XProgram comp_, check_;
    std::vector<std::pair<uint32_t, uint32_t>> mask_;
    Digest digest_;
    std::pair<uint64_t, uint64_t> padding_{0, 0};
};

Digest plain_statement_digest(const PlainStatement &st);

}  // namespace gl
}  // namespace ssh
