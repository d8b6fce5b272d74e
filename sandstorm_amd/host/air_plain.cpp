// air_plain.cpp — see air_plain.hpp.  layouts/plain.py and air_program.py are the specification: the constraints below are their
// expressions restated operator for operator, because the lowered program has to be the same code words.
#include "air_plain.hpp"

#include <algorithm>
#include <cstring>
#include <set>
#include <stdexcept>

namespace ssh {
namespace gl {

// ---- the field
uint64_t fp_mul(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % GL_P); }
uint64_t fp_add(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a + b) % GL_P); }
uint64_t fp_sub(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a + GL_P - b % GL_P) % GL_P); }
uint64_t fp_pow(uint64_t a, uint64_t e) { uint64_t r = 1; for (; e; e >>= 1) { if (e & 1) r = fp_mul(r, a); a = fp_mul(a, a); } return r; }
uint64_t fp_inv(uint64_t a) { return fp_pow(a % GL_P, GL_P - 2); }
uint64_t fp_root_of_unity(uint32_t log_n) { return fp_pow(7, (GL_P - 1) >> log_n); }
Fq3 add3(const Fq3 &a, const Fq3 &b) { return Fq3{fp_add(a[0], b[0]), fp_add(a[1], b[1]), fp_add(a[2], b[2])}; }
Fq3 sub3(const Fq3 &a, const Fq3 &b) { return Fq3{fp_sub(a[0], b[0]), fp_sub(a[1], b[1]), fp_sub(a[2], b[2])}; }
Fq3 scale3(const Fq3 &a, uint64_t s) { return Fq3{fp_mul(a[0], s), fp_mul(a[1], s), fp_mul(a[2], s)}; }
Fq3 inv3(const Fq3 &a) {                                   // adjugate over the norm (layouts/plain.py inv3)
    const uint64_t two = 2;
    const Fq3 adj{fp_sub(fp_mul(a[0], a[0]), fp_mul(two, fp_mul(a[1], a[2]))), fp_sub(fp_mul(two, fp_mul(a[2], a[2])), fp_mul(a[0], a[1])),
                  fp_sub(fp_mul(a[1], a[1]), fp_mul(a[0], a[2]))};
    const uint64_t norm = fp_add(fp_mul(a[0], adj[0]), fp_add(fp_mul(two, fp_mul(a[2], adj[1])), fp_mul(two, fp_mul(a[1], adj[2]))));
    if (!norm) return Fq3{0, 0, 0};
    return scale3(adj, fp_inv(norm));
}
Fq3 pow3x(Fq3 a, uint64_t e) { Fq3 r{1, 0, 0}; for (; e; e >>= 1) { if (e & 1) r = mul3(r, a); a = mul3(a, a); } return r; }

// ---- the graph
namespace {
uint32_t crc32_of(const std::string &s) {                  // zlib.crc32
    static uint32_t table[256];
    static bool made = false;
    if (!made) {
        for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; table[i] = c; }
        made = true;
    }
    uint32_t c = 0xFFFFFFFFu;
    for (unsigned char ch : s) c = table[(c ^ ch) & 0xff] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
std::string u(uint64_t v) { return std::to_string(v); }
}  // namespace

int XGraph::intern(XNode n, const std::string &key) {
    auto it = pool_.find(key);
    if (it != pool_.end()) return it->second;
    // Python's repr((kind, *args)) with an Expr argument shown as ('e', its _skey)
    auto e = [&](int c) { return "('e', " + u(nodes_[c].skey) + ")"; };
    std::string r;
    switch (n.kind) {
    case XKind::X: r = "('x',)"; break;
    case XKind::Const: r = "('const', " + u(n.v) + ")"; break;
    case XKind::Const3: { const Fq3 &c = const3s_[n.v]; r = "('const3', " + u(c[0]) + ", " + u(c[1]) + ", " + u(c[2]) + ")"; break; }
    case XKind::Sym: r = "('sym', '" + symbols_[n.v] + "')"; break;
    case XKind::Trace: r = "('trace', " + u(n.v) + ", " + u(n.off) + ")"; break;
    case XKind::Table: r = "('table', " + u(n.v) + ")"; break;
    case XKind::Add: r = "('add', " + e(n.a) + ", " + e(n.b) + ")"; break;
    case XKind::Sub: r = "('sub', " + e(n.a) + ", " + e(n.b) + ")"; break;
    case XKind::Mul: r = "('mul', " + e(n.a) + ", " + e(n.b) + ")"; break;
    case XKind::Inv: r = "('inv', " + e(n.a) + ")"; break;
    }
    n.skey = crc32_of(r);
    nodes_.push_back(n);
    return pool_[key] = (int)nodes_.size() - 1;
}
int XGraph::x() { XNode n; n.kind = XKind::X; return intern(n, "x"); }
int XGraph::constant(uint64_t v) { XNode n; n.kind = XKind::Const; n.v = v; return intern(n, "c" + u(v)); }
int XGraph::constant3(const Fq3 &v) {
    const std::string key = "c3 " + u(v[0]) + " " + u(v[1]) + " " + u(v[2]);
    auto it = pool_.find(key);
    if (it != pool_.end()) return it->second;
    XNode n; n.kind = XKind::Const3; n.v = const3s_.size();
    const3s_.push_back(v);
    return intern(n, key);
}
int XGraph::sym(const std::string &name) {
    const std::string key = "s" + name;
    auto it = pool_.find(key);
    if (it != pool_.end()) return it->second;
    XNode n; n.kind = XKind::Sym; n.v = symbols_.size();
    sym_ix_[name] = (int)symbols_.size();
    symbols_.push_back(name);
    return intern(n, key);
}
int XGraph::trace(uint32_t col, uint32_t off) { XNode n; n.kind = XKind::Trace; n.v = col; n.off = off; return intern(n, "t" + u(col) + " " + u(off)); }
int XGraph::table(uint32_t index) { XNode n; n.kind = XKind::Table; n.v = index; return intern(n, "T" + u(index)); }
static bool skey_less(const std::vector<XNode> &nodes, int a, int b) {
    return nodes[a].skey != nodes[b].skey ? nodes[a].skey < nodes[b].skey : a < b;
}
int XGraph::add(int a, int b) { if (skey_less(nodes_, b, a)) std::swap(a, b); XNode n; n.kind = XKind::Add; n.a = a; n.b = b; return intern(n, "+" + u(a) + " " + u(b)); }
int XGraph::mul(int a, int b) { if (skey_less(nodes_, b, a)) std::swap(a, b); XNode n; n.kind = XKind::Mul; n.a = a; n.b = b; return intern(n, "*" + u(a) + " " + u(b)); }
int XGraph::sub(int a, int b) { XNode n; n.kind = XKind::Sub; n.a = a; n.b = b; return intern(n, "-" + u(a) + " " + u(b)); }
int XGraph::inv(int a) { XNode n; n.kind = XKind::Inv; n.a = a; return intern(n, "/" + u(a)); }

// ---- the lowering: air_program._lower_roots, call for call (a constant enters the table the first time operand() meets it, so
// the ORDER of those calls is part of what is mirrored)
namespace {
struct XLowerer {
    const XGraph &g;
    XProgram prog;
    std::vector<int> uses, need_of;
    std::map<int, uint32_t> slot_of;
    std::vector<uint32_t> free_slots;
    std::map<std::string, uint32_t> const_ix;

    explicit XLowerer(const XGraph &gr) : g(gr), uses(gr.nodes().size(), 0), need_of(gr.nodes().size(), -1) {}
    uint32_t alloc_slot() {
        if (!free_slots.empty()) { uint32_t s = free_slots.back(); free_slots.pop_back(); return s; }
        return prog.n_slots++;
    }
    void emit(uint32_t op, uint32_t dst, uint32_t kind = 0, uint32_t payload = 0) {
        prog.code.push_back(op | (dst << 8) | (kind << 12));
        prog.code.push_back(payload);
    }
    uint32_t const_value(const Fq3 &v) {
        const std::string key = "v" + u(v[0]) + " " + u(v[1]) + " " + u(v[2]);
        auto it = const_ix.find(key);
        if (it != const_ix.end()) return it->second;
        prog.consts.push_back(XConst{false, v, -1});
        return const_ix[key] = (uint32_t)prog.consts.size() - 1;
    }
    bool operand(int n, uint32_t &kind, uint32_t &payload) {
        const XNode &nd = g.nodes()[n];
        switch (nd.kind) {
        case XKind::X: kind = SS_SRC_X; payload = 0; return true;
        case XKind::Const: kind = SS_SRC_CONST; payload = const_value(f3(nd.v)); return true;
        case XKind::Const3: { const Fq3 &c = g.const3s()[nd.v]; kind = SS_SRC_CONST; payload = const_value(Fq3{c[0] % GL_P, c[1] % GL_P, c[2] % GL_P}); return true; }
        case XKind::Sym: {
            const std::string key = "s" + g.symbols()[nd.v];
            auto it = const_ix.find(key);
            if (it == const_ix.end()) { prog.consts.push_back(XConst{true, Fq3{0, 0, 0}, (int)nd.v}); it = const_ix.emplace(key, (uint32_t)prog.consts.size() - 1).first; }
            kind = SS_SRC_CONST; payload = it->second; return true; }
        case XKind::Trace: kind = SS_SRC_TRACE; payload = ((uint32_t)nd.v << 24) | nd.off; return true;
        case XKind::Table: kind = SS_SRC_TABLE; payload = (uint32_t)nd.v; return true;
        default: break;
        }
        auto it = slot_of.find(n);
        if (it == slot_of.end()) return false;
        kind = SS_SRC_SLOT; payload = it->second;
        return true;
    }
    bool has_operand(int n) { uint32_t k, p; return operand(n, k, p); }
    void emit_op(uint32_t opc, uint32_t dst, int n) { uint32_t k = 0, p = 0; operand(n, k, p); emit(opc, dst, k, p); }
    void consume(int n) {
        if (g.leaf(n)) return;
        if (--uses[n] == 0) { auto it = slot_of.find(n); if (it != slot_of.end()) { free_slots.push_back(it->second); slot_of.erase(it); } }
    }
    int need(int n) {                                        // accumulators a fresh evaluation takes (leaves: 0)
        if (g.leaf(n)) return 0;
        if (need_of[n] >= 0) return need_of[n];
        const XNode &nd = g.nodes()[n];
        int v;
        if (nd.kind == XKind::Inv) v = std::max(1, need(nd.a));
        else {
            const int a = need(nd.a), b = need(nd.b);
            v = std::max(1, nd.a == nd.b ? a : (a == b ? a + 1 : std::max(a, b)));
        }
        return need_of[n] = v;
    }
    void gen(int n, uint32_t dst) {
        uint32_t k, p;
        if (operand(n, k, p)) { emit(SS_OP_MOV, dst, k, p); consume(n); return; }
        const XNode &nd = g.nodes()[n];
        if (nd.kind == XKind::Inv) {
            gen(nd.a, dst);
            emit(SS_OP_INV, dst);
        } else {
            const int l = nd.a, r = nd.b;
            const uint32_t opc = nd.kind == XKind::Add ? SS_OP_ADD : nd.kind == XKind::Sub ? SS_OP_SUB : SS_OP_MUL;
            const uint32_t rev = nd.kind == XKind::Sub ? (uint32_t)SS_OP_RSUB : opc;
            if (l == r && !has_operand(l)) {
                --uses[l];                                   // both references served by one evaluation
                gen(l, dst);
                emit(opc, dst, SS_SRC_ACC, dst);
            } else if (has_operand(r)) {
                gen(l, dst);
                emit_op(opc, dst, r);
                consume(r);
            } else if (has_operand(l)) {
                gen(r, dst);
                emit_op(rev, dst, l);
                consume(l);
            } else {
                // both operands need code: the one that needs more accumulators goes first (Sethi-Ullman)
                const bool swapped = need(l) < need(r);
                const int first = swapped ? r : l, second = swapped ? l : r;
                const uint32_t op_ab = swapped ? rev : opc;
                gen(first, dst);
                if (has_operand(second)) { emit_op(op_ab, dst, second); consume(second); }
                else if (dst + 1 < 4) { gen(second, dst + 1); emit(op_ab, dst, SS_SRC_ACC, dst + 1); }
                else {
                    const uint32_t s = alloc_slot();
                    emit(SS_OP_ST, dst, 0, s);
                    gen(second, dst);
                    emit(swapped ? opc : rev, dst, SS_SRC_SLOT, s);   // acc[dst] holds `second` now, the slot `first`
                    free_slots.push_back(s);
                }
            }
        }
        if (--uses[n] > 0) {                                 // more parents: park it
            const uint32_t s = alloc_slot();
            slot_of[n] = s;
            emit(SS_OP_ST, dst, 0, s);
        }
    }
};
}  // namespace

XProgram lower_ext(const XGraph &g, const std::vector<int> &roots, bool checks) {
    XLowerer L(g);
    std::vector<char> seen(g.nodes().size(), 0);
    std::vector<int> stack(roots.begin(), roots.end());
    while (!stack.empty()) {
        const int n = stack.back(); stack.pop_back();
        if (seen[n]) continue;
        seen[n] = 1;
        const XNode &nd = g.nodes()[n];
        for (int c : {nd.a, nd.b}) if (c >= 0) { ++L.uses[c]; stack.push_back(c); }
    }
    for (int r : roots) ++L.uses[r];
    for (size_t k = 0; k < roots.size(); ++k) {
        L.gen(roots[k], 0);
        if (checks) L.emit(SS_OP_CHECK, 0, 0, (uint32_t)k); else L.emit(SS_OP_OUT, 0);
    }
    return L.prog;
}

Fq3 evaluate_ext(const XGraph &g, int root, const Fq3 &x, const std::function<Fq3(uint32_t, uint32_t)> &trace_at,
                 const std::function<Fq3(uint32_t)> &table_at, const std::vector<Fq3> &sv) {
    const auto &nodes = g.nodes();
    std::vector<Fq3> val(nodes.size());
    std::vector<char> done(nodes.size(), 0);
    std::vector<int> stack{root};
    while (!stack.empty()) {                                 // iterative post-order: children first
        const int id = stack.back();
        if (done[id]) { stack.pop_back(); continue; }
        const XNode &nd = nodes[id];
        const bool need_a = nd.a >= 0 && !done[nd.a], need_b = nd.b >= 0 && !done[nd.b];
        if (need_a) stack.push_back(nd.a);
        if (need_b) stack.push_back(nd.b);
        if (need_a || need_b) continue;
        switch (nd.kind) {
        case XKind::X: val[id] = x; break;
        case XKind::Const: val[id] = f3(nd.v); break;
        case XKind::Const3: val[id] = g.const3s()[nd.v]; break;
        case XKind::Sym: val[id] = sv.at(nd.v); break;
        case XKind::Trace: val[id] = trace_at((uint32_t)nd.v, nd.off); break;
        case XKind::Table: val[id] = table_at((uint32_t)nd.v); break;
        case XKind::Add: val[id] = add3(val[nd.a], val[nd.b]); break;
        case XKind::Sub: val[id] = sub3(val[nd.a], val[nd.b]); break;
        case XKind::Mul: val[id] = mul3(val[nd.a], val[nd.b]); break;
        case XKind::Inv: val[id] = inv3(val[nd.a]); break;
        }
        done[id] = 1;
        stack.pop_back();
    }
    return val[root];
}

// ---- the layout's expressions.  E is air_program.Expr's operators over the graph being built
namespace {
thread_local XGraph *G = nullptr;
struct E {
    int id;
    E operator+(const E &o) const { return E{G->add(id, o.id)}; }
    E operator-(const E &o) const { return E{G->sub(id, o.id)}; }
    E operator*(const E &o) const { return E{G->mul(id, o.id)}; }
    E inverse() const { return E{G->inv(id)}; }
};
E C(uint64_t v) { return E{G->constant(v)}; }
E S(const std::string &name) { return E{G->sym(name)}; }
E T(uint32_t col, uint32_t off) { return E{G->trace(col, off)}; }

enum { COL_FLAGS = 0, COL_NPC = 1, COL_MEMORY = 2, COL_RANGE_CHECK = 3, COL_AUXILIARY = 4, NUM_BASE = 5 };
enum { CYCLE = 16, PUBLIC_MEMORY_STEP = 8, MEMORY_STEP = 2, RANGE_CHECK_STEP = 4 };
// enum Flag (binary/src/lib.rs:740-772)
enum { DST_REG, OP0_REG, OP1_IMM, OP1_FP, OP1_AP, RES_ADD, RES_MUL, PC_JUMP_ABS, PC_JUMP_REL, PC_JNZ, AP_ADD, AP_ADD1, OPCODE_CALL, OPCODE_RET, OPCODE_ASSERT_EQ };
namespace Npc { enum { PC = 0, INSTRUCTION = 1, PUB_MEM_ADDR = 2, PUB_MEM_VAL = 3, MEM_OP0_ADDR = 4, MEM_OP0 = 5, MEM_DST_ADDR = 8, MEM_DST = 9, MEM_OP1_ADDR = 12, MEM_OP1 = 13 }; }
namespace Rc { enum { OFF_DST = 0, ORDERED = 2, OFF_OP1 = 4, OFF_OP0 = 8 }; }
struct Cell { uint32_t col, off; };
const Cell AUX_AP{COL_RANGE_CHECK, 3}, AUX_OP0_MUL_OP1{COL_RANGE_CHECK, 7}, AUX_FP{COL_RANGE_CHECK, 11}, AUX_RES{COL_RANGE_CHECK, 15};
const Cell AUX_TMP0{COL_AUXILIARY, 0}, AUX_TMP1{COL_AUXILIARY, 8};

E flag(uint32_t f) { return T(COL_FLAGS, f) - (T(COL_FLAGS, f + 1) + T(COL_FLAGS, f + 1)); }
E npc(uint32_t cell, uint32_t cycle = 0) { return T(COL_NPC, CYCLE * cycle + cell); }
E rc(uint32_t cell, uint32_t cycle = 0) { return T(COL_RANGE_CHECK, CYCLE * cycle + cell); }
E aux(const Cell &c, uint32_t cycle = 0) { return T(c.col, CYCLE * cycle + c.off); }
E mem(uint32_t cell, uint32_t step = 0) { return T(COL_MEMORY, MEMORY_STEP * step + cell); }
E rc_ordered(uint32_t step = 0) { return T(COL_RANGE_CHECK, RANGE_CHECK_STEP * step + Rc::ORDERED); }
E perm(uint32_t off) {
    const E x1{G->constant3(Fq3{0, 1, 0})}, x2{G->constant3(Fq3{0, 0, 1})};
    return T(NUM_BASE, off) + x1 * T(NUM_BASE + 1, off) + x2 * T(NUM_BASE + 2, off);
}
E perm_memory(uint32_t step = 0) { return perm(MEMORY_STEP * step); }
E perm_range_check(uint32_t step = 0) { return perm(4 * step + 1); }

using Factors = std::vector<std::pair<uint64_t, uint64_t>>;
struct Domain { const char *name; std::function<Factors(uint64_t)> num, den; };
Domain every(uint64_t k, const char *name) {
    return Domain{name, [](uint64_t) { return Factors{}; }, [k](uint64_t n) { return Factors{{n / k, 0}}; }};
}
Domain every_except_last(uint64_t k, const char *name) {
    return Domain{name, [k](uint64_t n) { return Factors{{1, n - k}}; }, [k](uint64_t n) { return Factors{{n / k, 0}}; }};
}
Domain row_from_end(uint64_t k, const char *name) {
    return Domain{name, [](uint64_t) { return Factors{}; }, [k](uint64_t n) { return Factors{{1, n - k}}; }};
}

struct Built { std::string name; E numerator; Domain domain; };

// layouts/recursive.py cpu_constraints over this layout's cells, then layouts/plain.py constraints()' 14, with every hint and challenge
// a named constant
std::vector<Built> build_constraints() {
    const Domain ALL_CYCLES = every(CYCLE, "every cycle"), ALL_CYCLES_EXCEPT_LAST = every_except_last(CYCLE, "every cycle but the last");
    const Domain FLAG_ROWS{"every row holding a flag", [](uint64_t n) { return Factors{{n / CYCLE, 15 * n / CYCLE}}; }, [](uint64_t n) { return Factors{{n, 0}}; }};
    const Domain FLAG_ZERO_ROWS{"the 16th row of every cycle", [](uint64_t) { return Factors{}; }, [](uint64_t n) { return Factors{{n / CYCLE, 15 * n / CYCLE}}; }};
    const Domain FIRST_ROW{"first row", [](uint64_t) { return Factors{}; }, [](uint64_t) { return Factors{{1, 0}}; }};
    const Domain LAST_CYCLE = row_from_end(CYCLE, "first row of the last cycle");
    const Domain EVERY_2ND_EXCEPT_LAST = every_except_last(2, "every 2nd row but the last"), SECOND_LAST_ROW = row_from_end(2, "row n-2");
    const Domain EVERY_4TH_EXCEPT_LAST = every_except_last(4, "every 4th row but the last"), FOURTH_LAST_ROW = row_from_end(4, "row n-4");
    const Domain EVERY_8TH_ROW = every(8, "every 8th row");

    const E h_initial_ap = S("hint:initial_ap"), h_initial_pc = S("hint:initial_pc"), h_final_ap = S("hint:final_ap"), h_final_pc = S("hint:final_pc");
    const E h_rc_min = S("hint:range_check_min"), h_rc_max = S("hint:range_check_max"), h_memory_quotient = S("hint:memory_quotient");
    const E h_rc_product = S("hint:range_check_product");
    const E one = C(1), two = C(2), four = C(4), offset_size = C(1 << 16), half_offset_size = C(1 << 15);
    const E flag_op1_base_op0_0 = one - (flag(OP1_IMM) + flag(OP1_AP) + flag(OP1_FP));
    const E flag_res_op1_0 = one - (flag(RES_ADD) + flag(RES_MUL) + flag(PC_JNZ));
    const E flag_pc_update_regular_0 = one - (flag(PC_JUMP_ABS) + flag(PC_JUMP_REL) + flag(PC_JNZ));
    const E fp_update_regular_0 = one - (flag(OPCODE_CALL) + flag(OPCODE_RET));
    const E npc_reg_0 = npc(Npc::PC) + flag(OP1_IMM) + one;
    const E whole_flag_prefix = T(COL_FLAGS, 0);
    std::vector<Built> c;
    auto add = [&](const char *name, const E &numerator, const Domain &d) { c.push_back(Built{name, numerator, d}); };

    add("cpu/decode/opcode_rc/bit", flag(DST_REG) * flag(DST_REG) - flag(DST_REG), FLAG_ROWS);
    add("cpu/decode/opcode_rc/zero", whole_flag_prefix, FLAG_ZERO_ROWS);
    add("cpu/decode/opcode_rc_input",
        npc(Npc::INSTRUCTION) - (((whole_flag_prefix * offset_size + rc(Rc::OFF_OP1)) * offset_size + rc(Rc::OFF_OP0)) * offset_size + rc(Rc::OFF_DST)), ALL_CYCLES);
    add("cpu/decode/flag_op1_base_op0_bit", flag_op1_base_op0_0 * flag_op1_base_op0_0 - flag_op1_base_op0_0, ALL_CYCLES);
    add("cpu/decode/flag_res_op1_bit", flag_res_op1_0 * flag_res_op1_0 - flag_res_op1_0, ALL_CYCLES);
    add("cpu/decode/flag_pc_update_regular_bit", flag_pc_update_regular_0 * flag_pc_update_regular_0 - flag_pc_update_regular_0, ALL_CYCLES);
    add("cpu/decode/fp_update_regular_bit", fp_update_regular_0 * fp_update_regular_0 - fp_update_regular_0, ALL_CYCLES);
    add("cpu/operands/mem_dst_addr",
        npc(Npc::MEM_DST_ADDR) + half_offset_size - (flag(DST_REG) * aux(AUX_FP) + (one - flag(DST_REG)) * aux(AUX_AP) + rc(Rc::OFF_DST)), ALL_CYCLES);
    add("cpu/operands/mem0_addr",
        npc(Npc::MEM_OP0_ADDR) + half_offset_size - (flag(OP0_REG) * aux(AUX_FP) + (one - flag(OP0_REG)) * aux(AUX_AP) + rc(Rc::OFF_OP0)), ALL_CYCLES);
    add("cpu/operands/mem1_addr",
        npc(Npc::MEM_OP1_ADDR) + half_offset_size
            - (flag(OP1_IMM) * npc(Npc::PC) + flag(OP1_AP) * aux(AUX_AP) + flag(OP1_FP) * aux(AUX_FP) + flag_op1_base_op0_0 * npc(Npc::MEM_OP0) + rc(Rc::OFF_OP1)),
        ALL_CYCLES);
    add("cpu/operands/ops_mul", aux(AUX_OP0_MUL_OP1) - npc(Npc::MEM_OP0) * npc(Npc::MEM_OP1), ALL_CYCLES);
    add("cpu/operands/res",
        (one - flag(PC_JNZ)) * aux(AUX_RES)
            - (flag(RES_ADD) * (npc(Npc::MEM_OP0) + npc(Npc::MEM_OP1)) + flag(RES_MUL) * aux(AUX_OP0_MUL_OP1) + flag_res_op1_0 * npc(Npc::MEM_OP1)),
        ALL_CYCLES);
    add("cpu/update_registers/update_pc/tmp0", aux(AUX_TMP0) - flag(PC_JNZ) * npc(Npc::MEM_DST), ALL_CYCLES_EXCEPT_LAST);
    add("cpu/update_registers/update_pc/tmp1", aux(AUX_TMP1) - aux(AUX_TMP0) * aux(AUX_RES), ALL_CYCLES_EXCEPT_LAST);
    add("cpu/update_registers/update_pc/pc_cond_negative",
        (one - flag(PC_JNZ)) * npc(Npc::PC, 1) + aux(AUX_TMP0) * (npc(Npc::PC, 1) - (npc(Npc::PC) + npc(Npc::MEM_OP1)))
            - (flag_pc_update_regular_0 * npc_reg_0 + flag(PC_JUMP_ABS) * aux(AUX_RES) + flag(PC_JUMP_REL) * (npc(Npc::PC) + aux(AUX_RES))),
        ALL_CYCLES_EXCEPT_LAST);
    add("cpu/update_registers/update_pc/pc_cond_positive", (aux(AUX_TMP1) - flag(PC_JNZ)) * (npc(Npc::PC, 1) - npc_reg_0), ALL_CYCLES_EXCEPT_LAST);
    add("cpu/update_registers/update_ap/ap_update",
        aux(AUX_AP, 1) - (aux(AUX_AP) + flag(AP_ADD) * aux(AUX_RES) + flag(AP_ADD1) + flag(OPCODE_CALL) * two), ALL_CYCLES_EXCEPT_LAST);
    add("cpu/update_registers/update_fp/fp_update",
        aux(AUX_FP, 1) - (fp_update_regular_0 * aux(AUX_FP) + flag(OPCODE_RET) * npc(Npc::MEM_DST) + flag(OPCODE_CALL) * (aux(AUX_AP) + two)), ALL_CYCLES_EXCEPT_LAST);
    add("cpu/opcodes/call/push_fp", flag(OPCODE_CALL) * (npc(Npc::MEM_DST) - aux(AUX_FP)), ALL_CYCLES);
    add("cpu/opcodes/call/push_pc", flag(OPCODE_CALL) * (npc(Npc::MEM_OP0) - (npc(Npc::PC) + flag(OP1_IMM) + one)), ALL_CYCLES);
    add("cpu/opcodes/call/off0", flag(OPCODE_CALL) * (rc(Rc::OFF_DST) - half_offset_size), ALL_CYCLES);
    add("cpu/opcodes/call/off1", flag(OPCODE_CALL) * (rc(Rc::OFF_OP0) - (half_offset_size + one)), ALL_CYCLES);
    add("cpu/opcodes/call/flags", flag(OPCODE_CALL) * (flag(OPCODE_CALL) + flag(OPCODE_CALL) + one + one - (flag(DST_REG) + flag(OP0_REG) + four)), ALL_CYCLES);
    add("cpu/opcodes/ret/off0", flag(OPCODE_RET) * (rc(Rc::OFF_DST) + two - half_offset_size), ALL_CYCLES);
    add("cpu/opcodes/ret/off2", flag(OPCODE_RET) * (rc(Rc::OFF_OP1) + one - half_offset_size), ALL_CYCLES);
    add("cpu/opcodes/ret/flags", flag(OPCODE_RET) * (flag(PC_JUMP_ABS) + flag(DST_REG) + flag(OP1_FP) + flag_res_op1_0 - four), ALL_CYCLES);
    add("cpu/opcodes/assert_eq/assert_eq", flag(OPCODE_ASSERT_EQ) * (npc(Npc::MEM_DST) - aux(AUX_RES)), ALL_CYCLES);
    add("initial_ap", aux(AUX_AP) - h_initial_ap, FIRST_ROW);
    add("initial_fp", aux(AUX_FP) - h_initial_ap, FIRST_ROW);
    add("initial_pc", npc(Npc::PC) - h_initial_pc, FIRST_ROW);
    add("final_ap", aux(AUX_AP) - h_final_ap, LAST_CYCLE);
    add("final_fp", aux(AUX_FP) - h_initial_ap, LAST_CYCLE);
    add("final_pc", npc(Npc::PC) - h_final_pc, LAST_CYCLE);

    const E z = S("challenge:0"), a = S("challenge:1"), zr = S("challenge:2");
    const E address_diff = mem(0, 1) - mem(0);
    const E diff = rc_ordered(1) - rc_ordered();
    add("memory/multi_column_perm/perm/init0", (z - (mem(0) + a * mem(1))) * perm_memory() + npc(Npc::PC) + a * npc(Npc::INSTRUCTION) - z, FIRST_ROW);
    add("memory/multi_column_perm/perm/step0",
        (z - (mem(0, 1) + a * mem(1, 1))) * perm_memory(1) - (z - (T(COL_NPC, 2) + a * T(COL_NPC, 3))) * perm_memory(), EVERY_2ND_EXCEPT_LAST);
    add("memory/multi_column_perm/perm/last", perm_memory() - h_memory_quotient, SECOND_LAST_ROW);
    add("memory/diff_is_bit", address_diff * address_diff - address_diff, EVERY_2ND_EXCEPT_LAST);
    add("memory/is_func", (address_diff - one) * (mem(1) - mem(1, 1)), EVERY_2ND_EXCEPT_LAST);
    add("memory/initial_addr", mem(0) - one, FIRST_ROW);
    add("public_memory_addr_zero", npc(Npc::PUB_MEM_ADDR), EVERY_8TH_ROW);
    add("public_memory_value_zero", npc(Npc::PUB_MEM_VAL), EVERY_8TH_ROW);
    add("rc16/perm/init0", (zr - rc_ordered()) * perm_range_check() + rc(Rc::OFF_DST) - zr, FIRST_ROW);
    add("rc16/perm/step0", (zr - rc_ordered(1)) * perm_range_check(1) - (zr - T(COL_RANGE_CHECK, 4)) * perm_range_check(), EVERY_4TH_EXCEPT_LAST);
    add("rc16/perm/last", perm_range_check() - h_rc_product, FOURTH_LAST_ROW);
    add("rc16/diff_is_bit", diff * diff - diff, EVERY_4TH_EXCEPT_LAST);
    add("rc16/minimum", rc_ordered() - h_rc_min, FIRST_ROW);
    add("rc16/maximum", rc_ordered() - h_rc_max, FOURTH_LAST_ROW);
    return c;
}

// layouts/plain.py Tables: factors with p > 1 are tables, a single-row factor X - g^r is an expression and the single-row denominators
// share one inversion
struct TablesBuilder {
    uint64_t n;
    std::vector<TableSpec> specs;
    std::vector<uint64_t> single_rows;
    std::map<uint64_t, int> single_inv;
    explicit TablesBuilder(uint64_t n_) : n(n_) {
        std::set<uint64_t> rows{0 % n, (n - CYCLE) % n, (n - 2) % n, (n - 4) % n};
        single_rows.assign(rows.begin(), rows.end());
    }
    E row_point(uint64_t r) {
        r %= n;
        if (r == 0) return C(1);
        return S("g^(n-" + std::to_string(n - r) + ")");
    }
    E table(uint64_t p, uint64_t e, bool inverse) {
        for (size_t i = 0; i < specs.size(); ++i)
            if (specs[i].p == p && specs[i].e == e && specs[i].inverse == inverse) return E{G->table((uint32_t)i)};
        specs.push_back(TableSpec{p, e, inverse});
        return E{G->table((uint32_t)specs.size() - 1)};
    }
    E factor(uint64_t p, uint64_t e, bool inverse) {
        if (p != 1) return table(p, e, inverse);
        const E X{G->x()};
        const E f = X - row_point(e);
        if (!inverse) return f;
        if (std::find(single_rows.begin(), single_rows.end(), e % n) == single_rows.end() || single_rows.size() < 2) return f.inverse();
        if (single_inv.empty()) {
            std::vector<E> fs;
            for (uint64_t r : single_rows) fs.push_back(X - row_point(r));
            E prod = fs[0];
            for (size_t j = 1; j < fs.size(); ++j) prod = prod * fs[j];
            const E inv_all = prod.inverse();
            for (size_t k = 0; k < single_rows.size(); ++k) {
                E others{-1};
                for (size_t j = 0; j < fs.size(); ++j)
                    if (j != k) others = others.id < 0 ? fs[j] : others * fs[j];
                single_inv[single_rows[k]] = (inv_all * others).id;
            }
        }
        return E{single_inv.at(e % n)};
    }
    E multiplier(const Factors &num, const Factors &den) {
        E m{-1};
        for (auto &f : num) { const E v = factor(f.first, f.second, false); m = m.id < 0 ? v : m * v; }
        for (auto &f : den) { const E v = factor(f.first, f.second, true); m = m.id < 0 ? v : m * v; }
        return m;
    }
};

void be64(std::vector<uint8_t> &b, uint64_t v) { for (int k = 7; k >= 0; --k) b.push_back((uint8_t)(v >> (8 * k))); }
uint64_t gcd64(uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; }
}  // namespace

Digest plain_statement_digest(const PlainStatement &st) {   // goldilocks.py statement_digest
    std::vector<uint8_t> b;
    be64(b, st.n_steps); be64(b, st.rc_min); be64(b, st.rc_max); be64(b, 2);
    const std::pair<const char *, const uint64_t *> segs[2] = {{"execution", st.execution}, {"program", st.program}};     // sorted by name
    for (auto &s : segs) {
        const size_t len = strlen(s.first);
        be64(b, len);
        b.insert(b.end(), s.first, s.first + len);
        be64(b, s.second[0]); be64(b, s.second[1]);
    }
    be64(b, st.public_memory.size());
    for (auto &c : st.public_memory) { be64(b, c.first); be64(b, c.second); }
    return keccak256(b.data(), b.size());
}

PlainAir::PlainAir(ss_ctx *ctx, const PlainStatement &st) : ctx_(ctx), st_(st) {
    if (!st.n_steps || (st.n_steps & (st.n_steps - 1)) || st.n_steps > (1ull << 28)) throw std::runtime_error("plain AIR: the number of cycles must be a power of two, at most 2^28");
    n_ = CYCLE * st.n_steps;
    log_n_ = 0;
    while ((1ull << log_n_) < n_) ++log_n_;
    g_ = fp_root_of_unity(log_n_);
    bool have_padding = false;
    for (auto &c : st.public_memory) {
        if (c.second >= GL_P) throw std::runtime_error("plain AIR: a public-memory value is not an element of the field");
        if (c.first == 1 && !have_padding) { padding_ = c; have_padding = true; }
    }
    if (!have_padding) throw std::runtime_error("plain AIR: the public memory has no entry at address 1 (the padding cell)");
    digest_ = plain_statement_digest(st);

    G = &graph_;
    const std::vector<Built> built = build_constraints();
    TablesBuilder tables(n_);
    E root{-1};
    std::vector<int> numerators;
    std::set<std::pair<uint32_t, uint32_t>> cells;
    for (size_t k = 0; k < built.size(); ++k) {
        PlainConstraint pc;
        pc.name = built[k].name; pc.domain = built[k].domain.name;
        pc.num = built[k].domain.num(n_); pc.den = built[k].domain.den(n_);
        pc.numerator = built[k].numerator.id;
        if (pc.num.size() > SS_CHECK_MAX_FACTORS || pc.den.size() > SS_CHECK_MAX_FACTORS) throw std::runtime_error("plain AIR: a domain has too many factors");
        const E term = S("alpha^" + std::to_string(k)) * (built[k].numerator * tables.multiplier(pc.num, pc.den));
        root = root.id < 0 ? term : root + term;
        numerators.push_back(pc.numerator);
        constraints_.push_back(pc);
    }
    G = nullptr;
    root_ = root.id;
    specs_ = tables.specs;
    comp_ = lower_ext(graph_, {root_}, false);
    check_ = lower_ext(graph_, numerators, true);
    {                                                        // the mask: every trace cell a numerator reads, sorted
        std::vector<char> seen(graph_.nodes().size(), 0);
        std::vector<int> stack(numerators.begin(), numerators.end());
        while (!stack.empty()) {
            const int id = stack.back(); stack.pop_back();
            if (seen[id]) continue;
            seen[id] = 1;
            const XNode &nd = graph_.nodes()[id];
            if (nd.kind == XKind::Trace) cells.insert({(uint32_t)nd.v, nd.off});
            for (int c : {nd.a, nd.b}) if (c >= 0) stack.push_back(c);
        }
        mask_.assign(cells.begin(), cells.end());
    }
    // Tables.device_tables over the 2n-point coset with offset 7
    const uint64_t N = 2 * n_, wN = fp_root_of_unity(log_n_ + 1);
    for (const TableSpec &s : specs_) {
        const uint64_t len = N / gcd64(N, s.p);
        uint32_t log_len = 0;
        while ((1ull << log_len) < len) ++log_len;
        table_desc_.push_back((uint32_t)table_values_.size());
        table_desc_.push_back(log_len);
        const uint64_t step = fp_pow(wN, s.p), ge = fp_pow(g_, s.e);
        uint64_t cur = fp_pow(7, s.p);
        for (uint64_t i = 0; i < len; ++i) {
            const uint64_t v = fp_sub(cur, ge);
            table_values_.push_back(s.inverse && v ? fp_inv(v) : v);
            cur = fp_mul(cur, step);
        }
    }
    if (table_values_.empty()) table_values_.push_back(0);
    if (ctx_) {
        void *p = nullptr;
        if (ss_dev_alloc(ctx_, table_values_.size() * 8, &p) != SS_OK) throw std::runtime_error(ss_last_error());
        d_tables_ = (uint64_t *)p;
        if (ss_upload(ctx_, d_tables_, table_values_.data(), table_values_.size() * 8) != SS_OK) {
            const std::string err = ss_last_error();
            (void)ss_dev_free(ctx_, d_tables_);
            throw std::runtime_error(err);
        }
    }
}

PlainAir::~PlainAir() {
    if (d_tables_) { (void)ss_ctx_sync(ctx_); (void)ss_dev_free(ctx_, d_tables_); }
}

Fq3 PlainAir::public_memory_quotient(const Fq3 &z, const Fq3 &alpha) const {     // layouts/plain.py public_memory_quotient
    const uint64_t s = n_ / PUBLIC_MEMORY_STEP, count = st_.public_memory.size();
    if (count > s) throw std::runtime_error("public memory does not fit");
    Fq3 den{1, 0, 0};
    for (auto &c : st_.public_memory) den = mul3(den, sub3(z, add3(scale3(alpha, c.second % GL_P), f3(c.first))));
    den = mul3(den, pow3x(sub3(z, add3(scale3(alpha, padding_.second % GL_P), f3(padding_.first))), s - count));
    return mul3(pow3x(z, s), inv3(den));
}

std::vector<Fq3> PlainAir::symbol_values(const std::vector<Fq3> &ch, const Fq3 *alpha) const {
    if (ch.size() != 3) throw std::runtime_error("the plain layout draws three challenges");
    for (auto &c : ch) for (uint64_t v : c) if (v >= GL_P) throw std::runtime_error("plain AIR: a challenge is not an element of the extension");
    const auto &names = graph_.symbols();
    std::vector<Fq3> sv(names.size(), Fq3{0, 0, 0});
    std::vector<Fq3> alpha_pow;
    if (alpha) {
        for (uint64_t v : *alpha) if (v >= GL_P) throw std::runtime_error("plain AIR: the composition coefficient is not an element of the extension");
        Fq3 cur{1, 0, 0};
        for (size_t k = 0; k < constraints_.size(); ++k) { alpha_pow.push_back(cur); cur = mul3(cur, *alpha); }
    }
    for (size_t i = 0; i < names.size(); ++i) {
        const std::string &s = names[i];
        if (s == "hint:initial_ap") sv[i] = f3(st_.execution[0]);
        else if (s == "hint:initial_pc") sv[i] = f3(st_.program[0]);
        else if (s == "hint:final_ap") sv[i] = f3(st_.execution[1]);
        else if (s == "hint:final_pc") sv[i] = f3(st_.program[1]);
        else if (s == "hint:range_check_min") sv[i] = f3(st_.rc_min);
        else if (s == "hint:range_check_max") sv[i] = f3(st_.rc_max);
        else if (s == "hint:memory_quotient") sv[i] = public_memory_quotient(ch[0], ch[1]);
        else if (s == "hint:range_check_product") sv[i] = Fq3{1, 0, 0};
        else if (s.compare(0, 10, "challenge:") == 0) sv[i] = ch.at(std::stoul(s.substr(10)));
        else if (s.compare(0, 6, "alpha^") == 0) { if (alpha) sv[i] = alpha_pow.at(std::stoul(s.substr(6))); }
        else if (s.compare(0, 5, "g^(n-") == 0) sv[i] = f3(fp_pow(g_, n_ - std::stoull(s.substr(5))));
        else throw std::runtime_error("plain AIR: unknown symbol " + s);
    }
    return sv;
}

std::vector<uint64_t> PlainAir::fill_consts(const XProgram &p, const std::vector<Fq3> &sv) const {
    std::vector<uint64_t> out;
    out.reserve(3 * p.consts.size());
    for (const XConst &c : p.consts) {
        const Fq3 &v = c.is_symbol ? sv[c.symbol] : c.value;
        out.insert(out.end(), v.begin(), v.end());
    }
    return out;
}

ProgramData PlainAir::program(const std::vector<Fq3> &challenges, const Fq3 &alpha) const {
    ProgramData pd;
    pd.code = comp_.code;
    pd.consts = fill_consts(comp_, symbol_values(challenges, &alpha));
    pd.n_slots = comp_.n_slots;
    pd.d_tables = d_tables_;
    pd.table_desc = table_desc_;
    return pd;
}

CheckBlob PlainAir::check_program(const std::vector<Fq3> &challenges) const {
    CheckBlob cb;
    cb.code = check_.code;
    cb.consts = fill_consts(check_, symbol_values(challenges, nullptr));
    cb.n_slots = check_.n_slots;
    for (const PlainConstraint &c : constraints_) {
        ss_check_domain d;
        memset(&d, 0, sizeof d);
        d.n_num = (uint32_t)c.num.size(); d.n_den = (uint32_t)c.den.size();
        for (size_t j = 0; j < c.num.size(); ++j) { d.num[j][0] = c.num[j].first; d.num[j][1] = c.num[j].second; }
        for (size_t j = 0; j < c.den.size(); ++j) { d.den[j][0] = c.den[j].first; d.den[j][1] = c.den[j].second; }
        cb.domains.push_back(d);
        cb.names.push_back(c.name);
        cb.domain_names.push_back(c.domain);
    }
    return cb;
}

Fq3 PlainAir::table_value_at(const TableSpec &s, const Fq3 &x) const {
    const Fq3 v = sub3(pow3x(x, s.p), f3(fp_pow(g_, s.e)));
    return s.inverse ? inv3(v) : v;
}

Fq3 PlainAir::evaluate(const std::vector<Fq3> &challenges, const Fq3 &alpha, const Fq3 &z, const std::function<Fq3(uint32_t, uint32_t)> &trace_at) const {
    return evaluate_ext(graph_, root_, z, trace_at, [&](uint32_t t) { return table_value_at(specs_.at(t), z); }, symbol_values(challenges, &alpha));
}

}  // namespace gl
}  // namespace ssh
