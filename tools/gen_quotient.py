#!/usr/bin/env python3
"""Compile a layout's composition constraint into straight-line HIP ("stop interpreting the AIR").

The constraint program of a layout is static: `ssh::lower` (sandstorm_amd/host/air_program.cpp) turns the `Expr` DAG of
layouts/src/{starknet,recursive}/air.rs into the same instruction sequence for every statement of the layout - per-proof
values (challenges, hints, powers of the composition coefficient, powers of the trace generator) are interned by symbol,
not by value, so they only change the CONSTANT TABLE, never the code.  This tool takes that sequence from the C++ host
(`ssh_air_dump`) and writes sandstorm_amd/csrc/quotient_gen_<layout>.hip: one kernel whose body is the program unrolled,
with

  * the four accumulators and the scratch slots as register-resident 9 x 28-bit lazy values (no slot file in HBM),
  * operand kinds, column numbers, row offsets and table numbers as immediates,
  * constants read through the scalar cache, pre-limbed on the host (R256 limbs for add / sub / mov, R280 limbs for the
    cheaper fl_mul_r280),
  * the weak reductions of the lazy form placed here, at generation time, by the bound rules of csrc/quotient.hip.

ss_eval_quotient recognises a program by the hash of its code words and launches the compiled kernel for it; any other
program (the mini AIR, the random programs of the parity tests, a trace too short for the layout's usual shape) runs on
the interpreter of csrc/quotient.hip.  Both paths are held to the oracle's constraint VM (tests/test_gpu_real_quotient.py).

Usage (build container, after `make -C sandstorm_amd/host`):  python tools/gen_quotient.py [layout ...]
The generated sources are committed; the build does not run this tool.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT_DIR = os.environ.get("QG_OUT_DIR", os.path.join(ROOT, "sandstorm_amd", "csrc"))     # QG_OUT_DIR: write elsewhere (tests/test_quotient_gen_host.py
                                                                                          # checks that the committed sources are what this tool writes)
OP_MOV, OP_ADD, OP_SUB, OP_RSUB, OP_MUL, OP_INV, OP_ST, OP_OUT = range(8)
SRC_ACC, SRC_SLOT, SRC_CONST, SRC_TRACE, SRC_TABLE, SRC_X = range(6)
MAX_BOUND = 8           # csrc/quotient.hip VM_MAX_BOUND: value < 2 b p, limbs < b 2^28


def code_hash(code):
    """FNV-1a over the 32-bit code words: what ss_eval_quotient computes to recognise the program"""
    h = 0xcbf29ce484222325
    for w in code:
        for k in range(4):
            h = ((h ^ ((int(w) >> (8 * k)) & 0xff)) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def template_program(layout):
    """the layout's lowered program at a size and statement where it has its usual shape"""
    import numpy as np
    from oracle import oracle_py as oracle              # only its to_mont helper
    from sandstorm_amd import hostlib
    P = 2**251 + 17 * 2**192 + 1
    ch = [oracle.to_mont([pow(7, 11 + 3 * i, P)])[0] for i in range(6)]
    alpha = oracle.to_mont([pow(5, 77, P)])[0]
    if layout == "starknet":
        from test_layout_starknet import starknet_example
        _, _, pi = starknet_example(11)
        air = hostlib.StarknetHostAir(None, pi, 21)
        n = 1 << 21
    else:
        from test_layout_recursive import load_run
        _, _, pi = load_run()
        air = hostlib.RecursiveHostAir(None, pi, 18)
        n = 1 << 18
    code, consts, n_slots, specs = air.dump(n, ch, alpha)
    ncols = air.num_base_columns + air.num_extension_columns
    # the same program with other challenges, another composition coefficient and (starknet) another statement: what a constant is
    # in BOTH dumps it is by the layout's structure, not by the proof (structural_constants)
    ch2 = [oracle.to_mont([pow(11, 5 + 7 * i, P)])[0] for i in range(6)]
    alpha2 = oracle.to_mont([pow(3, 101, P)])[0]
    air2 = air
    if layout == "starknet":
        _, _, pi2 = starknet_example(12)
        air2 = hostlib.StarknetHostAir(None, pi2, 21)
    code2, consts2, _, _ = air2.dump(n, ch2, alpha2)
    if air2 is not air:
        air2.close()
    air.close()
    assert np.array_equal(np.asarray(code, dtype=np.uint32), np.asarray(code2, dtype=np.uint32)), "the program depends on the statement"
    template_program.specs[layout] = specs
    template_program.structural[layout] = structural_constants(decode(np.asarray(code, dtype=np.uint32)), consts, consts2)
    return np.asarray(code, dtype=np.uint32), len(consts), n_slots, len(specs), ncols


template_program.specs = {}                         # layout -> the table specs of its last template (generate reads the tables' kinds)
template_program.structural = {}                    # layout -> its structural small constants (structural_constants)
FIELD_P = 2**251 + 17 * 2**192 + 1
SMALL_MULTIPLE_MAX = 256                            # |c| up to which a structural constant is a candidate for shifts and adds


def felt_of(words):
    """4 x u64 little endian -> integer"""
    return sum(int(w) << (64 * k) for k, w in enumerate(words))


def structural_constants(ins, consts, consts2):
    """The compiled kernel is chosen by the hash of the code words; the constant table arrives at run time.  A constant may be baked
    into the code (a multiplication by it written as shifts and adds) only if it is the layout's, not the proof's: the SAME value in
    two dumps that differ in challenges, composition coefficient and statement, a small integer c (2 <= |c| <= SMALL_MULTIPLE_MAX), and
    a multiplier somewhere ("MUL acc, c" or "MOV acc, c; MUL acc, x": a boundary value that happens to be small is subtracted, not
    multiplied by).  -> {constant index: (c, Montgomery image as an integer)}.  The launch still compares every baked constant with
    the table it is given (QGenKernel::baked) and interprets the program on a mismatch: a wrong guess here costs time, not the result."""
    consts, consts2 = [felt_of(c) for c in consts], [felt_of(c) for c in consts2]
    rinv = pow(1 << 256, -1, FIELD_P)
    mul_use = set()
    for pc, (op, d, kind, w1) in enumerate(ins):
        if op <= OP_MUL and kind == SRC_CONST:
            nxt = ins[pc + 1] if pc + 1 < len(ins) else None
            if op == OP_MUL or (op == OP_MOV and nxt is not None and nxt[0] == OP_MUL and nxt[1] == d and not (nxt[2] == SRC_ACC and (nxt[3] & 3) == d)):
                mul_use.add(w1)
    out = {}
    for k in sorted(mul_use):
        if consts[k] != consts2[k] or consts[k] >= FIELD_P:
            continue
        v = consts[k] * rinv % FIELD_P
        c = v if v <= SMALL_MULTIPLE_MAX else v - FIELD_P if FIELD_P - v <= SMALL_MULTIPLE_MAX else None
        if c is not None and abs(c) >= 2:
            out[k] = (c, consts[k])
    return out


PRODUCT_COST = 185      # vector instructions of fl_mul_r280 (profiles/r04_quotient_algebra.txt)
WIDE_TERM_COST = 162    # a term of a wide sum: 81 multiply-adds at half rate
REDUCE_COST = 54        # fl_weak_reduce


def scale_plan(c, b):
    """|c| x (a lazy value of bound b) by fl_scale<f> steps with f x bound <= MAX_BOUND, a weak reduction wherever the next factor
    would pass it: c's factors <= MAX_BOUND, largest first (10 = 5 x 2, 16 = 8 x 2, 256 = 8 x 8 x 4; 11 has no such plan).
    -> (steps: "R" or a factor, cost in vector instructions, bound of the result) or None"""
    c = abs(c)
    factors = []
    while c > 1:
        f = next((f for f in range(min(c, MAX_BOUND), 1, -1) if c % f == 0), None)
        if f is None:
            return None
        factors.append(f)
        c //= f
    steps, cost = [], 0
    for f in factors:
        if b * f > MAX_BOUND:
            steps.append("R")
            cost += REDUCE_COST
            b = 1
        steps.append(f)
        b *= f
        # a limb of f x: one shift (power of two), else a shift-and-add per further set bit and a shift per trailing zero
        cost += 9 * (1 if f & (f - 1) == 0 else bin(f).count("1") - 1 + (1 if f % 2 == 0 else 0))
    return steps, cost, b


def decode(code):
    return [(int(code[2 * pc]) & 0xff, (int(code[2 * pc]) >> 8) & 0xf, (int(code[2 * pc]) >> 12) & 0xf, int(code[2 * pc + 1])) for pc in range(len(code) // 2)]


def split_program(ins, parts, inner_split=False):
    """Cut the program into `parts` programs whose outputs SUM to the program's output (several kernels by
    constraint group, each small enough in registers for two workgroups per CU and in code for the instruction cache).

    The composition is a sum of terms "group of constraints times the inverse of their zerofier" (42 for starknet, hardly a
    value shared between two of them).  The instruction stream is executed symbolically into a value graph, the output's
    top-level additions are flattened into those terms, the terms are dealt into `parts` runs of consecutive terms with
    balanced multiplication counts, and part j keeps - in the original order, with the original accumulators, slots,
    constants and tables - exactly the instructions its terms depend on; a top-level addition one of whose sides has no
    term in the part degenerates into a move or disappears.  -> [instruction list] (each ends in OUT)."""
    nodes = []                                     # (kind, a, b): kind in LEAF / ADD / SUB / MUL / INV
    def new(kind, a=None, b=None):
        nodes.append((kind, a, b))
        return len(nodes) - 1
    acc, slot, produced, root = [None] * 4, {}, [None] * len(ins), None
    for pc, (op, d, kind, w1) in enumerate(ins):
        if op <= OP_MUL:
            src = acc[w1 & 3] if kind == SRC_ACC else slot[w1] if kind == SRC_SLOT else new("LEAF")
        if op == OP_MOV:
            acc[d] = src
        elif op in (OP_ADD, OP_SUB, OP_MUL):
            acc[d] = new({OP_ADD: "ADD", OP_SUB: "SUB", OP_MUL: "MUL"}[op], acc[d], src)
        elif op == OP_RSUB:
            acc[d] = new("SUB", src, acc[d])
        elif op == OP_INV:
            acc[d] = new("INV", acc[d])
        elif op == OP_ST:
            slot[w1] = acc[d]
        else:
            root = acc[d]
        produced[pc] = acc[d] if op != OP_ST else slot[w1]
    assert root is not None and ins[-1][0] == OP_OUT
    uses = {}
    for kind, a, b in nodes:
        for x in (a, b):
            if x is not None:
                uses[x] = uses.get(x, 0) + 1
    terms, inner, scale = [], set(), set()
    stack = [root]
    while stack:                                   # the flattened top-level sum: inner additions, leaves = the terms
        v = stack.pop()
        kind, a, b = nodes[v]
        if kind == "ADD" and (v == root or uses.get(v, 0) == 1):
            inner.add(v)
            stack += [a, b]
        elif inner_split and kind == "MUL" and uses.get(v, 0) == 1 and nodes[b][0] == "LEAF" and nodes[a][0] in ("ADD", "MUL"):
            # "sum of constraints x inverse zerofier" / "constraint x alpha^k": a scaling by a table or constant distributes over
            # the sum below it, so the split may cut INSIDE a group (each side then pays the scaling once)
            scale.add(v)
            stack.append(a)
        else:
            terms.append(v)
    terms.sort()                                   # value numbers grow with the program counter
    def cone(v, seen):
        st = [v]
        while st:
            x = st.pop()
            if x in seen:
                continue
            seen.add(x)
            st += [y for y in nodes[x][1:] if y is not None]
        return seen
    weight = [sum(1 for x in cone(t, set()) if nodes[x][0] == "MUL") + 1 for t in terms]
    total, cuts, run = sum(weight), [], 0
    for k, wgt in enumerate(weight):               # consecutive runs of ~ total / parts multiplications
        run += wgt
        if len(cuts) < parts - 1 and run >= total * (len(cuts) + 1) / parts:
            cuts.append(k + 1)
    bounds = [0] + cuts + [len(terms)]
    out = []
    for j in range(parts):
        mine = terms[bounds[j]:bounds[j + 1]]
        assert mine, "more parts than terms"
        need = set()
        for t in mine:
            cone(t, need)
        # which inner sums are non-empty in this part
        full = set(mine)
        def nonempty(v):
            if v in full:
                return True
            if v in scale:
                r = nonempty(nodes[v][1])
                if r:
                    full.add(v)
                return r
            if v not in inner:
                return False
            _, a, b = nodes[v]
            r = nonempty(a) | nonempty(b)          # no short circuit: memoise both
            if r:
                full.add(v)
            return r
        nonempty(root)
        acc, slot, part = [None] * 4, {}, []
        for pc, (op, d, kind, w1) in enumerate(ins):   # replay: same symbolic values, filtered emission
            if op <= OP_MUL:
                src = acc[w1 & 3] if kind == SRC_ACC else slot[w1] if kind == SRC_SLOT else None
            v = produced[pc]
            if op == OP_MOV:
                val = src if kind in (SRC_ACC, SRC_SLOT) else v
                if (val in need or val in full) if kind in (SRC_ACC, SRC_SLOT) else (v in need):
                    part.append(ins[pc])
                acc[d] = v
            elif op == OP_ST:
                if v in need or v in full:
                    part.append(ins[pc])
                slot[w1] = v
            elif op == OP_OUT:
                part.append(ins[pc])
            elif v in scale:                       # the scaling of a (partial) sum: only where something is summed
                if nodes[v][1] in full:
                    part.append(ins[pc])
                acc[d] = v
            elif v in inner:                       # a top-level addition: d = d + src
                a_, b_ = nodes[v][1], nodes[v][2]
                ea, eb = a_ in full, b_ in full
                if ea and eb:
                    part.append(ins[pc])
                elif eb:                           # nothing of this part on the accumulator's side yet: the sum starts here
                    part.append((OP_MOV, d, kind, w1))
                acc[d] = v
            else:
                if v in need:
                    part.append(ins[pc])
                acc[d] = v
        out.append(part)
    return out, [weight[bounds[j]:bounds[j + 1]] for j in range(parts)]


def compact_slots(ins):
    """rename the scratch slots of a (part) program so that values with disjoint lifetimes share a slot: -> (program, slots).
    A slot's value lives from its ST to its last read before the next ST of the same slot."""
    lives, open_ = [], {}                          # [first pc, last pc, [pcs that name it]]
    for pc, (op, d, kind, w1) in enumerate(ins):
        if op <= OP_MUL and kind == SRC_SLOT:
            iv = open_[w1]
            iv[1] = pc
            iv[2].append(pc)
        elif op == OP_ST:
            open_[w1] = [pc, pc, [pc]]
            lives.append(open_[w1])
    out, free_at, n = list(ins), [], 0             # free_at[c] = pc after which colour c is free
    for first, last, pcs in sorted(lives, key=lambda iv: iv[0]):
        c = next((c for c in range(n) if free_at[c] < first), None)
        if c is None:
            c = n
            n += 1
            free_at.append(0)
        free_at[c] = last
        for pc in pcs:
            op, d, kind, _ = out[pc]
            out[pc] = (op, d, kind, c)
    return out, n


TEMP_ACC = 4            # a fifth accumulator the generator may use (the program format has four)
SRC_DERIVED = 6         # an operand kind of the generator's own (the program format has six): a cell of a DERIVED COLUMN,
                        # w1 = (derived column << 24) | row offset - see derived_column_of
SRC_TALPHA = 7          # another one: a cell of an ALPHA COPY of a multiplier-only periodic table - the table times one constraint's
                        # coefficient (fold_alpha_tables); w1 = (table << 16) | constant
MAX_DERIVED = 2         # derived columns per layout (each costs the launch one column of scratch and one streaming pass)
# ... and the loads a column has to save per point to be given that pass and that memory.  Measured (2^25 points,
# profiles/quotient_derived_flag_column.json): the flag column saves 100 loads per point and 4.0 ms of starknet's first part for a
# 0.37 ms pass and N felts of the context's scratch (1 GB there).  The recursive layout's other candidate (column 6, cell - 2 x (cell
# four rows on): 9 uses, 18 loads saved) measured 1.2 ms off its kernel for a second 0.38 ms pass - 0.8 ms net, 0.4 % of a proof -
# and a second gigabyte: below this floor it stays rematerialised.  The floor is that trade, set between the two; lower it to take it.
MIN_DERIVED_LOADS_SAVED = 32


def derived_column_of(recipe):
    """A recipe (rematerialize_cheap_slots) whose operands are cells of ONE trace column is a fixed integer combination of that
    column's rows: sum_t coefficient_t x column[row + offset_t].  Recipes that agree up to a common row shift read the same
    DERIVED COLUMN F[i] = sum_t coefficient_t x column[i + (offset_t - base) << log_blowup] at different rows - the 16 decoded flags
    of the CPU constraints, cell_j - 2 cell_(j+1), are F = column 0 - 2 x (column 0, one row on) at row offsets 0 .. 15.
    -> ((column, ((offset - base, coefficient), ...)), base), or None (a constant among the operands, two columns, all cancelled)"""
    coef = {}
    for op, _, kind, w1 in recipe:
        if kind != SRC_TRACE:
            return None
        if op == OP_MOV:
            coef = {}
        elif op == OP_RSUB:
            coef = {k: -c for k, c in coef.items()}
        coef[w1] = coef.get(w1, 0) + (-1 if op == OP_SUB else 1)
    terms = {w1 & 0xffffff: c for w1, c in coef.items() if c}
    if len(set(w1 >> 24 for w1 in coef)) != 1 or not terms:
        return None
    base = min(terms)
    return (next(iter(coef)) >> 24, tuple(sorted((off - base, c) for off, c in terms.items()))), base


def choose_derived_columns(found, max_columns=MAX_DERIVED, min_saved=None):
    """found: derived column -> [reads per point, loads saved per point] (rematerialize_cheap_slots over every part that
    rematerialises).  A column nobody reads twice, or that saves fewer than MIN_DERIVED_LOADS_SAVED loads, is not worth its pass; of the
    others the ones that save the most loads."""
    min_saved = MIN_DERIVED_LOADS_SAVED if min_saved is None else min_saved
    keep = sorted((-saved, key) for key, (reads, saved) in found.items() if reads >= 2 and saved >= min_saved)
    return [key for _, key in keep[:max_columns]]


def rematerialize_cheap_slots(ins, max_recipe=4, derived=(), found=None):
    """Scratch values that are a few additions of trace cells (the 16 decoded flags of the CPU constraints: cell - 2 x next cell)
    need not sit in a slot from their definition to their last use - 17 of them at once keep the starknet program's first part
    at one wave per SIMD (139 KB of LDS per 256 lanes).  Such a value is recomputed where it is read: its defining instructions
    (a MOV from a trace cell / constant followed by ADD / SUB / RSUB of cells or constants, at most `max_recipe` instructions) are
    replayed into a fifth accumulator in front of the reading instruction, and its store disappears.  -> program

    `derived`: the layout's derived columns (derived_column_of, choose_derived_columns).  A recipe that is a row of one of them is
    not recomputed at all: every read of it is ONE load of that column (operand kind SRC_DERIVED), and so is its definition where
    the defining instructions stand together (they and the store disappear).  The loaded value is a cell like any other: canonical,
    bound 1.  `found`, if given, collects per derived column the reads and the loads a point would save."""
    leafy = lambda kind: kind in (SRC_TRACE, SRC_CONST)
    recipe = [None] * 4                            # per accumulator: the instructions that made its value, if they qualify
    slot_recipe, out = {}, []
    for op, d, kind, w1 in ins:
        if op <= OP_MUL and kind == SRC_SLOT and w1 in slot_recipe:
            col = derived_column_of(slot_recipe[w1])
            if col is not None and found is not None:
                found.setdefault(col[0], [0, 0])
                found[col[0]][0] += 1
                found[col[0]][1] += len(slot_recipe[w1]) - 1
            if col is not None and col[0] in derived:
                out.append((op, d, SRC_DERIVED, (list(derived).index(col[0]) << 24) | col[1]))
                if d < 4:
                    recipe[d] = None
                continue
            for rop, _, rkind, rw1 in slot_recipe[w1]:
                out.append((rop, TEMP_ACC, rkind, rw1))
            out.append((op, d, SRC_ACC, TEMP_ACC))
            if d < 4:
                recipe[d] = None                   # (a MOV from such a slot is not itself a recipe: keep it simple)
            continue
        if op == OP_ST:
            if recipe[d] is not None and len(recipe[d]) <= max_recipe:
                slot_recipe[w1] = list(recipe[d])  # no store: every read below recomputes
                col = derived_column_of(recipe[d])
                if col is not None and out[-len(recipe[d]):] == recipe[d]:      # the definition itself: one load as well
                    if found is not None:
                        found.setdefault(col[0], [0, 0])[1] += len(recipe[d]) - 1
                    if col[0] in derived:
                        out[-len(recipe[d]):] = [(OP_MOV, d, SRC_DERIVED, (list(derived).index(col[0]) << 24) | col[1])]
                continue
            slot_recipe.pop(w1, None)
            out.append((op, d, kind, w1))
            continue
        if op == OP_MOV and leafy(kind):
            recipe[d] = [(op, d, kind, w1)]
        elif op in (OP_ADD, OP_SUB, OP_RSUB) and leafy(kind) and recipe[d] is not None:
            recipe[d] = recipe[d] + [(op, d, kind, w1)]
        elif op != OP_OUT:
            recipe[d] = None
        out.append((op, d, kind, w1))
    return out


def encode(ins):
    import numpy as np
    code = np.zeros(2 * len(ins), dtype=np.uint32)
    for pc, (op, d, kind, w1) in enumerate(ins):
        code[2 * pc], code[2 * pc + 1] = op | (d << 8) | (kind << 12), w1
    return code


def fold_alpha_tables(ins, scaled_tables, report=None):
    """A zerofier group is  (sum_k alpha^k C_k) x T  added to the part's total: a ten-step reduction of the group's sum and a full
    product by the domain's multiplier table T at every point.  Where T is a multiplier-only periodic table (`scaled_tables`: at most
    2^17 entries whatever the trace length) the launch can make one copy of it per constraint, T'_k = alpha^k T (times 2^24 and a sign,
    as the constant forms do), and since (sum_k alpha^k C_k) T = sum_k C_k (alpha^k T) every constraint is then one term of the part's
    total: the group's reduction and product are gone.  This pass rewrites the instruction stream accordingly:

        [C_0 in g]; MUL g, alpha^k0;  [C_1 in e]; MUL e, alpha^k1; ADD g, e;  ...;  MUL g, TABLE t;  ADD tot, g     becomes
        [C_0 in g]; MUL g, T'(t, k0); ADD tot, g;  [C_1 in e]; MUL e, T'(t, k1); ADD tot, e;  ...

    with operands of the generator's own kind SRC_TALPHA ("MOV tot, g" at the tail - the part's first group - makes the first
    constraint's addition the move).  Taken only where the stream has exactly that shape: the group's sum is used by the table
    product alone, every term of it is a product by a constant used once, the additions go into g, and nothing between the group's
    first coefficient and its tail touches `tot`.  Groups with a further factor (X - g^e) behind the table, and the full-length
    inverse tables of the single-row domains, do not match and stay as they are.
    -> (program, groups folded, constraints folded, the new program's pcs of each folded group's last addition into the total)"""
    nodes, made_at, lhs = [], {}, {}

    def new(kind, a=None, b=None):
        nodes.append((kind, a, b))
        return len(nodes) - 1
    acc, slot = [None] * 8, {}
    for pc, (op, d, kind, w1) in enumerate(ins):
        src = None
        if op <= OP_MUL:
            src = acc[w1 & 7] if kind == SRC_ACC else slot.get(w1) if kind == SRC_SLOT else new("LEAF")
        if op == OP_MOV:
            acc[d] = src
        elif op in (OP_ADD, OP_SUB, OP_MUL):
            lhs[pc] = acc[d]
            acc[d] = new({OP_ADD: "ADD", OP_SUB: "SUB", OP_MUL: "MUL"}[op], acc[d], src)
            made_at[acc[d]] = pc
        elif op == OP_RSUB:
            acc[d] = new("SUB", src, acc[d])
            made_at[acc[d]] = pc
        elif op == OP_INV:
            acc[d] = new("INV", acc[d])
        elif op == OP_ST:
            slot[w1] = acc[d]
        elif op == OP_OUT:
            new("OUT", acc[d])
    uses = {}
    for kind, a, b in nodes:
        for x in (a, b):
            if x is not None:
                uses[x] = uses.get(x, 0) + 1
    node_at = {k: v for v, k in made_at.items()}
    drop, replace, after, group_last = set(), {}, {}, []
    groups = constraints = seen_groups = 0
    for pc in range(len(ins) - 1):
        op, g, kind, t = ins[pc]
        op2, tot, kind2, w2 = ins[pc + 1]
        if not (op == OP_MUL and kind == SRC_TABLE and t in scaled_tables):
            continue
        why = None
        if not (op2 in (OP_ADD, OP_MOV) and kind2 == SRC_ACC and (w2 & 7) == g and tot != g):
            why = "the product is not added to a total"
        elif uses.get(node_at[pc], 0) != 1:
            why = "the product is used again"
        terms, inner, stack = [], [], [lhs[pc]]
        while why is None and stack:
            v = stack.pop()
            if v is None:
                why = "an empty operand"
            elif nodes[v][0] == "ADD" and uses.get(v, 0) == 1:
                inner.append(v)
                stack += [nodes[v][1], nodes[v][2]]
            else:
                terms.append(v)
        if why is None:
            for v in terms:
                k = made_at.get(v)
                if nodes[v][0] != "MUL" or uses.get(v, 0) != 1 or k is None or ins[k][0] != OP_MUL or ins[k][2] != SRC_CONST or k in replace:
                    why = "a term that is not a product by a constant used once"
                    break
        if why is None:
            term_pcs = sorted(made_at[v] for v in terms)
            adds = sorted(made_at[v] for v in inner)
            # the first constraint is computed in g itself, every other one in an accumulator that is then added to g
            if ins[term_pcs[0]][1] != g or len(adds) != len(term_pcs) - 1:
                why = "the sum does not start in the group's accumulator"
            for k, a_pc in zip(term_pcs[1:], adds):
                e = ins[k][1]
                if ins[a_pc] != (OP_ADD, g, SRC_ACC, e) or e in (g, tot) or not k < a_pc:
                    why = "an addition of another shape"
            for q in range(term_pcs[0], pc):
                qop, qd, qkind, qw1 = ins[q]
                if qd == tot or (qop <= OP_MUL and qkind == SRC_ACC and (qw1 & 7) == tot):
                    why = "the total's accumulator is used inside the group"
                    break
        if why is None and "QG_ALPHA_SKIP" in os.environ and str(seen_groups) in os.environ["QG_ALPHA_SKIP"].split(","):
            why = "skipped by QG_ALPHA_SKIP"
        seen_groups += 1 if (why is None or why.startswith("skipped")) else 0
        if why is not None:
            if report is not None:
                report.append("table %d at pc %d stays a product: %s" % (t, pc, why))
            continue
        for n_, k in enumerate(term_pcs):
            e, c = ins[k][1], ins[k][3]
            assert t < (1 << 15) and c < (1 << 16)
            replace[k] = (OP_MUL, e, SRC_TALPHA, (t << 16) | c)
            after[k] = (OP_MOV if op2 == OP_MOV and n_ == 0 else OP_ADD, tot, SRC_ACC, e)
        drop.update(adds)
        drop.update((pc, pc + 1))
        group_last.append(term_pcs[-1])
        groups += 1
        constraints += len(term_pcs)
    out, ends, last_of_group = [], set(), set(group_last)
    for pc, instr in enumerate(ins):
        if pc in drop:
            continue
        out.append(replace.get(pc, instr))
        if pc in after:
            out.append(after[pc])
            if pc in last_of_group:
                ends.add(len(out) - 1)
    return out, groups, constraints, ends


PREFETCH_DEPTH = 6      # memory operands in flight ahead of their use (one wave per SIMD: nothing else hides the latency)
LAZY_PRODUCT_MAX = int(os.environ.get("QG_LAZY_PRODUCT", "0"))   # bound(a) x bound(b) a plain product takes without reducing a factor first
DOT_MAX_TERMS = 16      # products accumulated in the 64-bit columns before a Montgomery reduction (16 * 9 * 2^56 < 2^64)
# Fusing "MUL acc, alpha^k ; ADD sum, acc" chains into dot products (one Montgomery reduction per DOT_MAX_TERMS units of bound)
# removes ~9 % of the vector instructions.  Left to itself the machine scheduler interleaves several program instructions
# and the 19 x 64-bit column accumulator then costs ~150 registers (scratch spills, 2.7x slower: round-2 v2); with a
# scheduling fence after every program instruction it costs its own 38 and the starknet kernel gains 9 % (154 -> 140 ms).
# The recursive kernel lives on two workgroups per CU (256 registers) and has no room for the accumulator: unfused.


# Kernel variants built side by side (ss_eval_quotient takes variant 0; SS_QG_VARIANT=k selects another for A/B runs, built by
# `make QG_AB=1`).  A variant = (name suffix, inner split, [one configuration per PART]); a part's configuration =
#   (operand prefetch depth, slots in registers instead of LDS, workgroups per CU the register budget is set for, scheduling
#    fence after every program instruction, "MUL alpha^k; ADD" chains as fused dot products, lanes per workgroup)
# Round 2, one kernel per layout, measured on the MI355X (profiles/r02_quotient_codegen_experiments.txt; 2^25 points): the
# starknet program is register bound - LDS slots, one workgroup per CU, a shallow prefetch (unfused, depth 3: 153.7 ms, 2:
# 154.3, 1: 159.6, 4: 153.7, 6: 171.5; slots in registers at two workgroups per CU: 352, scratch spills; fenced + fused, depth
# 3: 140.2, 2: 140.6, 4: 167.8, slots in registers: 161.6); the recursive one fits two workgroups per CU with its slots in
# registers (depth 4: 65.5 ms, 6: 66.0, 2: 65.1; LDS slots at one workgroup per CU: 76.9; fenced + fused at one workgroup per
# CU: 86).  Round 3: the program cut into parts that each fit two workgroups per CU - split_program above.
ONE_WG = (3, False, 1, True, True, 256)            # round 2's starknet kernel: 17 LDS slots, fused dot products, one wave per SIMD
TWO_WG = (3, False, 2, True, False, 256)           # <= 7 LDS slots + constants in 80 KB, 256 registers: two waves per SIMD
TWO_WG_FUSED = (3, False, 2, True, True, 256)
TWO_WG_REGS = (4, True, 2, False, False, 256)      # round 2's recursive kernel: slots in registers
BIG_WG = (3, False, 1, True, False, 512)           # ONE 512-lane workgroup per CU: two waves per SIMD behind one barrier, constants shared
BIG_WG_FUSED = (3, False, 1, True, True, 512)
sync = lambda cfg, every=8: cfg + (every,)         # + a workgroup barrier every `every` program instructions
depth = lambda cfg, d: (d,) + cfg[1:]
# Round 3, MI355X, 2^25 points (profiles/r03_quotient_parts_ab.txt).  starknet: round 2's kernel 140.3 ms (with barriers 147.8);
# cut into 6 at two workgroups per CU 131.7 (+ barriers every 8 instructions 136.1, every 32: 133.3; + fused dot products
# 130.2; 4 parts 136.7, 8 parts 136.0; cuts between zerofier groups only, 3 parts: 134.1); the five light parts as ONE
# 512-lane workgroup per CU: 133.4 without barriers, 128.9 with (every 16: 127.2, every 4: 132.1; prefetch depth 2 / 4: 129.5 /
# 129.3; 8 parts 130.1), with fused dot products 122.1 (barriers every 16: 120.3; part 0 without: 120.9; 5 / 7 / 8 parts: 126.5 /
# 121.3 / 123.3; prefetch depth 2 / 4: 122.5 / 122.8).  recursive: round 2's kernel 63.1 ms stays the best (3 - 4 parts: 63.3 - 68.6).
# Then the 16 decoded flags (cell - 2 x next cell) recomputed at their uses instead of parked in scratch slots (17 -> 6 slots: the
# first part fits a 512-lane workgroup as well): starknet 120.8 -> 117.5 ms (7 parts: 117.5, 5 parts: 121.7); recursive as ONE
# 512-lane workgroup with fused dot products 63.7 -> 60.1 ms (round 2's shape with the flags recomputed: 67.5).
# (suffix, cuts inside zerofier groups, [part configurations], recompute cheap scratch values at their uses)
VARIANTS = {
    "starknet": [("", True, [sync(BIG_WG_FUSED, 16)] * 6, True)],      # (round 2's one kernel and round 3's 17-slot first part no longer fit the LDS beside today's constants)
    "recursive": [("", False, [sync(BIG_WG_FUSED, 16)], True),
                  # round 6 A/B (profiles/r06_call_j_recursive_quotient_parts.txt): the program cut into 2 / 3 parts has the same 229
                  # multiplications and runs 55.3 / 54.0 ms against the one part's 53.9 - 143 G products/s of the multiplier's 157
                  ("_v2", True, [sync(BIG_WG_FUSED, 16)] * 2, True),
                  ("_v3", True, [sync(BIG_WG_FUSED, 16)] * 3, True)],
}
LDS_BYTES_PER_CU = 160 * 1024
REMAT_ABOVE_SLOTS = 8


def generate(layout, all_variants=False):
    """variant 0 is what the library builds; --all-variants also writes the others (`make QG_AB=1` builds them, SS_QG_VARIANT=k
    selects one at run time).  -> [(variant, suffix, [part source names])]"""
    code, n_consts, n_slots, n_tables, ncols = template_program(layout)
    ins = decode(code)
    written = []
    for k, (suffix, inner, cfgs, remat) in enumerate(VARIANTS[layout] if all_variants else VARIANTS[layout][:1]):
        parts, weights = split_program(ins, len(cfgs), inner) if len(cfgs) > 1 else ([ins], None)
        # tables that are only ever MULTIPLIERS (zerofier inverses and their kin; not the periodic columns, which are also added and
        # subtracted): the launch makes a copy of them times 2^24 (csrc/capi.hip eval_quotient_compiled, QGenKernel::scaled), so that
        # "sum x table" is a product with the ten-step reduction - 185 instead of 223 instructions, 46 / 23 of them per point
        scaled = []
        if SCALED_TABLES and k == 0:
            uses = {}
            for op, d, kind, w1 in ins:
                if op <= OP_MUL and kind == SRC_TABLE:
                    uses.setdefault(w1, set()).add(op)
            # ... but not the DOMAIN-sized ones (kind "inverse": the per-point inverses of the single-point zerofiers, 2 n entries
            # each): their copies were five 2^27-entry tables at 2^22 steps - what broke the two-rank proof of that size in round 4
            # (VERDICT r4 #4).  What is copied is periodic: at most 2^17 entries per table, a few megabytes per launch in all.
            full_length = {t for t, spec in enumerate(template_program.specs[layout]) if spec[0] == "inverse"}
            scaled = sorted(t for t, ops in uses.items() if ops == {OP_MUL} and t not in full_length)
        names, baked = [], set()
        alpha = []                                  # the layout's alpha copies, in the order the bodies number them: (table, constant, form)
        # the parts that rematerialise (the decoded flags: recomputed at their uses instead of parked, 17 -> 6 slots) - and what of
        # that is a row of a derived column, read instead of recomputed (one list per layout: the launch builds the columns once)
        compacted = [compact_slots(part) for part in parts]
        remat_here = [remat and part_slots > REMAT_ABOVE_SLOTS for _, part_slots in compacted]
        derived = []
        if DERIVED_COLUMNS:
            found = {}
            for (part, _), here in zip(compacted, remat_here):
                if here:
                    rematerialize_cheap_slots(part, found=found)
            derived = choose_derived_columns(found)
        for j, ((part, part_slots), cfg) in enumerate(zip(compacted, cfgs)):
            depth, slots_in_regs, wgs, fence, fuse, threads = cfg[:6]
            sync = int(os.environ.get("QG_SYNC", cfg[6] if len(cfg) > 6 else 0))
            if remat_here[j]:
                part, part_slots = compact_slots(rematerialize_cheap_slots(part, derived=derived))
            if not slots_in_regs:
                lds = part_slots * 2 * threads * 16 + n_consts * 36 * 4
                assert lds * wgs <= LDS_BYTES_PER_CU, "%s%s part %d: %d slots + constants = %d B of LDS x %d workgroups per CU" % (layout, suffix, j, part_slots, lds, wgs)
            base = "quotient_gen_%s%s_p%d" % (layout, suffix, j)
            wide_here, depth_here, lazy_sub, const_factor, min_terms, small_here, dedup_here, alpha_here = (
                PART_TUNING.get(layout, {}).get((suffix, j), (False, depth, False, False, 1, False, False, False)) + (False,))[:8]
            if "QG_ALPHA_TABLES" in os.environ:               # A/B builds: "all", "0", or "starknet:1,starknet:3,..."
                alpha_here = os.environ["QG_ALPHA_TABLES"] == "all" or ("%s:%d" % (layout, j)) in os.environ["QG_ALPHA_TABLES"].split(",")
            alpha_flush = os.environ.get("QG_ALPHA_FLUSH", alpha_here if isinstance(alpha_here, str) else "never")
            alpha_here = bool(alpha_here) and fuse and bool(scaled)
            group_ends = set()
            if alpha_here:
                report = []
                part, n_groups, n_folded, group_ends = fold_alpha_tables(part, set(scaled), report)
                print("%s part %d: %d groups (%d constraints) take their coefficients from alpha copies of their tables" % (layout, j, n_groups, n_folded))
                if os.environ.get("QG_VERBOSE"):
                    print("".join("   %s\n" % line for line in report), end="")
            small_here =os.environ["QG_SMALL_MULTIPLES"] != "0" if "QG_SMALL_MULTIPLES" in os.environ else small_here      # A/B builds: every part alike
            dedup_here = os.environ["QG_DEDUP"] != "0" if "QG_DEDUP" in os.environ else dedup_here
            min_terms = int(os.environ.get("QG_WIDE_MIN_TERMS", min_terms))
            if "QG_WIDE_PARTS" in os.environ:                 # A/B builds (tools/qg_wide_ab.sh): the same choice for every part
                wide_here = ("%s:%d" % (layout, j)) in os.environ["QG_WIDE_PARTS"].split(",") or os.environ["QG_WIDE_PARTS"] == "all"
            depth_here = int(os.environ.get("QG_DEPTH", depth_here))
            lazy_sub = os.environ["QG_SUB_LAZY2"] != "0" if "QG_SUB_LAZY2" in os.environ else lazy_sub
            const_factor = os.environ["QG_CONST_FACTOR"] != "0" if "QG_CONST_FACTOR" in os.environ else const_factor
            body = generate_body(layout, part, n_consts, part_slots, n_tables, ncols, depth_here, base + ".inc", fuse,
                                 "QG_OUT" if j == 0 else "QG_OUT_ACC", sync, wide_here, lazy_sub, const_factor, min_terms, scaled, derived=derived,
                                 small=template_program.structural[layout] if small_here else {}, dedup=dedup_here,
                                 alpha=alpha if alpha_here else None, group_ends=group_ends if alpha_flush == "group" else ())
            baked.update(body["baked"])
            write_part(layout, suffix, j, len(parts), base, body, len(part), n_consts, part_slots, slots_in_regs, wgs, fence, threads, sync)
            names.append(base + ".hip")
        write_kernel_table(layout, suffix, k, code, n_consts, n_tables, ncols, len(parts), scaled, derived,
                           [(c, template_program.structural[layout][c][1]) for c in sorted(baked)], alpha)
        if k == 0:
            report_alpha_scratch(layout, alpha)
        names.append("quotient_gen_%s%s.hip" % (layout, suffix))
        written.append((k, suffix, names))
    return written



ALPHA_PIN = os.environ.get("QG_ALPHA_PIN", "1") != "0"         # QG_PIN_WIDE behind the terms by alpha copies (A/B: QG_ALPHA_PIN=0)
ALPHA_FORMS = ("R280", "R280_UP", "R280_UPN")       # an alpha copy is its table times the constant in one of the constant forms of quotient_gen.h


def report_alpha_scratch(layout, alpha):
    """what the alpha copies add to the launch's scratch: 32 bytes per entry of every copy - the periods times the blow-up, whatever the
    trace length (printed at blow-up 2; it doubles with the blow-up as the scaled tables do)"""
    import importlib
    lay = importlib.import_module("sandstorm_amd.layouts." + layout)
    tables = lay.Tables(1 << (21 if layout == "starknet" else 18))         # the template's size: its specs name powers of X by n / period
    specs = template_program.specs[layout]
    entries = 0
    for t, _, _ in alpha:
        assert specs[t][0] != "inverse"
        entries += tables.length(specs[t])
    print("%s: %d alpha copies of %d tables, %d entries = %d bytes of scratch per launch at blow-up 2"
          % (layout, len(alpha), len(set(t for t, _, _ in alpha)), entries, 32 * entries))
    return entries


WIDE_MAX_OTHER_PRODUCTS = int(os.environ.get("QG_WIDE_OTHER", "0"))     # other multiplications allowed while a constraint's wide sum is open
WIDE_ANY_CONST_MUL = os.environ.get("QG_WIDE_ANY_CONST", "1") != "0"   # constraints whose alpha power is not a fused dot term close at their constant too
SCALED_TABLES = os.environ.get("QG_SCALED_TABLES", "1") != "0"         # multiplier-only tables from a 2^24-fold copy (r280 products)
DERIVED_COLUMNS = os.environ.get("QG_DERIVED", "1") != "0"             # recipes over one trace column read from a derived column (A/B: QG_DERIVED=0)
WIDE_MAX_SPAN = int(os.environ.get("QG_WIDE_SPAN", "1000"))            # program instructions from its first product to its alpha multiplication
# the parts (variant suffix, part number) whose constraints' top-level products accumulate in a second wide accumulator (see
# plan_wide_constraints); QG_WIDE_PARTS="starknet:1,starknet:3,..." overrides for A/B builds
# Chosen per part on the MI355X (profiles/r04_quotient_algebra.txt: every part is its own kernel, 16 builds timed part by part):
# (variant suffix, part) -> (wide sums, operand prefetch depth, lazy subtrahends, constants as factors, products a constraint needs
# to get a wide sum of its own).  The instruction counts fall everywhere; the time
# follows only where the register allocator keeps its spills (a second 38-register accumulator beside the dot product's) - part 4
# of starknet is faster as it was, with a shallower prefetch.
# With the decoded flags read from a derived column (rematerialize_cheap_slots: starknet part 0 and the recursive kernel lose nearly
# half their operand loads) those two were rebuilt at depth 2 / 3 / 4 (profiles/quotient_derived_flag_column.json): starknet part 0
# 18.78 / 18.82 / 18.94 ms (2 and 3 within the launches' own scatter: 3 stays), recursive 50.13 / 50.75 / 51.03 ms (2 stays).
# Two further switches per part (profiles/quotient_small_multiples.json): SMALL MULTIPLES - a multiplication by a structural small
# integer (structural_constants: 2, 4, 6, 8, 10, 16, -2, -4 in the Poseidon rounds, the bit unpackings, the bitwise builtin) as
# fl_scale shifts and adds where scale_plan prices it below the product - and REPEATED OPERANDS - two consecutive memory operands
# that name the same cell ("x + x" lowers to MOV acc, T; ADD acc, T) as one load.
# A part whose scratch (spill) bytes grow under a cut keeps that cut off - the condition the cuts were taken under, checked on the
# cross-compiled kernels: part 1 spills 76 -> 104 bytes per lane with its two small multiples (off), part 3 0 -> 272 with its 21
# repeated operands as single loads (off: the shared register lives across the fence between its two uses).
PART_TUNING = {"starknet": {("", 0): (True, 3, True, True, 1, True, True, True), ("", 1): (True, 2, True, True, 1, False, True, True),
                            ("", 2): (True, 3, False, False, 1, True, True, True), ("", 3): (True, 3, True, True, 2, True, False, True),
                            ("", 4): (True, 2, False, False, 2, True, True, True), ("", 5): (True, 3, True, True, 1, True, True, True)},
               "recursive": {("", 0): (True, 2, True, True, 1, True, True, "group"),
                             ("_v2", 0): (True, 2, True, True, 1, False, False), ("_v2", 1): (True, 2, True, True, 1, False, False),
                             ("_v3", 0): (True, 2, True, True, 1, False, False), ("_v3", 1): (True, 2, True, True, 1, False, False),
                             ("_v3", 2): (True, 2, True, True, 1, False, False)}}


class WideViolation(Exception):
    """the emission met a use of a half-summed constraint it cannot express: that constraint goes back to plain products"""
    def __init__(self, k, why):
        Exception.__init__(self, "constraint at pc %d: %s" % (k, why))
        self.k = k


def plan_wide_constraints(ins, fused, banned, const_factor=True, min_terms=1, scaled_tables=frozenset(), small=frozenset()):
    """Round 4.  A constraint C = sum_i s_i A_i B_i + L (A_i, B_i, L: sums of cells, constants and earlier values;
    most of the program's products sit at this top level) paid a whole Montgomery product per A_i B_i - 81 multiply-adds plus a
    142-instruction reduction - and, where a product waited for its siblings in a scratch slot, a weak reduction, a store and a
    load on top.  The products of ONE constraint can share one reduction: their 81 partial products each go into the 19 64-bit
    columns of a wide accumulator (fl252.h FlWide), L joins as L * 2^256 (its limbs shifted 4 bits into columns 9..17), and one
    ten-step reduction by 2^280 yields g C 2^-24 (g = +-1, chosen so that most products need no negation) - which the
    multiplication by the constraint's power of the composition coefficient, already a term of a fused dot product, takes back
    by using g alpha^k 2^24 as its constant (quotient_gen.h QG_CONST_R280_UP / _UPN).

    This function finds, in the value graph of the instruction stream, for every fused "MUL acc, alpha^k" (pc in `fused`) the
    flattened signed sum below the multiplied value and its product terms.  -> (wide_mul: pc of a product -> (constraint, sign),
    close: pc of the alpha multiplication -> (g, number of products), struct: pc of an ADD / SUB / RSUB inside the sum ->
    constraint).  A constraint is named by the pc of its alpha multiplication.

    `small`: the constants whose multiples are shifts and adds (structural_constants).  "MOV acc, c; MUL acc, x" with such a c is no
    product term: c x is a plain value, and where it stands in a constraint's sum it joins the linear part L."""
    nodes = []                                     # (kind, a, b)
    small_node, small_mul = set(), set()           # CONST nodes of `small`; pcs of the multiplications by them

    def new(kind, a=None, b=None):
        nodes.append((kind, a, b))
        return len(nodes) - 1
    acc, slot = [None] * 8, {}
    made_at, root_of = {}, {}                      # node -> pc of the instruction that made it; pc of an alpha MUL -> node multiplied
    by_scaled_table = set()
    for pc, (op, d, kind, w1) in enumerate(ins):
        src = None
        if op <= OP_MUL:
            src = acc[w1 & 7] if kind == SRC_ACC else slot[w1] if kind == SRC_SLOT else new("CONST" if kind == SRC_CONST else "LEAF")
            if kind == SRC_CONST and w1 in small:
                small_node.add(src)
        if op == OP_MOV:
            acc[d] = src
        elif op in (OP_ADD, OP_SUB):
            acc[d] = new("ADD" if op == OP_ADD else "SUB", acc[d], src)
            made_at[acc[d]] = pc
        elif op == OP_RSUB:
            acc[d] = new("SUB", src, acc[d])
            made_at[acc[d]] = pc
        elif op == OP_MUL:
            if pc in fused or (WIDE_ANY_CONST_MUL and kind in (SRC_CONST, SRC_TALPHA)):      # any scaling by a constant can take the 2^24 back (an alpha copy too)
                root_of[pc] = acc[d]
            if src in small_node or acc[d] in small_node:
                small_mul.add(pc)
            acc[d] = new("MUL", acc[d], src)
            made_at[acc[d]] = pc
            if kind == SRC_TABLE and w1 in scaled_tables:                       # (the table's copy carries 2^24: a plain r280 product)
                by_scaled_table.add(acc[d])
        elif op == OP_INV:
            acc[d] = new("INV", acc[d])
        elif op == OP_ST:
            slot[w1] = acc[d]
        elif op == OP_OUT:
            new("OUT", acc[d])
    uses = {}
    for kind, a, b in nodes:
        for x in (a, b):
            if x is not None:
                uses[x] = uses.get(x, 0) + 1
    wide_mul, close, struct = {}, {}, {}
    taken = set()
    for k in sorted(root_of):
        if k in banned:
            continue
        r = root_of[k]
        if r is None or uses.get(r, 0) != 1:
            continue
        terms, inner, stack = [], [], [(1, r)]
        while stack:
            sgn, v = stack.pop()
            kind, a, b = nodes[v]
            if kind in ("ADD", "SUB") and (v == r or uses.get(v, 0) == 1):
                inner.append(v)
                stack.append((sgn, a))
                stack.append((sgn if kind == "ADD" else -sgn, b))
            else:
                terms.append((sgn, v))
        prods = [(sgn, v) for sgn, v in terms
                 if nodes[v][0] == "MUL" and uses.get(v, 0) == 1 and nodes[v][1] != nodes[v][2] and v not in taken and v not in by_scaled_table
                 and nodes[nodes[v][2]][0] != "CONST" and (const_factor or nodes[nodes[v][1]][0] != "CONST") and made_at[v] not in root_of
                 and nodes[v][1] not in small_node]
        # (a constant that was MOVed into the accumulator and multiplied by a cell is a factor like any other: its R256 limbs are the
        # value c 2^256, so c x cell comes out at the same 2^-24 as the products of two cells - sums of 2^(16 j) x cell_j, fourteen terms
        # long in the range-check and bit-unpacking constraints, become fourteen 81-multiply-add terms and ONE reduction)
        if len(prods) < min_terms:
            continue
        # register pressure: the wide sum (38 registers) lives from the constraint's first product to the alpha multiplication,
        # beside the alpha dot product's own 38; a plain product in between adds its 36 columns on top (scratch spills: the
        # recursive kernel ran 14 % SLOWER with every constraint widened) - so only constraints whose products follow each other
        first = min(made_at[v] for _, v in prods)
        mine = set(made_at[v] for _, v in prods)
        between = [pc for pc in range(first, k) if ins[pc][0] in (OP_MUL, OP_INV) and pc not in mine and pc not in small_mul]     # (shifts and adds: no columns)
        if len(between) > WIDE_MAX_OTHER_PRODUCTS or k - first > WIDE_MAX_SPAN:
            continue
        g = 1 if sum(1 for sgn, _ in prods if sgn > 0) * 2 >= len(prods) else -1
        for sgn, v in prods:
            wide_mul[made_at[v]] = (k, sgn * g)
            taken.add(v)
        for v in inner:
            struct[made_at[v]] = k
        close[k] = (g, len(prods))
    return wide_mul, close, struct


def generate_body(layout, ins, n_consts, n_slots, n_tables, ncols, PREFETCH_DEPTH, inc_name, FUSE_ALPHA_DOT_PRODUCTS=False, out_macro="QG_OUT",
                  sync_every=0, wide_products=False, lazy_sub=False, const_factor=False, min_terms=1, scaled_tables=(), derived=(), small=None, dedup=False, alpha=None, group_ends=()):
    """the straight-line body of one (part) program -> csrc/<inc_name>.  `derived`: the derived columns SRC_DERIVED operands name
    (rematerialize_cheap_slots); the body reads them through QG_DERIVED_RAW and carries a fallback definition of that macro over
    the real column, for a harness that defines only the other operand macros and fills only the real columns.
    `small`: the structural small constants whose multiples may be written as shifts and adds (structural_constants; {} = none).
    `dedup`: two consecutive memory operands that name the same cell are one load.
    `alpha`: the layout's list of alpha copies (table, constant, form) if the program holds SRC_TALPHA operands (fold_alpha_tables): the
    body's copies are appended to it, and QG_TABLE_ALPHA_RAW(j, idx) reads copy j of that list."""
    small = small or {}
    n_instr = len(ins)
    # ---- memory operands in program order: loaded PREFETCH_DEPTH operands ahead into a rotating set of registers
    mem_ops = []                                    # (pc, macro text)
    for pc, (op, d, kind, w1) in enumerate(ins):
        if op <= OP_MUL and kind == SRC_TRACE:
            assert (w1 >> 24) < ncols
            mem_ops.append((pc, "QG_TRACE_RAW(%d, %du, %%s)" % (w1 >> 24, w1 & 0xffffff)))
        elif op <= OP_MUL and kind == SRC_DERIVED:
            assert (w1 >> 24) < len(derived)
            mem_ops.append((pc, "QG_DERIVED_RAW(%d, %du, %%s)" % (w1 >> 24, w1 & 0xffffff)))
        elif op <= OP_MUL and kind == SRC_TABLE:
            assert w1 < n_tables
            if w1 in scaled_tables:          # its 2^24-fold copy: descriptor n_tables + j of the launch's descriptor array
                assert op == OP_MUL
                mem_ops.append((pc, "QG_TABLE_SCALED_RAW(%d, %%s)" % (n_tables + list(scaled_tables).index(w1))))
            else:
                mem_ops.append((pc, "QG_TABLE_RAW(%d, %%s)" % w1))
        elif op == OP_MUL and kind == SRC_TALPHA:
            assert alpha is not None and (w1 >> 16) in scaled_tables and (w1 & 0xffff) < n_consts
            mem_ops.append((pc, ("alpha copy", w1 >> 16, w1 & 0xffff)))          # which form: known with the plan (below)
    # "x + x" on a cell is MOV acc, T; ADD acc, T: the second operand is the first one's register, which is freed (its next load
    # issued) after the second use.  Only CONSECUTIVE operands: a register kept across other loads is a live range the allocator pays
    # for (profiles/r06_call_q_quotient_conversions_ablated.txt)
    mem_index, merged, deduped = {}, [], []
    for pc, text in mem_ops:
        if dedup and merged and merged[-1][1] == text:
            deduped.append((pc, text % "i"))
        else:
            merged.append((pc, text))
        mem_index[pc] = len(merged) - 1
    mem_ops = merged
    D = min(PREFETCH_DEPTH, len(mem_ops))
    # ---- which "MUL acc, alpha^k ; ADD sum, acc" pairs become terms of a fused dot product: the product's accumulator
    #      must die with the ADD (its next use, if any, is a write)
    def dies_after(acc, pc):
        for op, d, kind, w1 in ins[pc + 1:]:
            reads = (op <= OP_MUL and kind == SRC_ACC and (w1 & 7) == acc) or (d == acc and op in (OP_ADD, OP_SUB, OP_RSUB, OP_MUL, OP_INV, OP_ST, OP_OUT))
            if reads:
                return False
            if d == acc and op == OP_MOV:
                return True
        return True
    fused = {}                                      # pc of the MUL -> accumulator the term is added to
    for pc in range(n_instr - 1):
        op, e, kind, w1 = ins[pc]
        op2, d2, kind2, w2 = ins[pc + 1]
        if FUSE_ALPHA_DOT_PRODUCTS and op == OP_MUL and kind in (SRC_CONST, SRC_TALPHA) and op2 == OP_ADD and kind2 == SRC_ACC and (w2 & 7) == e and d2 != e and dies_after(e, pc + 1):
            fused[pc] = d2
    banned = set()
    while True:                                     # constraints whose half-summed value is used in a way the emission cannot express
        try:                                        # go back to plain products, one at a time (plan_wide_constraints)
            plan = plan_wide_constraints(ins, fused, banned, const_factor, min_terms, set(scaled_tables), set(small)) if wide_products and FUSE_ALPHA_DOT_PRODUCTS else ({}, {}, {})
            # an alpha copy carries what the constant would: the plain R280 form, or - where the multiplication takes a constraint's own
            # wide sum back - the form with 2^24 more and the sum's sign.  Copies are numbered across the layout's parts, in order of use
            copies = list(alpha or ())
            ops = []
            for pc_, text in mem_ops:
                if isinstance(text, tuple):
                    key = (text[1], text[2], 0 if pc_ not in plan[1] else 1 if plan[1][pc_][0] > 0 else 2)
                    if key not in copies:
                        copies.append(key)
                    text = "QG_TABLE_ALPHA_RAW(%d, %%s)" % copies.index(key)
                ops.append((pc_, text))
            out, stats = _emit_body(ins, n_consts, n_slots, ops, mem_index, D, fused, out_macro, sync_every, lazy_sub, const_factor, set(scaled_tables),
                                    plan, small, flush_on_switch=alpha is not None, flush_after=set(group_ends))
            mem_ops = ops
            if alpha is not None:
                alpha[:] = copies
            break
        except WideViolation as e:
            banned.add(e.k)
            if os.environ.get("QG_VERBOSE"):
                print("   plain again:", e)
    stats["wide_banned"] = len(banned)
    body = "\n".join(out)
    regs = "    Fp " + ", ".join("m%d" % k for k in range(D)) + ";\n"
    prime = "".join("    m%d = %s;\n" % (j, mem_ops[j][1] % "i32") for j in range(D))
    used = sorted(set(w1 >> 24 for op, _, kind, w1 in ins if op <= OP_MUL and kind == SRC_DERIVED))
    import re
    used_alpha = sorted(set(int(j_) for _, text in mem_ops for j_ in re.findall(r"QG_TABLE_ALPHA_RAW\((\d+),", text)))
    stats["alpha_copies"] = len(used_alpha)
    inc = _INC_TEMPLATE % dict(layout=layout, regs=regs, prime=prime, body=body, depth=D,
                               derived_begin=_alpha_fallback(alpha, used_alpha, n_tables, list(scaled_tables)) + _derived_fallback(derived, used),
                               small_begin=_SMALL_FALLBACK_BEGIN if stats["baked"] else "", small_end=_SMALL_FALLBACK_END if stats["baked"] else "",
                               derived_end=(_DERIVED_FALLBACK_END % "".join("#undef QG_DERIVED_FALLBACK_%d\n" % k for k in used) if used else "")
                                           + (_ALPHA_FALLBACK_END % "".join("#undef QG_TABLE_ALPHA_FALLBACK_%d\n" % k for k in used_alpha) if used_alpha else ""),
                               wide=("    QgWide wd;\n" if stats["fused"] else "") + ("    QgWide wq;\n" if stats["wide_terms"] else ""),
                               temp_acc=", acc4 = fl_zero()" if any(d == TEMP_ACC for _, d, _, _ in ins) else "")
    name = inc_name
    with open(os.path.join(OUT_DIR, name), "w") as f:
        f.write(inc)
    print("%s: %d instructions, %d multiplications (%d by constants, %d fused into %d dot products, %d as terms of %d constraints' own wide sums - %d "
          "negated, %d constraints kept plain), %d loads %d ahead, %d reductions -> %s"
          % (layout, len(ins), stats["mul"], stats["mulr"], stats["fused"], stats["flushes"], stats["wide_terms"], stats["wide_closes"], stats["wide_neg"],
             stats["wide_banned"], stats["loads"], D, stats["reduce"], name))
    if small or dedup:
        print("   small multiples: %s" % (", ".join("%d x const %d (%d)" % (n, k, small[k][0]) for k, n in sorted(stats["baked"].items())) or "none"))
        print("   repeated operands: %s" % (", ".join("pc %d %s" % d_ for d_ in deduped) or "none"))
    return dict(stats, inc=name, depth=D)


_INC_TEMPLATE = '''// GENERATED by tools/gen_quotient.py - DO NOT EDIT.  The body of the `%(layout)s` constraint kernel: the program unrolled over the
// operand macros of quotient_gen.h (operand loads issued %(depth)d operands ahead).  Included by the quotient_gen_%(layout)s*.hip
// wrappers (device) and, with host definitions of the same macros, by tests/cpp/quotient_gen_host_test.cpp, which runs it on
// the CPU against the oracle's constraint VM.
%(small_begin)s%(derived_begin)s    Fl acc0 = fl_zero(), acc1 = fl_zero(), acc2 = fl_zero(), acc3 = fl_zero()%(temp_acc)s;
%(wide)s%(regs)s    uint32_t i32 = (uint32_t)(lane < N ? lane : N - 1);
%(prime)s    QG_POINT_LOOP_BEGIN
%(body)s
    QG_POINT_LOOP_END
%(derived_end)s%(small_end)s'''


# A multiple by constant k, whose value the generator knows to be the small integer c (structural_constants), is written as
# QG_SCALE(k, f, x) [; fl_weak_reduce; QG_RESCALE(f', .) ...] [; QG_NEGSCALED(C, F, .)] with f f' ... = |c| (scale_plan).  The device
# (quotient_gen.h) takes fl_scale<f>(x), fl_scale<f'>(.) and fl_sub_c<C, F>(0, .) - its launch has checked the constant table against
# QGenKernel::baked; an includer that does not define the macros (a harness that runs the body on constants of its own choosing) takes
# the product by the table's constant for the first and nothing for the others: the same value, within the same bounds.
_SMALL_FALLBACK_BEGIN = '''// QG_SCALE(k, f, x) [QG_RESCALE(f', .) ...] [QG_NEGSCALED(C, F, .)] is x times constant k, a structural small integer +-f f' ... of the
// layout (tools/gen_quotient.py structural_constants): on the device shifts and adds (quotient_gen.h; the launch first checks the constant
// table against the kernel table's list).  Where the includer does not define the macros the first is the product by the table's
// constant and the others do nothing - the same value mod p, normalised.
#ifndef QG_SCALE
#define QG_SCALE_FALLBACK
#define QG_SCALE(k, C, x) fl_mul_r280(x, QG_CONST_R280(k))
#define QG_RESCALE(C, x) x
#define QG_NEGSCALED(C, F, x) x
#endif
'''
_SMALL_FALLBACK_END = '''#ifdef QG_SCALE_FALLBACK
#undef QG_SCALE
#undef QG_RESCALE
#undef QG_NEGSCALED
#undef QG_SCALE_FALLBACK
#endif
'''


def _small_multiple(expr, k):
    """k x expr (k >= 1) with fp_dbl / fp_add"""
    if k == 1:
        return expr
    if k % 2 == 0:
        return "fp_dbl(%s)" % _small_multiple(expr, k // 2)
    return "fp_add(%s, %s)" % (_small_multiple(expr, k - 1), expr)


def _derived_fallback(derived, used):
    """QG_DERIVED_RAW where nobody defined it: a cell of derived column k computed from the real column, fully reduced (fp252.h)"""
    if not used:
        return ""
    lines = ["// Operands QG_DERIVED_RAW(k, off, idx) are cells of DERIVED COLUMNS (tools/gen_quotient.py derived_column_of): the device builds",
             "// them once per launch (quotient_derive.h).  Where the includer does not define the macro, the cell is computed here, from the",
             "// column it derives from - the same fully reduced value.",
             "#ifndef QG_DERIVED_RAW", "#define QG_DERIVED_FALLBACK", "#define QG_DERIVED_RAW(k, off, idx) QG_DERIVED_FALLBACK_##k(off, idx)", "#endif",
             "#ifdef QG_DERIVED_FALLBACK"]
    for k in used:
        col, terms = derived[k]
        cell = lambda off: "QG_TRACE_RAW(%d, (off) + %du, idx)" % (col, off)
        pos = [_small_multiple(cell(off), c) for off, c in terms if c > 0]
        neg = [_small_multiple(cell(off), -c) for off, c in terms if c < 0]
        total = lambda xs: xs[0] if len(xs) == 1 else "fp_add(%s, %s)" % (total(xs[:-1]), xs[-1])
        expr = total(pos) if not neg else "fp_sub(%s, %s)" % (total(pos) if pos else "fp_zero()", total(neg))
        lines.append("#define QG_DERIVED_FALLBACK_%d(off, idx) %s" % (k, expr))
    lines.append("#endif")
    return "\n".join(lines) + "\n"


def _alpha_fallback(alpha, used, n_tables, scaled_tables):
    """QG_TABLE_ALPHA_RAW where nobody defined it: an entry of alpha copy j computed from the table's scaled copy and the constant table"""
    if not used:
        return ""
    lines = ["// Operands QG_TABLE_ALPHA_RAW(j, idx) are entries of ALPHA COPIES of multiplier-only periodic tables (tools/gen_quotient.py",
             "// fold_alpha_tables): copy j is a table times one constraint's coefficient in one of the constant forms - the launch makes them",
             "// behind the scaled tables (csrc/quotient.hip qg_copy_tables_kernel).  Where the includer does not define the macro, the entry is",
             "// the product of the scaled table's entry by that form of the constant - the same value mod p, fully reduced.",
             "#ifndef QG_TABLE_ALPHA_RAW", "#define QG_TABLE_ALPHA_FALLBACK", "#define QG_TABLE_ALPHA_RAW(j, idx) QG_TABLE_ALPHA_FALLBACK_##j(idx)",
             "#define QG_PIN_WIDE(w)", "#endif",
             "#ifdef QG_TABLE_ALPHA_FALLBACK"]
    for j in used:
        t, c, form = alpha[j]
        lines.append("#define QG_TABLE_ALPHA_FALLBACK_%d(idx) fl_to_fp(fl_mul_r280(fl_from_fp(QG_TABLE_SCALED_RAW(%d, idx)), QG_CONST_%s(%d)))"
                     % (j, n_tables + scaled_tables.index(t), ALPHA_FORMS[form], c))
    lines.append("#endif")
    return "\n".join(lines) + "\n"


_ALPHA_FALLBACK_END = '''#ifdef QG_TABLE_ALPHA_FALLBACK
%s#undef QG_TABLE_ALPHA_RAW
#undef QG_PIN_WIDE
#undef QG_TABLE_ALPHA_FALLBACK
#endif
'''
_DERIVED_FALLBACK_END = '''#ifdef QG_DERIVED_FALLBACK
%s#undef QG_DERIVED_RAW
#undef QG_DERIVED_FALLBACK
#endif
'''


def _emit_body(ins, n_consts, n_slots, mem_ops, mem_index, D, fused, out_macro, sync_every, SUB_LAZY2, CONST_FACTOR, SCALED, plan, small=None, flush_on_switch=False, flush_after=()):
    """one pass over the (part) program: -> (lines, stats); raises WideViolation"""
    n_instr = len(ins)
    wide_mul, wide_close, wide_struct = plan
    out = []
    emit = out.append
    bound = [1, 1, 1, 1, 1]                        # four accumulators of the program format + the generator's own (TEMP_ACC)
    stats = {"mul": 0, "mulr": 0, "reduce": 0, "loads": len(mem_ops), "fused": 0, "flushes": 0, "wide_terms": 0, "wide_closes": 0, "wide_neg": 0,
             "alpha_terms": 0, "baked": {}}                          # baked: constant -> multiplications by it written as shifts and adds
    small = small or {}
    last_use = {}                                  # memory operand -> the last instruction that reads it (repeated operands share one)
    for pc_, q_ in mem_index.items():
        last_use[q_] = max(last_use.get(q_, -1), pc_)
    wide = {"acc": None, "terms": 0}               # the one wide (unreduced 64-bit column) accumulator of the alpha dot products in flight
    # the constraint whose products are being summed in the second wide accumulator (wq), and which accumulators / slots hold a
    # part of that constraint's value: k -> the constraint, lin -> whether the register (slot) holds a plain part beside what is in wq
    wq = {"k": None, "units": 0, "terms": 0}
    wacc, wslot = [None] * 8, {}
    acc_const = [None] * 8                         # the constant an accumulator was just loaded with (MOV acc, CONST), if it still holds it

    def reduce_acc(d):
        emit("    acc%d = fl_weak_reduce(acc%d);" % (d, d))
        bound[d] = 1
        stats["reduce"] += 1

    def negate_acc(d):
        """acc = -acc as C p - acc, limb-wise and borrow-free (fl252.h fl_sub_c): the template by the value's bound"""
        if bound[d] > 4:
            reduce_acc(d)
        c, f, nb = {1: (2, 1, 2), 2: (8, 2, 4), 3: (16, 4, 8), 4: (16, 4, 8)}[bound[d]]
        emit("    acc%d = fl_sub_c<%d, %d>(fl_zero(), acc%d);" % (d, c, f, d))
        bound[d] = nb

    NEG_TEMPLATE = {1: (2, 1, 2), 2: (8, 2, 4), 3: (16, 4, 8), 4: (16, 4, 8)}      # fl_sub_c<C, F> by the subtrahend's bound -> the result's

    def small_multiple(k, b, product_cost):
        """constant k times a value of bound b as shifts and adds, if that is cheaper than the product it replaces: -> scale_plan's
        (steps, cost, bound), or None.  Priced with the weak reductions the bounds force: inside the plan, before a negation of a
        bound above 4, and one more for a result above 4 (the next subtraction or negation of it pays that)."""
        if k not in small:
            return None
        plan = scale_plan(small[k][0], b)
        if plan is None:
            return None
        steps, cost, ob = plan
        if small[k][0] < 0:
            cost += 9 + (REDUCE_COST if ob > 4 else 0)
            ob = NEG_TEMPLATE[1 if ob > 4 else ob][2]
        if ob > 4:
            cost += REDUCE_COST
        if cost >= product_cost and os.environ.get("QG_VERBOSE"):
            print("   stays a product: constant %d (%d) on bound %d, %d >= %d" % (k, small[k][0], b, cost, product_cost))
        return plan if cost < product_cost else None

    def emit_scaled(k, plan, d, expr):
        """acc_d = constant k x expr by the plan (its leading reduction, if any, was applied to expr by the caller)"""
        steps = [st for st in plan[0]]
        if steps[0] == "R":
            steps = steps[1:]
        emit("    acc%d = QG_SCALE(%d, %d, %s);" % (d, k, steps[0], expr))
        b = plan[3] * steps[0]
        for st in steps[1:]:
            if st == "R":
                bound[d] = b
                reduce_acc(d)
                b = 1
            else:
                emit("    acc%d = QG_RESCALE(%d, acc%d);" % (d, st, d))
                b *= st
        bound[d] = b
        if small[k][0] < 0:
            if bound[d] > 4:
                reduce_acc(d)
            c_, f_, nb = NEG_TEMPLATE[bound[d]]
            emit("    acc%d = QG_NEGSCALED(%d, %d, acc%d);" % (d, c_, f_, d))
            bound[d] = nb
        stats["baked"][k] = stats["baked"].get(k, 0) + 1

    def flush_wide():
        """fold the pending dot product into its accumulator: one Montgomery reduction for all its terms"""
        d = wide["acc"]
        if d is None:
            return
        if bound[d] + 1 > MAX_BOUND:
            reduce_acc(d)
        emit("    acc%d = fl_add(acc%d, qg_dot_reduce(wd));" % (d, d))
        bound[d] += 1
        wide["acc"], wide["terms"] = None, 0
        stats["flushes"] += 1

    def issue(j, nxt):
        """start the load of memory operand j (of this point, or of the next one) into its rotating register"""
        emit("    m%d = %s;  QG_PIN_LOADS" % (j % D, mem_ops[j][1] % ("inext" if nxt else "i32")))

    skip_add = set()
    for pc, (op, d, kind, w1) in enumerate(ins):
        v = "acc%d" % d
        const_before = acc_const[d] if d < 8 else None
        if op in (OP_MOV, OP_ADD, OP_SUB, OP_RSUB, OP_MUL, OP_INV) and d < 8:
            acc_const[d] = w1 if (op == OP_MOV and kind == SRC_CONST) else None
        if pc:
            emit("    QG_FENCE")
        if sync_every and pc and pc % sync_every == 0:
            emit("    QG_SYNC")
        if pc in skip_add:                          # the ADD of a fused pair: already accounted in the wide accumulator
            if pc in flush_after:
                flush_wide()
            continue
        # any other touch of the accumulator that carries a pending dot product needs its value: flush first
        touches = {d} | ({w1 & 7} if op <= OP_MUL and kind == SRC_ACC else set())
        if wide["acc"] is not None and wide["acc"] in touches and not (pc in fused and fused[pc] == wide["acc"] and wide["acc"] != d):
            flush_wide()
        # ---- the operand: an expression of type Fl and its lazy bound
        src, sb, src_acc = None, 1, None
        if op <= OP_MUL:
            if kind == SRC_ACC:
                src_acc = w1 & 7
                src, sb = "acc%d" % src_acc, bound[src_acc]
            elif kind == SRC_SLOT:
                assert w1 < n_slots
                src = "QG_SLOT(%d)" % w1
            elif kind == SRC_CONST:
                assert w1 < n_consts
                src = ("QG_CONST_R280(%d)" if op == OP_MUL else "QG_CONST(%d)") % w1
            elif kind in (SRC_TRACE, SRC_TABLE, SRC_DERIVED, SRC_TALPHA):
                src = "fl_from_fp(m%d)" % (mem_index[pc] % D)
            else:
                assert kind == SRC_X
                src = "x"

        def reduce_src():
            """weakly reduce the operand; an accumulator operand is reduced in place (same value mod p)"""
            nonlocal sb
            assert src_acc is not None
            if src_acc != d:
                reduce_acc(src_acc)
            sb = 1

        # ---- the constraint's own wide sum (plan_wide_constraints): what this instruction does to the PLAIN parts of its operands
        sm = wacc[src_acc] if src_acc is not None else (wslot.get(w1) if op <= OP_MUL and kind == SRC_SLOT else None)
        dm = wacc[d] if op != OP_MOV else None
        op_e = op                                   # None: nothing to compute; "NEG" / "NEGMOV": the plain part changes sign
        closed_here = False                         # this MUL takes a constraint's wide sum back: its constant stays a factor
        if op == OP_MOV:
            wacc[d] = dict(sm) if sm else None
            if sm and not sm["lin"]:
                op_e = None
        elif op == OP_ST:
            wslot[w1] = dict(dm) if dm else None
            if dm and not dm["lin"]:
                op_e = None
        elif op in (OP_ADD, OP_SUB, OP_RSUB):
            if sm or dm:
                k = (dm or sm)["k"]
                if sm and dm and sm["k"] != dm["k"]:
                    raise WideViolation(k, "meets another constraint's sum at pc %d" % pc)
                if wide_struct.get(pc) != k or src_acc == d:
                    raise WideViolation(k, "used outside its sum at pc %d" % pc)
                lin_d, lin_s = (dm["lin"] if dm else True), (sm["lin"] if sm else True)
                wacc[d] = {"k": k, "lin": lin_d or lin_s}
                if lin_d and lin_s:
                    pass
                elif lin_d:
                    op_e = "NEG" if op == OP_RSUB else None
                elif lin_s:
                    op_e = "NEGMOV" if op == OP_SUB else OP_MOV
                else:
                    op_e = None
        elif op == OP_MUL:
            if pc in wide_mul:
                op_e = "WMAD"
                if sm or dm:
                    raise WideViolation((sm or dm)["k"], "a factor at pc %d" % pc)
            elif dm is not None and pc in wide_close and dm["k"] == pc:
                g, nterms = wide_close[pc]
                if wq["k"] != pc or wq["terms"] != nterms:
                    raise WideViolation(pc, "closed with %d of %d products" % (wq["terms"], nterms))
                if dm["lin"]:                                      # + L 2^256 (g L where the sum is -C)
                    if g < 0:
                        negate_acc(d)
                    emit("    qg_wide_tail(wq, %s);" % v)
                emit("    %s = qg_dot_reduce(wq);" % v)               # g C 2^-24, normalised
                bound[d] = 1
                for r_ in range(8):
                    if wacc[r_] is not None and wacc[r_]["k"] == pc:
                        wacc[r_] = None
                for r_ in list(wslot):
                    if wslot[r_] is not None and wslot[r_]["k"] == pc:
                        wslot[r_] = None
                wq.update(k=None, units=0, terms=0)
                stats["wide_closes"] += 1
                closed_here = True
                if kind == SRC_CONST:                              # (an alpha copy was chosen in that form: generate_body)
                    src = ("QG_CONST_R280_UP(%d)" if g > 0 else "QG_CONST_R280_UPN(%d)") % w1
            elif sm or dm:
                raise WideViolation((sm or dm)["k"], "multiplied at pc %d" % pc)
            if kind == SRC_TALPHA and (pc in wide_close) != closed_here:
                raise WideViolation(pc, "planned to close a wide sum that is not there")
        elif op in (OP_INV, OP_OUT) and wacc[d] is not None:
            raise WideViolation(wacc[d]["k"], "used at pc %d" % pc)

        if op_e is None:
            pass
        elif op_e == "NEG":
            negate_acc(d)
        elif op_e == "NEGMOV":
            if sb > 1:
                reduce_src()
            emit("    %s = fl_sub_c<2, 1>(fl_zero(), %s);" % (v, src))
            bound[d] = 2
        elif op_e == "WMAD":
            k, sg = wide_mul[pc]
            if wq["k"] is None:
                emit("    qg_dot_zero(wq);")
                wq.update(k=k, units=0, terms=0)
            elif wq["k"] != k:                                    # the one that stays open across other constraints gives way
                raise WideViolation(max(k, wq["k"]), "the sums of constraints %d and %d overlap" % (wq["k"], k))
            # a term of factors bounded a and b puts < 9 a b 2^56 into a column: the sum's terms share DOT_MAX_TERMS units (one kept
            # for L 2^256; a negation doubles one factor's bound)
            room = min(DOT_MAX_TERMS - 1 - wq["units"], max(2, (DOT_MAX_TERMS - 1) // wide_close[k][1]))     # (a fair share per term)
            neg = 2 if sg < 0 else 1
            if bound[d] * sb * neg > room:
                if sb >= bound[d] and src_acc is not None:
                    reduce_src()
                else:
                    reduce_acc(d)
                if bound[d] * sb * neg > room and bound[d] > 1:
                    reduce_acc(d)
                if bound[d] * sb * neg > room and sb > 1 and src_acc is not None:
                    reduce_src()
                if bound[d] * sb * neg > room:
                    raise WideViolation(k, "more than a reduction's worth of products")
            a_expr, a_b, b_expr, b_b = v, bound[d], src, sb
            if sg < 0:                                             # - A B = A (2p - B): a normalised factor is negated
                if b_b == 1:
                    b_expr, b_b = "fl_sub_c<2, 1>(fl_zero(), %s)" % b_expr, 2
                else:
                    if a_b > 1:
                        reduce_acc(d)
                    a_expr, a_b = "fl_sub_c<2, 1>(fl_zero(), %s)" % a_expr, 2
                stats["wide_neg"] += 1
            if wq["units"] + a_b * b_b > DOT_MAX_TERMS - 1:        # (one unit kept for the L 2^256 term)
                raise WideViolation(k, "more than a reduction's worth of products")
            emit("    qg_dot_mad(wq, %s, %s);" % (a_expr, b_expr))
            wq["units"] += a_b * b_b
            wq["terms"] += 1
            wacc[d] = {"k": k, "lin": False}
            bound[d] = 1
            stats["wide_terms"] += 1
            stats["mul"] += 1
        elif op_e == OP_MOV:
            emit("    %s = %s;" % (v, src))
            bound[d] = sb
        elif op_e == OP_ADD:
            if src_acc == d:                                   # v + v
                if 2 * bound[d] > MAX_BOUND:
                    reduce_acc(d)
                emit("    %s = fl_add(%s, %s);" % (v, v, v))
                bound[d] *= 2
            else:
                if bound[d] + sb > MAX_BOUND:
                    reduce_acc(d)
                if bound[d] + sb > MAX_BOUND:
                    reduce_src()
                emit("    %s = fl_add(%s, %s);" % (v, v, src))
                bound[d] += sb
        elif op_e == OP_SUB:
            if src_acc == d:                                   # v - v
                reduce_acc(d)
                emit("    %s = fl_sub_c<2, 1>(%s, %s);" % (v, v, v))
                bound[d] = 2
            else:
                # a subtrahend of bound 2 (a sum of two normalised values, a difference of them) is taken as it is by fl_sub_c<8, 2>
                # (+ 8p: four units) where the result stays within MAX_BOUND - otherwise it is reduced first (54 instructions)
                if sb == 2 and SUB_LAZY2 and min(bound[d], 1 if bound[d] + 4 > MAX_BOUND else bound[d]) + 4 <= MAX_BOUND:
                    if bound[d] + 4 > MAX_BOUND:
                        reduce_acc(d)
                    emit("    %s = fl_sub_c<8, 2>(%s, %s);" % (v, v, src))
                    bound[d] += 4
                else:
                    if sb > 1:
                        reduce_src()
                    if bound[d] + 1 > MAX_BOUND:
                        reduce_acc(d)
                    emit("    %s = fl_sub_c<2, 1>(%s, %s);" % (v, v, src))
                    bound[d] += 1
        elif op_e == OP_RSUB:
            assert src_acc != d
            if bound[d] == 2 and SUB_LAZY2 and sb + 4 <= MAX_BOUND:      # the flags: cell - 2 x next cell
                emit("    %s = fl_sub_c<8, 2>(%s, %s);" % (v, src, v))
                bound[d] = sb + 4
            else:
                if bound[d] > 1:
                    reduce_acc(d)
                if sb + 1 > MAX_BOUND:
                    reduce_src()
                emit("    %s = fl_sub_c<2, 1>(%s, %s);" % (v, src, v))
                bound[d] = sb + 1
        elif op_e == OP_MUL:
            tgt = fused.get(pc)
            # ---- a small structural multiple instead of the product (structural_constants, scale_plan): "MUL acc, c" scales the
            #      accumulator, "MOV acc, c; MUL acc, x" the operand.  Priced against what the product would be here: a term of the
            #      open dot product (whose sum the plain ADD that follows then has to flush: a reduction more), else a product
            scaling = None
            if os.environ.get("QG_VERBOSE") and ((kind == SRC_CONST and w1 in small) or (const_before in small and kind != SRC_CONST)):
                print("   pc %d: small constant, closes a wide sum %s, fused %s, wide open on %s" % (pc, closed_here, tgt, wide["acc"]))
            if small and not closed_here and src_acc != d:
                if kind == SRC_CONST and w1 in small:
                    fused_here = tgt is not None and wide["acc"] in (None, tgt)
                    against = PRODUCT_COST if not fused_here else WIDE_TERM_COST if wide["acc"] is None else WIDE_TERM_COST - 9 - 104
                    plan_ = small_multiple(w1, bound[d], against)
                    if plan_ is not None:
                        if plan_[0][0] == "R":
                            reduce_acc(d)
                        scaling = (w1, plan_ + (bound[d],), v)
                elif kind not in (SRC_CONST, SRC_TALPHA) and const_before is not None and const_before in small and not (kind == SRC_TABLE and w1 in SCALED):
                    plan_ = small_multiple(const_before, sb, PRODUCT_COST)
                    if plan_ is not None and not (plan_[0][0] == "R" and src_acc is None):
                        if plan_[0][0] == "R":
                            reduce_src()
                        scaling = (const_before, plan_ + (sb,), src)
            if flush_on_switch and scaling is None and tgt is not None and wide["acc"] not in (None, tgt):
                flush_wide()                                   # the part's total gives way to a group's own sum, and back
            if scaling is not None:
                emit_scaled(scaling[0], scaling[1], d, scaling[2])
            elif tgt is not None and (wide["acc"] in (None, tgt)):
                # term of a dot product: acc_tgt += v * alpha^k with the reduction deferred.  A multiplicand of bound b (limbs
                # < b 2^28) adds < 9 b 2^56 to a column: the terms' bounds may sum to DOT_MAX_TERMS before the columns near 2^64
                if bound[d] > 4:
                    reduce_acc(d)
                if wide["acc"] is not None and wide["terms"] + bound[d] > DOT_MAX_TERMS:
                    flush_wide()
                if wide["acc"] is None:
                    emit("    qg_dot_zero(wd);")
                    wide["acc"] = tgt
                emit("    qg_dot_mad(wd, %s, %s);" % (v, src))
                if kind == SRC_TALPHA and ALPHA_PIN:               # (the factor is a register, not an LDS read: nothing else keeps the
                    emit("    QG_PIN_WIDE(wd)")                    #  81 multiply-adds here - see quotient_gen.h)
                wide["terms"] += bound[d]
                stats["fused"] += 1
                stats["alpha_terms"] += kind == SRC_TALPHA
                skip_add.add(pc + 1)
            elif src_acc == d:                                 # v * v: the square routine wants a normalised value
                if bound[d] > 1:
                    reduce_acc(d)
                emit("    %s = fl_sqr(%s);" % (v, v))
                bound[d] = 1
            elif kind in (SRC_CONST, SRC_TALPHA):                 # (an alpha copy is canonical and carries its 2^24, like a scaled table)
                emit("    %s = fl_mul_r280(%s, %s);" % (v, v, src))
                stats["mulr"] += 1
                bound[d] = 1
            elif kind == SRC_TABLE and w1 in SCALED:              # the table's 2^24-fold copy: canonical, normalised - an R280 operand
                emit("    %s = fl_mul_r280(%s, %s);" % (v, v, src))
                stats["mulr"] += 1
                bound[d] = 1
            elif CONST_FACTOR and const_before is not None and src_acc != d:      # MOV acc, c ; MUL acc, value: the constant is the R280 operand
                emit("    %s = fl_mul_r280(%s, QG_CONST_R280(%d));" % (v, src, const_before))
                stats["mulr"] += 1
                bound[d] = 1
            else:
                # both factors may be lazy: limbs < a 2^28 and < b 2^28 put < 9 a b 2^56 into a column (a b <= 16 fits 64 bits beside
                # the reduction's own terms) and the product / 2^256 + p stays below 2p - a normalised result - for a b <= 8
                # (round 4; before, one factor was always reduced first: 54 instructions for every product of two differences)
                if LAZY_PRODUCT_MAX == 0:                       # (rounds 2-3: one factor always normalised)
                    if sb > 1 and bound[d] > 1:
                        reduce_src()
                elif bound[d] * sb > LAZY_PRODUCT_MAX:
                    if sb >= bound[d] and src_acc is not None:
                        reduce_src()
                    else:
                        reduce_acc(d)
                    if bound[d] * sb > LAZY_PRODUCT_MAX:
                        reduce_acc(d) if bound[d] > 1 else reduce_src()
                emit("    %s = fl_mul(%s, %s);" % (v, v, src))
                bound[d] = 1
            stats["mul"] += 1
        elif op_e == OP_INV:
            if bound[d] > 1:
                reduce_acc(d)
            else:
                emit("    %s = fl_weak_reduce(%s);" % (v, v))
            emit("    %s = fn_inv(%s);" % (v, v))
            bound[d] = 1
        elif op_e == OP_ST:
            assert w1 < n_slots
            if bound[d] > 1:
                reduce_acc(d)
            emit("    QG_SLOT_STORE(%d, %s);" % (w1, v))
        else:
            flush_wide()
            emit("    %s(%s);" % (out_macro, v))
        # this instruction consumed memory operand q and freed register q % D: start the load of operand q + D there - or, in
        # the last D steps of a point, of the next point's operand whose home register that is (operand j lives in m[j % D];
        # when D does not divide the operand count the tail fills the registers in rotated order)
        if pc in mem_index and last_use[mem_index[pc]] == pc:
            q, L = mem_index[pc], len(mem_ops)
            if q + D < L:
                issue(q + D, False)
            else:
                issue(q % D, True)
    assert wide["acc"] is None
    if wq["k"] is not None:
        raise WideViolation(wq["k"], "never closed")
    return out, stats


def write_part(layout, suffix, part, n_parts, base, body, n_instr, n_consts, n_slots, slots_in_regs, wgs, fence, threads, sync=0):
    src = """// GENERATED by tools/gen_quotient.py - DO NOT EDIT; regenerate with `python tools/gen_quotient.py %(layout)s`.
//
// The composition constraint of the `%(layout)s` layout (layouts/src/%(layout)s/air.rs; lowered by
// sandstorm_amd/host/air_%(layout)s.cpp + air_program.cpp) as straight-line code for gfx950%(variant)s - PART %(part)d OF %(n_parts)d
// (the parts' outputs sum to the composition; part 0 stores, the others add into the output: tools/gen_quotient.py
// split_program): %(n_instr)d program instructions, %(mul)d multiplications (%(mulr)d by a constant in R280 form, %(fused)d as terms of
// %(flushes)d fused dot products), %(loads)d trace / table operand loads issued %(depth)d operands ahead of their use, %(reduce)d weak reductions
// placed at generation time, %(n_slots)d scratch values per point in %(where)s, constants in LDS, register budget for %(wgs)d
// workgroup(s) per CU%(fence)s.
%(define)s#include "quotient_gen.h"

namespace ss {
namespace {

__global__ __launch_bounds__(QG_THREADS, %(wgs)d) void quotient_%(layout)s%(suffix)s_p%(part)d_kernel(QGenArgs a) {
    QG_PROLOGUE(%(n_consts)d, %(lds_slots)d)
#include "%(inc)s"
}

hipError_t launch(hipStream_t st, const QGenArgs &a, uint32_t blocks) {
    const size_t lds = qg_lds_bytes(%(n_consts)d, %(lds_slots)d);
    static bool attr_set = false;            // > 64 KiB of dynamic LDS needs the per-function opt-in
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&quotient_%(layout)s%(suffix)s_p%(part)d_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(quotient_%(layout)s%(suffix)s_p%(part)d_kernel, dim3(blocks), dim3(QG_THREADS), lds, st, a);
    return hipGetLastError();
}

}  // namespace

QGenPart quotient_gen_%(layout)s%(suffix)s_p%(part)d() { return QGenPart{%(wgs)du, (uint32_t)QG_THREADS, %(n_instr)du, launch}; }

}  // namespace ss
""" % dict(layout=layout, suffix=suffix, variant=" (variant `%s`)" % suffix if suffix else "", part=part, n_parts=n_parts, n_instr=n_instr,
           n_slots=n_slots, n_consts=n_consts, wgs=wgs, lds_slots=0 if slots_in_regs else n_slots,
           where="registers" if slots_in_regs else "LDS",
           define=("#define QG_SLOTS_IN_REGISTERS\n" if slots_in_regs else "") + ("#define QG_FENCE_EVERY_INSTRUCTION\n" if fence else "")
                  + ("#define QG_THREADS_PER_WG %d\n" % threads if threads != 256 else "") + ("#define QG_SYNC_WAVES\n" if sync else ""),
           fence=(", a scheduling fence after every program instruction" if fence else "")
                 + (", a workgroup barrier every %d program instructions (the waves share their instruction fetches)" % sync if sync else ""), **body)
    with open(os.path.join(OUT_DIR, base + ".hip"), "w") as f:
        f.write(src)


def write_kernel_table(layout, suffix, variant, code, n_consts, n_tables, ncols, n_parts, scaled=(), derived=(), baked=(), alpha=()):
    """the host-side entry of one variant: what ss_eval_quotient looks up by the program's hash.  `baked`: (constant, Montgomery image)
    of every constant some part multiplies by with shifts and adds - the launch compares them with the program's constant table.
    `alpha`: the alpha copies (table, constant, form) the parts read through QG_TABLE_ALPHA_RAW, in the bodies' numbering"""
    decl = "".join("QGenPart quotient_gen_%s%s_p%d();\n" % (layout, suffix, j) for j in range(n_parts))
    parts = ", ".join("quotient_gen_%s%s_p%d()" % (layout, suffix, j) for j in range(n_parts))
    src = """// GENERATED by tools/gen_quotient.py - DO NOT EDIT; regenerate with `python tools/gen_quotient.py %(layout)s`.
//
// The compiled composition constraint of the `%(layout)s` layout, variant %(variant)d: %(n_parts)d kernel(s) (quotient_gen_%(layout)s%(suffix)s_p*.hip) whose
// outputs sum to the program's.  Code hash (FNV-1a of the program's code words) 0x%(hash)016x: ss_eval_quotient launches these
// kernels for exactly that program and interprets any other.
#include "quotient_gen.h"

namespace ss {

%(decl)s
const QGenKernel &quotient_gen_%(layout)s%(suffix)s() {
    // tables the kernels read from a copy times 2^24 (multiplier-only tables: tools/gen_quotient.py generate): descriptor n_tables + j
    static const uint32_t scaled[] = {%(scaled)s};
    // derived columns the kernels read (tools/gen_quotient.py derived_column_of; built per launch, quotient_derive.h): the trace column,
    // then (row offset, coefficient) per term
    // constants the kernels hold as code (small structural multiples: tools/gen_quotient.py structural_constants): constant index and the
    // interchange image it must have - ss_eval_quotient interprets a program whose table says otherwise
    static const QGenBaked baked[] = {%(baked)s};
    // alpha copies the kernels read (tools/gen_quotient.py fold_alpha_tables; made per launch behind the scaled tables): copy j is table
    // `table` times constant `constant` in form 0 (R280: times 2^24), 1 (R280_UP: times 2^48) or 2 (R280_UPN: times -2^48)
    static const QGenAlpha alpha[] = {%(alpha)s};
    static const QGenKernel k = {"%(layout)s", 0x%(hash)016xull, %(n_instr)du, %(n_consts)du, %(n_tables)du, %(ncols)du, %(variant)du, %(n_parts)du, {%(parts)s},
                                 %(n_baked)du, baked, %(n_alpha)du, alpha, %(n_scaled)du, scaled, %(n_derived)du, {%(derived)s}};
    return k;
}

}  // namespace ss
""" % dict(layout=layout, suffix=suffix, variant=variant, n_parts=n_parts, hash=code_hash(code), n_instr=len(code) // 2, n_consts=n_consts,
           n_tables=n_tables, ncols=ncols, decl=decl, parts=parts, n_scaled=len(scaled), scaled=", ".join("%du" % t for t in scaled) if scaled else "0u", n_derived=len(derived), n_baked=len(baked),
           n_alpha=len(alpha), alpha=", ".join("{%du, %du, %du}" % a for a in alpha) if alpha else "{0u, 0u, 0u}",
           baked=", ".join("{%du, {%s}}" % (c, ", ".join("0x%016xull" % ((v >> (64 * j)) & (2**64 - 1)) for j in range(4))) for c, v in baked) if baked else "{0u, {0, 0, 0, 0}}",
           derived=", ".join("{%du, %du, {%s}, {%s}}" % (col, len(terms), ", ".join("%du" % off for off, _ in terms), ", ".join("%d" % c for _, c in terms))
                             for col, terms in derived))
    with open(os.path.join(OUT_DIR, "quotient_gen_%s%s.hip" % (layout, suffix)), "w") as f:
        f.write(src)
    if not suffix:                                  # the same list for the host build of the bodies (tests/cpp/quotient_gen_host_test.cpp)
        with open(os.path.join(OUT_DIR, "quotient_gen_%s_scaled.inc" % layout), "w") as f:
            f.write("// GENERATED by tools/gen_quotient.py - DO NOT EDIT.  Tables the `%s` kernels read from a copy times 2^24.\n"
                    "static const uint32_t QG_N_TABLES = %du, QG_N_SCALED = %du;\nstatic const uint32_t QG_SCALED_TABLES[] = {%s};\n"
                    % (layout, n_tables, len(scaled), ", ".join("%du" % t for t in scaled) if scaled else "0u"))
            f.write("// ... and the alpha copies, in the bodies' numbering: {table, constant, form (0 R280, 1 R280_UP, 2 R280_UPN)}\n"
                    "static const uint32_t QG_N_ALPHA = %du;\nstatic const uint32_t QG_ALPHA_COPIES[][3] = {%s};\n"
                    % (len(alpha), ", ".join("{%du, %du, %du}" % a for a in alpha) if alpha else "{0u, 0u, 0u}"))


def write_source_lists(written, all_variants):
    """csrc/quotient_gen_sources.mk (what the Makefile and tests/hipemu/build.sh compile) and csrc/quotient_gen_variants.inc (the
    X-macro list capi.hip's lookup table is made of)"""
    csrc = OUT_DIR
    default = [n for layout in written for k, _, names in written[layout] if k == 0 for n in names]
    ab = [n for layout in written for k, _, names in written[layout] if k != 0 for n in names]
    with open(os.path.join(csrc, "quotient_gen_sources.mk"), "w") as f:
        f.write("# GENERATED by tools/gen_quotient.py: the generated constraint kernels' translation units\n")
        f.write("QG_SRCS := %s\n" % " ".join(default))
        if all_variants:
            f.write("# make QG_AB=1: the A/B variants (python tools/gen_quotient.py --all-variants), selected with SS_QG_VARIANT=k\n")
            f.write("QG_AB_SRCS := %s\n" % " ".join(ab))
    with open(os.path.join(csrc, "quotient_gen_variants.inc"), "w") as f:
        f.write("// GENERATED by tools/gen_quotient.py: QG_VARIANT(entry) per compiled program variant\n")
        for layout in written:
            for k, suffix, _ in written[layout]:
                line = "QG_VARIANT(quotient_gen_%s%s)\n" % (layout, suffix)
                f.write(line if k == 0 else "#ifdef SS_QG_AB_VARIANTS\n%s#endif\n" % line)


if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["starknet", "recursive"]
    assert sorted(names) == ["recursive", "starknet"], "the source lists cover both layouts: generate both"
    everything = "--all-variants" in sys.argv
    write_source_lists({name: generate(name, everything) for name in names}, everything)
