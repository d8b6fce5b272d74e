"""Alpha copies of the periodic multiplier tables (tools/gen_quotient.py fold_alpha_tables), checked without a GPU.

A zerofier group (sum_k alpha^k C_k) x T pays a reduction and a product by T at every point; where T is a multiplier-only periodic
table the kernels read T'_k = alpha^k T from one copy per constraint and every constraint is a term of the part's running wide sum.

  * the rewrite of the instruction stream on hand-made groups: which shapes are taken and which are left as they are, and that the
    rewritten program is the same function (the oracle's constraint VM on the original against the body of the rewritten one);
  * the committed bodies of both layouts built twice - with the harness that leaves QG_TABLE_ALPHA_RAW to the bodies' fallback (the
    scaled table's entry times the constant, at every read) and with the one that defines it as the device does, a read of copies made
    by the library's own per-entry function from descriptors laid out as the launch lays them out
    (tests/cpp/quotient_gen_alpha_host_test.cpp) - on the same random inputs, whole domain and a row block that starts inside a period;
  * qg_alpha_factor and the copies' entries against Python integers, factors and entries at 0, 1 and p - 1 included.

Results are field elements: equality, no tolerance."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_quotient_gen_host import CPP, ROOT, _extreme, part_bodies, program, run_host
from tests.test_gpu_real_quotient import _rand
from tests.test_layout_starknet import P

sys.path.insert(0, os.path.join(ROOT, "tools"))
ALPHA_CPP = os.path.join(ROOT, "tests", "cpp", "quotient_gen_alpha_host_test.cpp")

OP_MOV, OP_ADD, OP_SUB, OP_RSUB, OP_MUL, OP_INV, OP_ST, OP_OUT = range(8)
ACC, SLOT, CONST, TRACE, TABLE, X = range(6)
NCOLS, NCONSTS, NTABLES, NSLOTS, LOG_N = 6, 24, 4, 2, 6
T = lambda col, off: (TRACE, (col << 24) | off)


def alpha_copies(layout):
    """(table, constant, form) of the committed kernel table (csrc/quotient_gen_<layout>.hip)"""
    with open(os.path.join(ROOT, "sandstorm_amd", "csrc", "quotient_gen_%s.hip" % layout)) as f:
        listed = re.search(r"QGenAlpha alpha\[\] = \{(.*)\};", f.read()).group(1)
    return [tuple(int(v) for v in m) for m in re.findall(r"\{(\d+)u, (\d+)u, (\d+)u\}", listed)]


def hand_made():
    """four groups: three constraints times table 0 that open the total (MOV), one constraint times table 1, two constraints times
    table 2 AND the linear factor x (not taken), two constraints times table 3 whose first term is not a product by a constant (not taken)"""
    ins, alpha = [], [8]

    def e(op, d, kind=0, w1=0):
        ins.append((op, d, kind, w1))

    def close(first):
        e(OP_MUL, 2 if not first else 1, CONST, alpha[0])
        alpha[0] += 1
        if not first:
            e(OP_ADD, 1, ACC, 2)
    # group 0
    e(OP_MOV, 1, *T(0, 0)); e(OP_MUL, 1, *T(1, 0)); e(OP_SUB, 1, *T(2, 1)); close(True)
    e(OP_MOV, 2, *T(3, 0)); e(OP_MUL, 2, ACC, 2); e(OP_SUB, 2, *T(3, 0)); close(False)
    e(OP_MOV, 2, *T(4, 2)); e(OP_SUB, 2, *T(5, 0)); close(False)
    e(OP_MUL, 1, TABLE, 0); e(OP_MOV, 0, ACC, 1)
    # group 1: one constraint
    e(OP_MOV, 1, *T(1, 1)); e(OP_MUL, 1, *T(0, 2)); e(OP_ADD, 1, CONST, 2); close(True)
    e(OP_MUL, 1, TABLE, 1); e(OP_ADD, 0, ACC, 1)
    # group 2: a further factor behind the table
    e(OP_MOV, 1, *T(2, 0)); e(OP_SUB, 1, *T(2, 1)); close(True)
    e(OP_MOV, 2, *T(5, 1)); e(OP_MUL, 2, *T(4, 0)); close(False)
    e(OP_MUL, 1, TABLE, 2); e(OP_MUL, 1, X, 0); e(OP_ADD, 0, ACC, 1)
    # group 3: its first term carries no coefficient
    e(OP_MOV, 1, *T(3, 1)); e(OP_MUL, 1, *T(3, 2))
    e(OP_MOV, 2, *T(0, 1)); e(OP_SUB, 2, CONST, 3); close(False)
    e(OP_MUL, 1, TABLE, 3); e(OP_ADD, 0, ACC, 1)
    e(OP_OUT, 0)
    return ins


def test_the_rewrite_takes_the_groups_it_can_express():
    import gen_quotient as g
    ins = hand_made()
    report = []
    out, groups, constraints, ends = g.fold_alpha_tables(ins, {0, 1, 2, 3}, report)
    assert (groups, constraints) == (2, 4)
    assert len(report) == 2 and "table 2" in report[0] and "table 3" in report[1]
    talpha = [(d, w1 >> 16, w1 & 0xffff) for op, d, kind, w1 in out if kind == g.SRC_TALPHA]
    assert talpha == [(1, 0, 8), (2, 0, 9), (2, 0, 10), (1, 1, 11)]                     # (accumulator, table, constant)
    # the folded tables are no longer operands, the others still are; every folded constraint is added to the total on its own
    assert [w1 for op, _, kind, w1 in out if kind == TABLE] == [2, 3]
    k = [pc for pc, (_, _, kind, _) in enumerate(out) if kind == g.SRC_TALPHA]
    assert [out[pc + 1] for pc in k] == [(OP_MOV, 0, ACC, 1), (OP_ADD, 0, ACC, 2), (OP_ADD, 0, ACC, 2), (OP_ADD, 0, ACC, 1)]
    assert ends == {k[2] + 1, k[3] + 1}
    # a table that is not multiplier-only (not in the set) is left alone, and so is everything when the set is empty
    assert g.fold_alpha_tables(ins, set())[0] == ins
    assert g.fold_alpha_tables(ins, {1})[1:3] == (1, 1)
    # a total that the group itself uses as a temporary cannot take the group's terms early
    busy = list(ins)
    at = busy.index((OP_MOV, 2, *T(4, 2)))
    busy[at:at] = [(OP_MOV, 0, *T(0, 0))]
    assert g.fold_alpha_tables(busy, {0})[1] == 0


@pytest.mark.parametrize("knobs", [(True, True, 3, "never"), (True, False, 2, "group"), (False, False, 1, "never")],
                         ids=lambda k: "wide%d-lazy%d-d%d-%s" % (int(k[0]), int(k[1]), k[2], k[3]))
def test_hand_made_groups_through_both_harnesses(oracle, knobs, tmp_path, monkeypatch):
    import gen_quotient as g
    wide, lazy, depth, flush = knobs
    tmp = str(tmp_path)
    monkeypatch.setattr(g, "OUT_DIR", tmp)
    ins = hand_made()
    scaled = [0, 1, 2, 3]
    folded, _, _, ends = g.fold_alpha_tables(ins, set(scaled))
    alpha = []
    stats = g.generate_body("hand", folded, NCONSTS, NSLOTS, NTABLES, NCOLS, depth, "hand.inc", True, "QG_OUT", 0, wide, lazy, lazy, 1, scaled,
                            alpha=alpha, group_ends=ends if flush == "group" else ())
    assert stats["alpha_copies"] == 4 and sorted((t, c) for t, c, _ in alpha) == [(0, 8), (0, 9), (0, 10), (1, 11)]
    if wide:                                                   # constraints with products of their own close their wide sum at the copy
        assert {form for _, _, form in alpha} > {0}
    with open(os.path.join(tmp, "hand.inc")) as f:
        body = f.read()
    assert body.count("QG_PIN_WIDE(wd)") == stats["alpha_terms"] >= 2 and "#ifndef QG_TABLE_ALPHA_RAW" in body
    assert "QG_TABLE_SCALED_RAW(%d, i32)" % (NTABLES + 0) not in body.split("#endif")[-1]      # table 0 is read through its copies only
    with open(os.path.join(tmp, "qg_scaled.h"), "w") as f:
        f.write("static const uint32_t QG_N_TABLES = %du, QG_N_SCALED = %du;\nstatic const uint32_t QG_SCALED_TABLES[] = {%s};\n"
                "static const uint32_t QG_N_ALPHA = %du;\nstatic const uint32_t QG_ALPHA_COPIES[][3] = {%s};\n"
                % (NTABLES, len(scaled), ", ".join("%du" % t for t in scaled), len(alpha), ", ".join("{%du, %du, %du}" % a for a in alpha)))
    with open(os.path.join(tmp, "qg_parts.h"), "w") as f:
        f.write("static void run_lane_p0(HostArgs &a, uint64_t lane, uint64_t lanes) {\n    QG_LANE_PRELUDE\n#include \"%s\"\n}\n" % os.path.join(tmp, "hand.inc"))
        f.write("static const part_fn PARTS[] = {run_lane_p0};\n")
    exe = {}
    for name, cpp in (("device", ALPHA_CPP), ("fallback", CPP)):
        exe[name] = os.path.join(tmp, "qg_" + name)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fopenmp", "-I", tmp, "-I", os.path.dirname(CPP), "-DQG_PARTS_H=\"qg_parts.h\"",
                               "-DQG_SCALED_H=\"qg_scaled.h\"", "-o", exe[name], cpp])
    N = 2 << LOG_N
    rng = np.random.default_rng(311)
    g3 = oracle.to_mont([3])[0]
    w = oracle.to_mont([pow(3, (P - 1) // N, P)])[0]
    code = g.encode(ins)                                       # the ORIGINAL program: the rewrite is an identity
    for gen in (_rand, _extreme):
        tab = np.concatenate([gen(rng, 1 << k) for k in (0, 1, 3, 5)])
        desc = [0, 0, 1, 1, 3, 3, 11, 5]
        lde = [gen(rng, N) for _ in range(NCOLS)]
        consts = gen(rng, NCONSTS)
        want = oracle.eval_program(code, consts, tab, desc, NSLOTS, lde, LOG_N, 1, g3)
        for name in ("device", "fallback"):
            got = run_host(exe[name], tmp, lde, tab, desc, consts, N, 0, N - 1, 1, 24, g3, w)
            assert np.array_equal(got, want), name


def _build(layout, tmp, cpp, name):
    parts = part_bodies(layout)
    with open(os.path.join(tmp, "qg_parts.h"), "w") as f:
        for j, inc in enumerate(parts):
            f.write("static void run_lane_p%d(HostArgs &a, uint64_t lane, uint64_t lanes) {\n    QG_LANE_PRELUDE\n#include \"%s\"\n}\n" % (j, inc))
        f.write("static const part_fn PARTS[] = {%s};\n" % ", ".join("run_lane_p%d" % j for j in range(len(parts))))
    scaled = os.path.join(ROOT, "sandstorm_amd", "csrc", "quotient_gen_%s_scaled.inc" % layout)
    exe = os.path.join(tmp, "qg_%s_%s" % (name, layout))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fopenmp", "-I", tmp, "-I", os.path.dirname(CPP), "-DQG_PARTS_H=\"qg_parts.h\"",
                           "-DQG_SCALED_H=\"%s\"" % scaled, "-o", exe, cpp])
    return exe


@pytest.mark.parametrize("layout,log_n", [("recursive", 14), ("starknet", 16)])
def test_committed_bodies_device_definition_against_the_fallback(oracle, layout, log_n, tmp_path):
    tmp = str(tmp_path)
    copies = alpha_copies(layout)
    assert len(copies) >= 50, "the committed kernels of %s read no alpha copies" % layout
    assert any("QG_TABLE_ALPHA_RAW(" in open(p).read() for p in part_bodies(layout))
    lay, code, consts, n_slots, specs = program(oracle, layout, log_n)
    device, fallback = _build(layout, tmp, ALPHA_CPP, "device"), _build(layout, tmp, CPP, "fallback")
    n, N = 1 << log_n, 2 << log_n
    tables = lay.Tables(n)
    rng = np.random.default_rng(41)
    tabs, desc, off = [], [], 0
    for spec in specs:
        t = _rand(rng, tables.length(spec))
        desc += [off, len(t).bit_length() - 1]
        off += len(t)
        tabs.append(t)
    tab = np.concatenate(tabs)
    longest = max(1 << desc[2 * t + 1] for t, _, _ in copies)
    assert longest <= N // 2
    lde = [_rand(rng, N) for _ in range(10)]
    consts = np.array(consts, dtype=np.uint64).reshape(-1, 4).copy()
    consts[[c for _, c, _ in copies[::3]]] = _extreme(rng, len(copies[::3]))          # a third of the coefficients at the limb forms' edges
    g3 = oracle.to_mont([3])[0]
    w = oracle.to_mont([pow(3, (P - 1) // N, P)])[0]
    whole = run_host(fallback, tmp, lde, tab, desc, consts, N, 0, N - 1, 1, 96, g3, w)
    assert np.array_equal(run_host(device, tmp, lde, tab, desc, consts, N, 0, N - 1, 1, 96, g3, w), whole)
    assert np.array_equal(whole, oracle.eval_program(code, consts, tab, desc, n_slots, lde, log_n, 1, g3))
    # a row block whose first row is no multiple of the longest period
    B = N // 8
    row0 = 5 * B + 37
    assert row0 % longest != 0
    halo = max((int(c) & 0xffffff) for c in code[1::2][(code[0::2] >> 12) & 0xf == 3]) << 1
    idx = (row0 + np.arange(B + halo)) % N
    block = run_host(device, tmp, [c[idx] for c in lde], tab, desc, consts, B, row0, 0xffffffff, 1, 64, g3, w)
    assert np.array_equal(block, whole[(row0 + np.arange(B)) % N])


def test_the_factor_and_the_entries_against_integers(oracle, tmp_path):
    """qg_alpha_factor and qg_copy_entry (what the device's copy kernel runs per lane) against Python integers: tables of 1, 2 and 32
    entries, every form, constants and entries at 0, 1 and p - 1"""
    tmp = str(tmp_path)
    R = 1 << 256
    edge = [0, 1, P - 1, 2, (P - 1) // 2, pow(5, 77, P)]
    lens = [1, 2, 32]
    rng = np.random.default_rng(5)
    table = [edge[k % len(edge)] if k < 12 else int.from_bytes(rng.bytes(40), "little") % P for k in range(sum(lens))]
    src = os.path.join(tmp, "copy.cpp")
    with open(src, "w") as f:
        f.write('#include <cstdio>\n#include <vector>\n#include "%s/sandstorm_amd/csrc/fp252.h"\n#include "%s/sandstorm_amd/csrc/quotient_derive.h"\n' % (ROOT, ROOT)
                + "using namespace ss;\nint main(int argc, char **argv) {\n    FILE *f = fopen(argv[1], \"rb\");\n    uint32_t hdr[3];\n"
                "    if (fread(hdr, 4, 3, f) != 3) return 2;\n    std::vector<Fp> tab(hdr[0]), cs(hdr[1]);\n    std::vector<uint32_t> d(4 * hdr[2]);\n"
                "    if (fread(tab.data(), 32, tab.size(), f) != tab.size() || fread(cs.data(), 32, cs.size(), f) != cs.size() || fread(d.data(), 4, d.size(), f) != d.size()) return 2;\n"
                "    std::vector<QgCopy> copies; uint32_t total = 0;\n"
                "    for (uint32_t j = 0; j < hdr[2]; ++j) { QgCopy c = {}; c.src = d[4 * j]; c.len = d[4 * j + 1]; c.dst = total; total += c.len;\n"
                "        c.factor = qg_alpha_factor(cs[d[4 * j + 2]], d[4 * j + 3]); copies.push_back(c); }\n"
                "    std::vector<Fp> out(total);\n    for (uint32_t i = 0; i < total; ++i) if (!qg_copy_entry(copies.data(), hdr[2], i, [&tab](uint32_t k) { return tab.at(k); }, &out[i])) return 3;\n"
                "    Fp x; if (qg_copy_entry(copies.data(), hdr[2], total, [&tab](uint32_t k) { return tab.at(k); }, &x)) return 4;\n"
                "    f = fopen(argv[2], \"wb\"); fwrite(out.data(), 32, out.size(), f); fclose(f); return 0;\n}\n")
    exe = os.path.join(tmp, "copy")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src])
    felts = lambda vs: np.array([[(v >> (64 * k)) & ((1 << 64) - 1) for k in range(4)] for v in vs], dtype=np.uint64)
    copies, first = [], 0
    for length in lens:
        for c in range(len(edge)):
            for form in range(3):
                copies.append((first, length, c, form))
        first += length
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        f.write(np.array([len(table), len(edge), len(copies)], dtype=np.uint32).tobytes())
        f.write(felts([v * R % P for v in table]).tobytes())
        f.write(felts([v * R % P for v in edge]).tobytes())
        f.write(np.array(copies, dtype=np.uint32).tobytes())
    subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")])
    got = np.fromfile(os.path.join(tmp, "out.bin"), dtype=np.uint64).reshape(-1, 4)
    want = []
    for first, length, c, form in copies:
        factor = edge[c] * (1 << 24) * ((1 << 24) if form else 1) * (-1 if form == 2 else 1)
        want += [table[first + k] * factor % P * R % P for k in range(length)]
    assert np.array_equal(got, felts(want))
