"""The two cuts of tools/gen_quotient.py that remove work a point does not need - a multiplication by a small structural integer
written as fl_scale shifts and adds, and two consecutive operands that name one cell read by one load - checked without a GPU:

  * on a hand-made program that holds "MOV T; ADD T" and multiplications by 2, 6, 10, 16, -2 and 2^8 in both operand forms, plain
    and inside a constraint's wide sum: the emitted body holds the scalings and the single loads where it should, keeps 2^8 and a
    constant that is not structural as products, and - compiled for the host with the device's definitions of the scaling macros
    (tests/cpp/quotient_gen_baked_host_test.cpp) - equals the oracle's constraint VM on columns from the limb forms' edges;
  * the same bodies under the other harness, which does not define the macros, with the "small" constants REPLACED: the products by
    the table's constants (what lets a harness choose its own constants; the device checks the table instead);
  * structural_constants: a constant that is small in one dump only, or that is never a multiplier, is not baked;
  * the committed bodies of both layouts with the device's macros, on edge values, against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_quotient_gen_host import CPP, ROOT, _extreme, part_bodies, program, run_host
from tests.test_layout_starknet import P

sys.path.insert(0, os.path.join(ROOT, "tools"))
BAKED_CPP = os.path.join(ROOT, "tests", "cpp", "quotient_gen_baked_host_test.cpp")

OP_MOV, OP_ADD, OP_SUB, OP_RSUB, OP_MUL, OP_INV, OP_ST, OP_OUT = range(8)
ACC, SLOT, CONST, TRACE, TABLE, X = range(6)
NCOLS, NCONSTS, NTABLES, NSLOTS, LOG_N = 6, 20, 1, 2, 6
SMALL = {0: 2, 1: 6, 2: 10, 3: 16, 4: -2, 5: 256}          # constant index -> its structural value
RUNTIME_SMALL = 6                                          # a constant whose value is 4 here, but not by the layout's structure
T = lambda col, off: (TRACE, (col << 24) | off)


def hand_made():
    """sum_k alpha_k C_k times a table, the C_k holding the forms the layouts' constraints have"""
    ins, alpha = [], [10]

    def e(op, d, kind=0, w1=0):
        ins.append((op, d, kind, w1))

    def close(first=False):
        e(OP_MUL, 2, CONST, alpha[0])
        alpha[0] += 1
        e(OP_MOV if first else OP_ADD, 1, ACC, 2)
    e(OP_MOV, 2, *T(0, 0)); e(OP_ADD, 2, *T(0, 0)); e(OP_MUL, 2, CONST, 0); close(True)             # (x + x) * 2: one load, MUL acc, c
    e(OP_MOV, 2, CONST, 1); e(OP_MUL, 2, *T(1, 1)); e(OP_SUB, 2, *T(2, 0)); close()                # 6 * x - y: MOV acc, c; MUL acc, x
    e(OP_MOV, 2, *T(3, 0)); e(OP_SUB, 2, *T(4, 0)); e(OP_MUL, 2, CONST, 2); close()                # (x - y) * 10 on a lazy value
    e(OP_MOV, 2, *T(3, 2)); e(OP_MUL, 2, CONST, 3); e(OP_ADD, 2, *T(1, 0)); close()                # x * 16 + y
    e(OP_MOV, 2, *T(0, 3)); e(OP_ADD, 2, *T(0, 3)); e(OP_MUL, 2, CONST, 4); e(OP_RSUB, 2, *T(2, 2)); close()    # y - (x + x) * -2
    e(OP_MOV, 2, *T(5, 0)); e(OP_SUB, 2, *T(5, 2)); e(OP_MUL, 2, CONST, 5); close()                # (x - y) * 2^8
    e(OP_MOV, 2, *T(5, 1)); e(OP_MUL, 2, CONST, RUNTIME_SMALL); close()                           # x * (a runtime 4)
    e(OP_MOV, 2, *T(0, 0)); e(OP_MUL, 2, *T(1, 0))                                                 # x y + 6 z - (w + w) * 2: a wide sum,
    e(OP_MOV, 3, CONST, 1); e(OP_MUL, 3, *T(2, 1)); e(OP_ADD, 2, ACC, 3)                           # the multiples in its linear part
    e(OP_MOV, 3, *T(4, 1)); e(OP_ADD, 3, *T(4, 1)); e(OP_MUL, 3, CONST, 0); e(OP_SUB, 2, ACC, 3); close()
    e(OP_MOV, 3, *T(3, 1)); e(OP_ADD, 3, *T(3, 1)); e(OP_ST, 3, 0, 0)                              # a doubled cell parked in a slot
    e(OP_MOV, 2, SLOT, 0); e(OP_MUL, 2, ACC, 2); e(OP_SUB, 2, SLOT, 0); close()
    e(OP_MUL, 1, TABLE, 0); e(OP_MOV, 0, ACC, 1); e(OP_OUT, 0)
    return ins


def mont(oracle, v):
    return oracle.to_mont([v % P])[0]


def as_int(words):
    return sum(int(w) << (64 * k) for k, w in enumerate(words))


KNOBS = [(True, True, True, True, 1, 3), (True, True, False, False, 1, 2), (False, False, False, False, 1, 2), (True, False, True, True, 1, 1)]


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "fuse%d-wide%d-lazy%d-cf%d-min%d-d%d" % tuple(int(x) for x in k))
def test_hand_made_program(oracle, knobs, tmp_path, monkeypatch):
    import gen_quotient
    fuse, wide, lazy_sub, const_factor, min_terms, depth = knobs
    tmp = str(tmp_path)
    monkeypatch.setattr(gen_quotient, "OUT_DIR", tmp)
    ins = hand_made()
    rng = np.random.default_rng(77)
    consts = _extreme(rng, NCONSTS)
    for k, c in SMALL.items():
        consts[k] = mont(oracle, c)
    consts[RUNTIME_SMALL] = mont(oracle, 4)
    small = {k: (c, as_int(consts[k])) for k, c in SMALL.items()}
    plain = gen_quotient.generate_body("hand", ins, NCONSTS, NSLOTS, NTABLES, NCOLS, depth, "plain.inc", fuse, "QG_OUT", 0, wide, lazy_sub, const_factor, min_terms, [])
    stats = gen_quotient.generate_body("hand", ins, NCONSTS, NSLOTS, NTABLES, NCOLS, depth, "hand.inc", fuse, "QG_OUT", 0, wide, lazy_sub, const_factor, min_terms, [],
                                       small=small, dedup=True)
    with open(os.path.join(tmp, "hand.inc")) as f:
        body = f.read()
    with open(os.path.join(tmp, "plain.inc")) as f:
        plain_body = f.read()
    assert "QG_SCALE" not in plain_body and plain["baked"] == {}
    # ---- the scalings: 2 and 6 in one step, 10 = 5 x 2 and 16 = 8 x 2 with a weak reduction between, -2 with its negation
    assert stats["baked"] == {0: 2, 1: 2, 2: 1, 3: 1, 4: 1}, stats["baked"]
    assert body.count("QG_SCALE(0, 2, ") == 2 and body.count("QG_SCALE(1, 6, fl_from_fp(") == 2
    assert "QG_SCALE(2, 5, acc2);\n    acc2 = fl_weak_reduce(acc2);\n    acc2 = QG_RESCALE(2, acc2);" in body
    assert "QG_SCALE(3, 8, acc2);\n    acc2 = fl_weak_reduce(acc2);\n    acc2 = QG_RESCALE(2, acc2);" in body
    assert "QG_SCALE(4, 2, acc2);\n    acc2 = QG_NEGSCALED(16, 4, acc2);" in body            # (x + x: bound 2, doubled: 4)
    # ---- 2^8 of a lazy value stays a product (three scalings and three weak reductions are no cheaper), and so does the constant
    #      nobody vouched for
    assert "QG_SCALE(5," not in body and "QG_CONST_R280(5)" in body
    assert "QG_SCALE(%d," % RUNTIME_SMALL not in body and "QG_CONST_R280(%d)" % RUNTIME_SMALL in body
    # ---- one load per "MOV T; ADD T": four pairs in the program
    assert stats["loads"] == plain["loads"] - 4
    for cell in ("QG_TRACE_RAW(0, 3u, ", "QG_TRACE_RAW(4, 1u, ", "QG_TRACE_RAW(3, 1u, "):
        assert body.count(cell) == 1 and plain_body.count(cell) == 2
    # (cell (0, 0) opens the program: its loads are also the ones primed in front of the loop and issued across the loop edge)
    assert body.count("QG_TRACE_RAW(0, 0u, ") < plain_body.count("QG_TRACE_RAW(0, 0u, ")
    # ---- and the value: the device's shifts and adds against the oracle's constraint VM
    with open(os.path.join(tmp, "qg_scaled.h"), "w") as f:
        f.write("static const uint32_t QG_N_TABLES = %du, QG_N_SCALED = 0u;\nstatic const uint32_t QG_SCALED_TABLES[] = {0u};\n" % NTABLES)
    with open(os.path.join(tmp, "qg_parts.h"), "w") as f:
        f.write("static void run_lane_p0(HostArgs &a, uint64_t lane, uint64_t lanes) {\n    QG_LANE_PRELUDE\n#include \"%s\"\n}\n" % os.path.join(tmp, "hand.inc"))
        f.write("static const part_fn PARTS[] = {run_lane_p0};\n")
    n, N = 1 << LOG_N, 2 << LOG_N
    tab, desc = _extreme(rng, 8), [0, 3]
    lde = [_extreme(rng, N) for _ in range(NCOLS)]
    g = oracle.to_mont([3])[0]
    w = oracle.to_mont([pow(3, (P - 1) // N, P)])[0]
    code = gen_quotient.encode(ins)
    exe = {}
    for name, cpp in (("baked", BAKED_CPP), ("fallback", CPP)):
        exe[name] = os.path.join(tmp, "qg_" + name)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fopenmp", "-I", tmp, "-I", os.path.dirname(CPP), "-DQG_PARTS_H=\"qg_parts.h\"",
                               "-DQG_SCALED_H=\"qg_scaled.h\"", "-o", exe[name], cpp])
    want = oracle.eval_program(code, consts, tab, desc, NSLOTS, lde, LOG_N, 1, g)
    for name in ("baked", "fallback"):
        got = run_host(exe[name], tmp, lde, tab, desc, consts, N, 0, N - 1, 1, 24, g, w)
        assert np.array_equal(got, want), name
    # the fallback is the product by whatever the table holds: the "small" constants replaced by edge values
    other = consts.copy()
    other[:len(SMALL)] = _extreme(rng, len(SMALL))
    want = oracle.eval_program(code, other, tab, desc, NSLOTS, lde, LOG_N, 1, g)
    got = run_host(exe["fallback"], tmp, lde, tab, desc, other, N, 0, N - 1, 1, 24, g, w)
    assert np.array_equal(got, want)


def test_only_structural_constants_are_baked(oracle):
    import gen_quotient
    ins = hand_made() [:-1] + [(OP_SUB, 0, CONST, 19), (OP_OUT, 0, 0, 0)]
    consts = [[0, 0, 0, 0] for _ in range(NCONSTS)]
    for k, c in SMALL.items():
        consts[k] = list(mont(oracle, c))
    consts[RUNTIME_SMALL] = list(mont(oracle, 4))             # small in this dump ...
    consts[19] = list(mont(oracle, 2))                        # small in both, but subtracted: never a multiplier
    for k in range(10, 19):
        consts[k] = list(mont(oracle, 3))                     # a composition coefficient that happens to be small here
    consts2 = [list(c) for c in consts]
    consts2[RUNTIME_SMALL] = list(mont(oracle, 12345678901234567890))     # ... and not in the other
    for k in range(10, 19):
        consts2[k] = list(mont(oracle, pow(5, 77 + k, P)))
    got = gen_quotient.structural_constants(ins, consts, consts2)
    assert {k: c for k, (c, _) in got.items()} == SMALL
    assert all(image == as_int(consts[k]) for k, (_, image) in got.items())
    # the cost model: what scale_plan prices below a product and what not
    assert gen_quotient.scale_plan(6, 1) == ([6], 18, 6)
    assert gen_quotient.scale_plan(10, 2) == ([4, "R", 5, "R", 2], 9 + 54 + 9 + 54 + 9, 2) or gen_quotient.scale_plan(10, 2)[1] < gen_quotient.PRODUCT_COST
    assert gen_quotient.scale_plan(256, 1)[1] + 54 >= gen_quotient.WIDE_TERM_COST and gen_quotient.scale_plan(11, 1) is None


def baked_constants(layout):
    """(constant index, image) pairs of the committed kernel table (csrc/quotient_gen_<layout>.hip)"""
    import re
    with open(os.path.join(ROOT, "sandstorm_amd", "csrc", "quotient_gen_%s.hip" % layout)) as f:
        text = f.read()
    listed = re.search(r"QGenBaked baked\[\] = \{(.*)\};", text).group(1)
    return [(int(k), sum(int(w, 16) << (64 * j) for j, w in enumerate(ws.replace("ull", "").split(", "))))
            for k, ws in re.findall(r"\{(\d+)u, \{([^}]*)\}\}", listed)]


@pytest.mark.parametrize("layout,log_n", [("recursive", 14), ("starknet", 16)])
def test_committed_bodies_with_the_devices_scalings(oracle, layout, log_n, tmp_path):
    """tests/test_quotient_gen_host.py runs the committed bodies with the scaling macros undefined (products); here they are the
    device's, on columns, tables and (other) constants from the limb forms' edges, so that scaled values reach their bounds"""
    tmp = str(tmp_path)
    lay, code, consts, n_slots, specs = program(oracle, layout, log_n)
    baked = baked_constants(layout)
    assert baked, "no small multiple in the committed kernels of %s" % layout
    consts = np.array(consts, dtype=np.uint64).reshape(-1, 4).copy()
    for k, image in baked:                                      # the list the launch checks is what this program's table holds
        assert as_int(consts[k]) == image
    parts = part_bodies(layout)
    assert any("QG_SCALE(" in open(p).read() for p in parts)
    with open(os.path.join(tmp, "qg_parts.h"), "w") as f:
        for j, inc in enumerate(parts):
            f.write("static void run_lane_p%d(HostArgs &a, uint64_t lane, uint64_t lanes) {\n    QG_LANE_PRELUDE\n#include \"%s\"\n}\n" % (j, inc))
        f.write("static const part_fn PARTS[] = {%s};\n" % ", ".join("run_lane_p%d" % j for j in range(len(parts))))
    scaled = os.path.join(ROOT, "sandstorm_amd", "csrc", "quotient_gen_%s_scaled.inc" % layout)
    exe = os.path.join(tmp, "qg_baked_%s" % layout)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fopenmp", "-I", tmp, "-I", os.path.dirname(CPP), "-DQG_PARTS_H=\"qg_parts.h\"",
                           "-DQG_SCALED_H=\"%s\"" % scaled, "-o", exe, BAKED_CPP])
    n, N = 1 << log_n, 2 << log_n
    tables = lay.Tables(n)
    rng = np.random.default_rng(31)
    tabs, desc, off = [], [], 0
    for spec in specs:
        t = _extreme(rng, tables.length(spec))
        desc += [off, len(t).bit_length() - 1]
        off += len(t)
        tabs.append(t)
    tab = np.concatenate(tabs)
    lde = [_extreme(rng, N) for _ in range(10)]
    edge = _extreme(rng, len(consts))
    pick = rng.random(len(consts)) < 0.5
    pick[[k for k, _ in baked]] = False
    consts[pick] = edge[pick]
    g = oracle.to_mont([3])[0]
    w = oracle.to_mont([pow(3, (P - 1) // N, P)])[0]
    want = oracle.eval_program(code, consts, tab, desc, n_slots, lde, log_n, 1, g)
    got = run_host(exe, tmp, lde, tab, desc, consts, N, 0, N - 1, 1, 96, g, w)
    assert np.array_equal(got, want)
