"""The plain AIR over the 64-bit field lowered by the C++ host (sandstorm_amd/host/air_plain.cpp) and the C++ verifier of that claim
(host/goldilocks_verifier.cpp), without a device: hostlib.GlPlainAir(None, pi) is a host-only handle.

  1  the composition program is air_program.lower(layouts.plain.composition(...), ext=True)'s: code words, constants by value and
     order, slots, table descriptions and table values - at n = 2^8, 2^11 and 2^24, for the example and the busy program, and for
     statements and challenges chosen so that values collide (a program that interned a constant by value would differ); the FNV-1a
     hash of the code is the compiled kernel's (tools/gen_quotient_gl.py), so the compiled plain kernel runs, not the interpreter
  2  mask, statement digest and transcript seed are Python's; the check program's domains and names are layouts.plain.check_program's
  3  hostlib.gl_verify accepts the MI355X-made fixture with goldilocks.verify's positions, and refuses every tampered copy with the
     words goldilocks.verify refuses it with
  4  cut and garbled blobs are refused, none crashes - here through the library, and in tests/cpp/gl_verify_blob_test.cpp as a
     program of its own under the address and undefined-behaviour sanitizers"""
import copy
import dataclasses
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sandstorm_amd import air_program as ap  # noqa: E402
from sandstorm_amd import goldilocks as gs  # noqa: E402
from sandstorm_amd.layouts import plain as pl  # noqa: E402
from test_device_code_on_host import CLANG  # noqa: E402

P = pl.P
SEED = bytes(range(32))
GENERIC = ([(11, 22, 33), (5, 6, 7), (9, 8, 7)], (123, 456, 789))


@pytest.fixture(scope="module")
def hostlib():
    from sandstorm_amd import hostlib as h
    h.load()
    return h


def statement(program, cycles):
    states, memory = pl.run(program, cycles)
    return pl.public_input_of(program, states, memory)


@pytest.fixture(scope="module")
def statements():
    from tests import gl64_programs
    return {"example": statement(pl.example_program(10), 16), "busy": statement(gl64_programs.busy_program(), 128)}


def python_program(pi, challenges, alpha):
    n = pl.CYCLE_HEIGHT * pi.n_steps
    tables = pl.Tables(n, 1)
    root = pl.composition(n, pl.Hints.from_public_input(pi, challenges, n), challenges, alpha, tables)
    prog = ap.lower(root, P, ext=True, symbols=tables.symbols)
    values, desc = tables.device_tables()
    return prog, values, desc


def assert_same_program(hostlib, pi, challenges, alpha, what):
    import gen_quotient_gl as g
    air = hostlib.GlPlainAir(None, pi)
    got = air.program(challenges, alpha)
    prog, values, desc = python_program(pi, challenges, alpha)
    assert np.array_equal(got["code"], np.array(prog.code, dtype=np.uint32)), (what, "code words")
    assert np.array_equal(got["consts"], np.array(prog.consts, dtype=np.uint64).reshape(-1, 3)), (what, "constants")
    assert got["n_slots"] == prog.n_slots, (what, "slots")
    assert got["table_desc"] == [int(v) for v in desc], (what, "table descriptions")
    assert got["d_tables"] == 0 and np.array_equal(got["tables"], values), (what, "table values")
    assert g.code_hash(got["code"]) == g.code_hash(g.template_program()[0]), (what, "the compiled kernel's hash")
    air.close()


# ------------------------------------------------------------------------------------------------------ 1. the composition program
@pytest.mark.parametrize("name,log_steps", [("example", 4), ("example", 7), ("example", 20), ("busy", 7), ("busy", 20)])
def test_composition_program_is_the_python_lowering_word_for_word(hostlib, statements, name, log_steps):
    """n = 2^8, 2^11, 2^24: the statement of the run with its step count replaced (the program depends on the statement and n only).
    The busy program's 72 public-memory words do not fit the 32 cells of a 2^8-row trace: that statement has no memory quotient (the
    handle says so, in base_trace's words), so the busy program is lowered from 2^11 up"""
    pi = dataclasses.replace(statements[name], n_steps=1 << log_steps)
    assert_same_program(hostlib, pi, *GENERIC, what=(name, log_steps))


def test_public_memory_that_does_not_fit_is_refused_in_the_trace_generators_words(hostlib, statements):
    from sandstorm_amd._lib import SandstormHipError
    pi = dataclasses.replace(statements["busy"], n_steps=16)
    assert len(pi.public_memory) > 16 * pi.n_steps // pl.PUBLIC_MEMORY_STEP
    with pytest.raises(SandstormHipError, match="public memory does not fit"):
        hostlib.GlPlainAir(None, pi).program(*GENERIC)


COLLISIONS = {
    "two equal challenges": ([(11, 22, 33), (11, 22, 33), (9, 8, 7)], (123, 456, 789)),
    "challenges (1, 0, 0) and (2, 0, 0)": ([(1, 0, 0), (2, 0, 0), (9, 8, 7)], (123, 456, 789)),
    "every challenge (1, 0, 0)": ([(1, 0, 0), (1, 0, 0), (1, 0, 0)], (4, 0, 0)),
    "alpha = (1, 0, 0)": ([(11, 22, 33), (5, 6, 7), (9, 8, 7)], (1, 0, 0)),
    "alpha = (0, 1, 0), a challenge (0, 0, 1)": ([(0, 0, 1), (5, 6, 7), (65536, 0, 0)], (0, 1, 0)),
}


@pytest.mark.parametrize("case", sorted(COLLISIONS))
def test_colliding_challenges_leave_the_program_as_it_is(hostlib, statements, case):
    assert_same_program(hostlib, dataclasses.replace(statements["example"], n_steps=128), *COLLISIONS[case], what=case)


def test_colliding_hints_leave_the_program_as_it_is(hostlib, statements):
    """rc_min == rc_max, initial_ap == initial_pc, hints equal to the AIR's structural constants 1, 2, 4, 2^15 and 2^16"""
    pi = statements["example"]
    prog, exe = pi.memory_segments["program"], pi.memory_segments["execution"]
    cases = {"rc_min == rc_max": dataclasses.replace(pi, rc_min=pi.rc_max),
             "rc bounds 2^15 and 2^16 - 1": dataclasses.replace(pi, rc_min=1 << 15, rc_max=(1 << 16) - 1),
             "initial_ap == initial_pc": dataclasses.replace(pi, memory_segments={"program": prog, "execution": (prog[0], exe[1])}),
             "final_ap == final_pc == 2": dataclasses.replace(pi, memory_segments={"program": (prog[0], 2), "execution": (exe[0], 2)}),
             "segments 4 and 65536": dataclasses.replace(pi, memory_segments={"program": (4, 65536), "execution": (65536, 4)})}
    for what, st in cases.items():
        for log_steps in (4, 7):
            assert_same_program(hostlib, dataclasses.replace(st, n_steps=1 << log_steps), *GENERIC, what=what)
            assert_same_program(hostlib, dataclasses.replace(st, n_steps=1 << log_steps), *COLLISIONS["every challenge (1, 0, 0)"], what=what)


def test_two_programs_from_one_handle_differ_in_their_constants_only(hostlib, statements):
    air = hostlib.GlPlainAir(None, statements["busy"])
    a, b = air.program(*GENERIC), air.program([(1, 2, 3), (4, 5, 6), (7, 8, 9)], (10, 11, 12))
    assert np.array_equal(a["code"], b["code"]) and a["table_desc"] == b["table_desc"] and np.array_equal(a["tables"], b["tables"])
    assert not np.array_equal(a["consts"], b["consts"])
    again = air.program(*GENERIC)
    assert np.array_equal(a["consts"], again["consts"])


# ------------------------------------------------------------------------------------------------------ 2. mask, digest, seed, checks
def test_mask_statement_digest_and_transcript_seed_are_pythons(hostlib, statements):
    for name, pi in statements.items():
        air = hostlib.GlPlainAir(None, pi)
        assert air.mask == pl.mask(), name
        assert air.statement_digest() == gs.statement_digest(pi), name
        for opt in (gs.Options(), gs.Options(num_queries=8, log_blowup=2, grinding=4, fold=2, max_remainder=4, hash="sha256")):
            assert air.transcript_seed(SEED, opt) == gs.transcript_seed(SEED, opt, 16 * pi.n_steps, pi), (name, opt)


def test_check_program_has_pythons_domains_and_names_and_vanishes_where_pythons_does(hostlib, statements):
    """the check program need not be word-identical: its domains and names are layouts.plain.check_program's, it holds one CHECK per
    constraint in order, and - run by a small interpreter of the VM over the rows of each domain - it vanishes on the example's trace and
    fails exactly where the numerators do on a broken one"""
    prog = pl.example_program(10)
    states, memory = pl.run(prog, 16)
    pi = pl.public_input_of(prog, states, memory)
    challenges = GENERIC[0]
    n = 16 * pi.n_steps
    _, domains, names, domain_names = pl.check_program(n, pl.Hints.from_public_input(pi, challenges, n), challenges)
    got = hostlib.GlPlainAir(None, pi).check_program(challenges)
    assert got["names"] == names and got["domain_names"] == domain_names
    assert got["domains"] == [([tuple(f) for f in num], [tuple(f) for f in den]) for num, den in domains]
    code = [int(w) for w in got["code"]]
    assert [code[i + 1] for i in range(0, len(code), 2) if code[i] & 0xff == ap.OP.CHECK] == list(range(len(names)))
    cols = pl.base_trace(states, memory, pi)
    ext, _ = pl.extension_columns(cols, challenges)
    cols8 = [list(c) for c in cols] + ext
    consts = [tuple(int(v) for v in c) for c in got["consts"]]

    def failing(cols8):
        """the constraints whose numerator the C++ host's check program leaves non-zero on a row of its domain"""
        bad = set()
        rows_of = [list(c.domain.rows(n)) for c in pl.constraints(pl.Hints.from_public_input(pi, challenges, n), challenges)]
        for r in sorted({r for rows in rows_of for r in rows}):
            acc, slots = [(0, 0, 0)] * 4, {}
            for i in range(0, len(code), 2):
                op, dst, kind, payload = code[i] & 0xff, (code[i] >> 8) & 0xf, code[i] >> 12, code[i + 1]
                if op == ap.OP.CHECK:
                    if r in rows_of[payload] and any(acc[dst]):
                        bad.add(payload)
                    continue
                if op == ap.OP.ST:
                    slots[payload] = acc[dst]
                    continue
                if op == ap.OP.INV:
                    acc[dst] = pl.inv3(acc[dst])
                    continue
                v = (acc[payload] if kind == ap.SRC.ACC else slots[payload] if kind == ap.SRC.SLOT else consts[payload] if kind == ap.SRC.CONST
                     else (cols8[payload >> 24][(r + (payload & 0xffffff)) % n], 0, 0))
                assert kind in (ap.SRC.ACC, ap.SRC.SLOT, ap.SRC.CONST, ap.SRC.TRACE)
                acc[dst] = (v if op == ap.OP.MOV else pl.add3(acc[dst], v) if op == ap.OP.ADD else pl.sub3(acc[dst], v) if op == ap.OP.SUB
                            else pl.sub3(v, acc[dst]) if op == ap.OP.RSUB else pl.mul3(acc[dst], v))
        return bad
    assert failing(cols8) == set()
    broken = [list(c) for c in cols8]
    broken[pl.COL_NPC][16 * 3 + pl.Npc.MEM_DST] = (broken[pl.COL_NPC][16 * 3 + pl.Npc.MEM_DST] + 1) % P
    want = {k for k, c in enumerate(pl.constraints(pl.Hints.from_public_input(pi, challenges, n), challenges)) if pl.failing_rows(c, broken, n, limit=1)}
    assert want and failing(broken) == want


# ------------------------------------------------------------------------------------------------------ 3. the verifier
@pytest.fixture(scope="module")
def fixture_proof():
    prog = pl.example_program(10)
    states, memory = pl.run(prog, 64)
    pi = pl.public_input_of(prog, states, memory)
    with np.load(os.path.join(ROOT, "tests", "golden", "goldilocks_plain_proof.npz")) as f:
        arrays = {k: f[k] for k in f.files}
    return pi, arrays


BITS = 28                # what the fixture's 20 queries and 8 grinding bits conjecture


def both_refuse(hostlib, air, pi, proof, bits=BITS):
    """-> the check goldilocks.verify names; hostlib.gl_verify must name the same one"""
    from sandstorm_amd._lib import SandstormHipError
    with pytest.raises(gs.VerificationError) as py:
        gs.verify(proof, gs.plain_air(), SEED, statement=pi, required_security_bits=bits)
    with pytest.raises(SandstormHipError) as cpp:
        hostlib.gl_verify(air, proof, SEED, bits)
    assert str(cpp.value) == "host: " + str(py.value)
    return str(py.value)


def test_cpp_verifier_accepts_the_gpu_made_proof_with_pythons_positions(hostlib, fixture_proof):
    pi, arrays = fixture_proof
    proof = gs.proof_from_arrays(arrays)
    air = hostlib.GlPlainAir(None, pi)
    want = gs.verify(proof, gs.plain_air(), SEED, statement=pi, required_security_bits=BITS)
    assert hostlib.gl_verify(air, proof, SEED, BITS) == want and len(want) >= 15
    assert "bits of security, 80 required" in both_refuse(hostlib, air, pi, proof, bits=80)
    assert "28 bits of security, 29 required" in both_refuse(hostlib, air, pi, proof, bits=29)
    other = copy.deepcopy(pi)
    other.memory_segments["execution"] = (other.memory_segments["execution"][0], other.memory_segments["execution"][1] + 1)
    from sandstorm_amd._lib import SandstormHipError
    with pytest.raises(SandstormHipError, match="do not satisfy the AIR"):
        hostlib.gl_verify(hostlib.GlPlainAir(None, other), proof, SEED, BITS)
    with pytest.raises(SandstormHipError, match="trace length: the proof's is 1024, the AIR handle was made for 256"):
        hostlib.gl_verify(hostlib.GlPlainAir(None, dataclasses.replace(pi, n_steps=16)), proof, SEED, BITS)


def flip(array, index):
    array[index] = int(array[index]) ^ 1


def bump(array, index):
    array[index] = (int(array[index]) + 1) % P


AIR_IDENTITY = "the out-of-domain values do not satisfy the AIR"
PATH = ": authentication path does not reach the root"
TAMPERINGS = {
    "base root": (lambda p: setattr(p, "base_root", bytes([p.base_root[0] ^ 1]) + p.base_root[1:]), AIR_IDENTITY),
    "extension root": (lambda p: setattr(p, "ext_root", bytes([p.ext_root[0] ^ 1]) + p.ext_root[1:]), AIR_IDENTITY),
    "composition root": (lambda p: setattr(p, "comp_root", p.comp_root[:31] + bytes([p.comp_root[31] ^ 0x80])), AIR_IDENTITY),
    "out-of-domain trace value": (lambda p: bump(p.ood_trace, (7, 1)), AIR_IDENTITY),
    "out-of-domain composition value": (lambda p: bump(p.ood_comp, (5, 2)), AIR_IDENTITY),
    "out-of-domain value = p": (lambda p: p.ood_trace.__setitem__((0, 0), P), "out-of-domain values: range"),
    "base row": (lambda p: flip(p.base.rows, (3, 2)), "base trace" + PATH),
    "extension row": (lambda p: flip(p.ext.rows, (0, 1)), "extension trace" + PATH),
    "composition row": (lambda p: flip(p.comp.rows, (p.comp.rows.shape[0] - 1, 5)), "composition trace" + PATH),
    "FRI layer 0 row": (lambda p: flip(p.fri_layers[0].opening.rows, (1, 4)), "FRI layer 0" + PATH),
    "last FRI layer row": (lambda p: flip(p.fri_layers[-1].opening.rows, (0, 0)), "FRI layer %d" + PATH),
    "base path byte": (lambda p: flip(p.base.paths, (2, 1, 31)), "base trace" + PATH),
    "composition path byte": (lambda p: flip(p.comp.paths, (0, 0, 0)), "composition trace" + PATH),
    "FRI layer 0 path byte": (lambda p: flip(p.fri_layers[0].opening.paths, (0, 0, 0)), "FRI layer 0" + PATH),
    "remainder coefficient above the degree bound": (lambda p: p.remainder.__setitem__((p.remainder.shape[0] >> p.options.log_blowup, 0), 1), "FRI remainder: shape / degree"),
    "remainder coefficient = p": (lambda p: p.remainder.__setitem__((0, 0), P), "FRI remainder: shape / degree"),
    "remainder coefficient": (lambda p: bump(p.remainder, (0, 0)), None),
    "nonce": (lambda p: setattr(p, "pow_nonce", p.pow_nonce + 1), None),
    "num_queries": (lambda p: setattr(p, "options", dataclasses.replace(p.options, num_queries=p.options.num_queries + 1)), AIR_IDENTITY),
    "num_queries 257": (lambda p: setattr(p, "options", dataclasses.replace(p.options, num_queries=257)), "options out of range"),
    "log_blowup 2": (lambda p: setattr(p, "options", dataclasses.replace(p.options, log_blowup=2)), AIR_IDENTITY),
    "log_blowup 5": (lambda p: setattr(p, "options", dataclasses.replace(p.options, log_blowup=5)), "options: log_blowup must be 1, 2, 3 or 4 (LDE blowup 2, 4, 8 or 16), not 5"),
    "grinding": (lambda p: setattr(p, "options", dataclasses.replace(p.options, grinding=p.options.grinding + 1)), AIR_IDENTITY),
    "grinding 41": (lambda p: setattr(p, "options", dataclasses.replace(p.options, grinding=41)), "options out of range"),
    "fold 4": (lambda p: setattr(p, "options", dataclasses.replace(p.options, fold=4)), AIR_IDENTITY),
    "fold 3": (lambda p: setattr(p, "options", dataclasses.replace(p.options, fold=3)), "options out of range"),
    "max_remainder 8": (lambda p: setattr(p, "options", dataclasses.replace(p.options, max_remainder=8)), AIR_IDENTITY),
    "max_remainder 0": (lambda p: setattr(p, "options", dataclasses.replace(p.options, max_remainder=0)), "options out of range"),
    "hash sha256": (lambda p: setattr(p, "options", dataclasses.replace(p.options, hash="sha256")), AIR_IDENTITY),
    "hash md5": (lambda p: setattr(p, "options", dataclasses.replace(p.options, hash="md5")), "options: hash"),
    "a layer's log_len": (lambda p: setattr(p.fri_layers[0], "log_len", p.fri_layers[0].log_len + 1), "FRI layer length"),
    "the last layer's log_len": (lambda p: setattr(p.fri_layers[-1], "log_len", p.fri_layers[-1].log_len - 1), "FRI layer length"),
    "a layer's root": (lambda p: setattr(p.fri_layers[0], "root", bytes(32)), None),
    "a layer dropped": (lambda p: p.fri_layers.pop(), "number of FRI layers"),
    "trace length 1000": (lambda p: setattr(p, "trace_len", 1000), "trace length"),
}


@pytest.mark.parametrize("what", sorted(TAMPERINGS))
def test_both_verifiers_refuse_a_tampered_proof_and_name_the_same_check(hostlib, fixture_proof, what):
    pi, arrays = fixture_proof
    proof = gs.proof_from_arrays(copy.deepcopy(arrays))
    mutate, check = TAMPERINGS[what]
    mutate(proof)
    named = both_refuse(hostlib, hostlib.GlPlainAir(None, pi), pi, proof)
    if check is not None:
        assert named == (check % (len(proof.fri_layers) - 1) if "%d" in check else check), named


def test_trace_length_of_another_handle_is_refused_by_name(hostlib, fixture_proof):
    from sandstorm_amd._lib import SandstormHipError
    pi, arrays = fixture_proof
    proof = gs.proof_from_arrays(copy.deepcopy(arrays))
    proof.trace_len //= 2
    with pytest.raises(SandstormHipError, match="trace length: the proof's is 512, the AIR handle was made for 1024"):
        hostlib.gl_verify(hostlib.GlPlainAir(None, pi), proof, SEED, BITS)


# ------------------------------------------------------------------------------------------------------ 4. malformed blobs
def count_words(blob):
    """the indices of the blob's count words (host_capi.cpp's layout): the layer count, the two value counts, every layer's log length,
    every opening's three"""
    at = [3]
    o = 16
    at.append(o)
    o += 1 + 3 * int(blob[o]) + 18
    at.append(o)
    o += 1 + 3 * int(blob[o])
    n_layers = int(blob[3])
    for _ in range(n_layers):
        at.append(o + 4)
        o += 5
    for _ in range(2 + int(blob[2]) + n_layers):
        npos, width, depth = (int(v) for v in blob[o:o + 3])
        at += [o, o + 1, o + 2]
        o += 3 + npos * width + npos * depth * 4
    assert o == len(blob)
    return at


def test_cut_and_garbled_blobs_are_refused(hostlib, fixture_proof):
    from sandstorm_amd._lib import SandstormHipError
    pi, arrays = fixture_proof
    proof = gs.proof_from_arrays(arrays)
    air = hostlib.GlPlainAir(None, pi)
    blob = hostlib.gl_blob_of_proof(proof)
    want = hostlib.gl_verify_blob(air, proof.options, SEED, blob, BITS)
    assert want == gs.verify(proof, gs.plain_air(), SEED, statement=pi, required_security_bits=BITS)
    rng = np.random.default_rng(0x61A1)
    header = 4 + 12 + 1                                     # the counts, the three roots, the first value count
    cuts = list(range(header + 1)) + sorted(int(v) for v in rng.integers(header + 1, len(blob), size=32))
    for cut in cuts:
        with pytest.raises(SandstormHipError, match="proof blob: "):
            hostlib.gl_verify_blob(air, proof.options, SEED, blob[:cut], BITS)
    for at in count_words(blob):
        for value in (1 << 63, (1 << 64) - 1, int(blob[at]) + 1):
            bad = blob.copy()
            bad[at] = value
            with pytest.raises(SandstormHipError):
                hostlib.gl_verify_blob(air, proof.options, SEED, bad, BITS)
    with pytest.raises(SandstormHipError, match="words left over"):
        hostlib.gl_verify_blob(air, proof.options, SEED, np.concatenate([blob, blob[:1]]), BITS)


def case_file(pi, proof, blob, bits):
    opt = proof.options
    prog, exe = pi.memory_segments["program"], pi.memory_segments["execution"]
    words = [pi.n_steps, pi.rc_min, pi.rc_max, prog[0], prog[1], exe[0], exe[1], len(pi.public_memory)]
    words += [v for cell in pi.public_memory for v in cell]
    words += [opt.num_queries, opt.log_blowup, opt.grinding, opt.fold, opt.max_remainder, 1 if opt.hash == "sha256" else 0, bits]
    return np.concatenate([np.array(words, dtype=np.uint64), np.frombuffer(SEED, dtype=np.uint64), np.array([len(blob)], dtype=np.uint64), blob])


def test_parser_and_verifier_under_the_sanitizers(tmp_path, fixture_proof):
    """tests/cpp/gl_verify_blob_test.cpp: the parser, the verifier and the AIR built with -fsanitize=address,undefined as a program of its
    own (its own executable, no device runtime): the fixture verifies, every cut blob and every blob with a count set to 2^63 is refused,
    256 garbled ones are judged, and no read leaves a blob"""
    from sandstorm_amd import hostlib as h
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang++ to build the program with (%s)" % CLANG)
    pi, arrays = fixture_proof
    proof = gs.proof_from_arrays(arrays)
    case = str(tmp_path / "case.bin")
    case_file(pi, proof, h.gl_blob_of_proof(proof), BITS).tofile(case)
    host = os.path.join(ROOT, "sandstorm_amd", "host")
    exe = str(tmp_path / "gl_verify_blob_test")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", host, os.path.join(ROOT, "tests", "cpp", "gl_verify_blob_test.cpp")] +
                          [os.path.join(host, f) for f in ("goldilocks_verifier.cpp", "air_plain.cpp", "gl_transcript.cpp", "coin.cpp")] + ["-o", exe])
    out = subprocess.run([exe, case], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "malformed blobs refused" in out.stdout and ", 0 failures" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
