"""The 64-bit field's claim proved and checked through the plain AIR the C++ host lowers itself (sandstorm_amd/host/air_plain.cpp): no
callback of any kind between the files, or resident columns, and the proof.

  1  hostlib.gl_prove_files_air, goldilocks.prove_files(lowering="host") and hostlib.gl_prove_air write the proof
     goldilocks.prove_files and goldilocks.Prover write for the same seed and statement, array for array - log_blowup 1 and 2, folds 2
     and 8, both hashes, validation off and on; hostlib.gl_verify and goldilocks.verify accept them
  2  hostlib.gl_check_trace_air returns goldilocks.check_trace's report on a clean trace and on one broken cell per constraint family,
     and a validating prove call fails with goldilocks.prove_files(validate=True)'s message
  3  refused files, log_blowup 0 and 5 and a FRI geometry no verifier takes are refused in today's words, before any launch
  4  a handle made for one trace length is refused by name for columns of another; two proofs from one handle are one proof, and a
     fresh handle's

Runs on the MI355X (`-m gpu`) and, in the CPU suite, on the host build of the device code (tests/test_gl64_air_on_host.py)."""
import os

import numpy as np
import pytest

from sandstorm_amd.layouts import plain as pl
from tests import gl64_programs

pytestmark = pytest.mark.gpu
EMULATED = os.environ.get("SS_TEST_HIPEMU") == "1"          # (the device code on the CPU: torch CPU tensors are its device buffers)
P = pl.P
SEED = bytes(range(32))
BITS = 8                                                    # 8 queries at blowup 2 + 4 grinding bits conjecture 12


@pytest.fixture(scope="module")
def env():
    """-> (context, torch device): ONE stream for torch's tensor ops and the C ABI's kernels, as tests/test_goldilocks_stark.py sets up"""
    import torch
    from sandstorm_amd import backend as be
    if EMULATED:
        c, dev = be.Context(0), torch.device("cpu")
    else:
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        torch.cuda.set_stream(stream)
        c = be.Context(0, stream=stream.cuda_stream)
    yield c, dev
    c.close()
    if not EMULATED:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))


_runs = {}


def run_of(name):
    """-> (public input, states, memory, trace.bin, memory.bin, host-made base columns) of a program run for a number of cycles"""
    from sandstorm_amd import binary as bn
    if name not in _runs:
        kind, cycles = name.split("-")
        prog = {"example": lambda: pl.example_program(10), "busy": gl64_programs.busy_program, "wide": gl64_programs.wide_offsets_program,
                "long": gl64_programs.long_program, "holes": gl64_programs.holes_program}[kind]()
        states, memory = pl.run(prog, int(cycles))
        pi = pl.public_input_of(prog, states, memory)
        cols = pl.base_trace(states, memory, pi) if kind in ("example", "busy") else None
        _runs[name] = (pi, states, memory, bn.write_register_states(states), bn.write_memory(memory), cols)
    return _runs[name]


def options(lb=1, fold=8, hash_name="blake2s", queries=8):
    from sandstorm_amd import goldilocks as gs
    return gs.Options(num_queries=queries, log_blowup=lb, grinding=4, fold=fold, hash=hash_name)


def tensors(cols, dev):
    import torch
    return [torch.from_numpy(np.array(c, dtype=np.uint64).view(np.int64)).to(dev) for c in cols]


def empty_columns(n, dev):
    import torch
    return [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(5)]


def assert_same_arrays(proof, want, what=""):
    from sandstorm_amd import goldilocks as gs
    got = gs.proof_to_arrays(proof)
    assert set(got) == set(want), what
    for k in sorted(want):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


# ------------------------------------------------------------------------------------------------------ 1. the same proof
RUNS = ["example-16", "example-128", "busy-128"] + ([] if EMULATED else ["example-1024"])
# (log_blowup, fold, hash, validate): both blowups, both folds, both hashes and validation off and on, each value with each other once
CASES = [(1, 8, "blake2s", False), (2, 2, "blake2s", True), (1, 2, "sha256", True), (2, 8, "sha256", False)]


@pytest.mark.parametrize("case", CASES, ids=["lb%d-fold%d-%s-%s" % (c[0], c[1], c[2], "validate" if c[3] else "plain") for c in CASES])
@pytest.mark.parametrize("name", RUNS)
def test_same_proof_as_the_python_lowering(env, name, case):
    from sandstorm_amd import goldilocks as gs, hostlib
    c, dev = env
    lb, fold, hash_name, validate = case
    opt = options(lb, fold, hash_name)
    pi, states, memory, trace_bin, memory_bin, cols = run_of(name)
    n = 16 * pi.n_steps
    want = gs.proof_to_arrays(gs.prove_files(c, trace_bin, memory_bin, pi, SEED, opt, out=empty_columns(n, dev), validate=validate))
    base = tensors(cols, dev)
    python = gs.Prover(c, gs.plain_air(), opt, validate=validate).prove(SEED, base, lambda ch: gs.plain_extension_on_device(c, base, ch)[0], statement=pi)
    assert_same_arrays(python, want, "goldilocks.Prover")
    air = hostlib.GlPlainAir(c, pi)
    proof, times = hostlib.gl_prove_files_air(c, air, opt, SEED, trace_bin, memory_bin, empty_columns(n, dev), validate=validate)
    assert_same_arrays(proof, want, "hostlib.gl_prove_files_air")
    assert times["total_s"] >= times["trace_gen_s"] > 0
    assert_same_arrays(hostlib.gl_prove_air(c, air, opt, SEED, base, validate=validate), want, "hostlib.gl_prove_air")
    assert_same_arrays(gs.prove_files(c, trace_bin, memory_bin, pi, SEED, opt, out=empty_columns(n, dev), validate=validate, lowering="host"), want,
                       "goldilocks.prove_files(lowering='host')")
    positions = gs.verify(proof, gs.plain_air(), SEED, statement=pi, expected_options=opt, required_security_bits=BITS)
    assert hostlib.gl_verify(air, proof, SEED, BITS) == positions
    assert hostlib.gl_verify(hostlib.GlPlainAir(None, pi), proof, SEED, BITS) == positions            # a host-only handle verifies as well
    air.close()


def test_the_handles_program_is_the_one_the_callback_hands_over(env):
    """with a context the handle's tables live on the device: the program names their address, and the descriptions are Python's"""
    from sandstorm_amd import hostlib
    c, dev = env
    pi = run_of("example-16")[0]
    air, host_only = hostlib.GlPlainAir(c, pi), hostlib.GlPlainAir(None, pi)
    ch, alpha = [(11, 22, 33), (5, 6, 7), (9, 8, 7)], (123, 456, 789)
    a, b = air.program(ch, alpha), host_only.program(ch, alpha)
    assert a["d_tables"] != 0 and a["tables"] is None and b["d_tables"] == 0
    assert np.array_equal(a["code"], b["code"]) and np.array_equal(a["consts"], b["consts"]) and a["table_desc"] == b["table_desc"]
    assert a["d_tables"] == air.program(ch, (1, 2, 3))["d_tables"], "the tables are the handle's, not made per proof"
    air.close()


# ------------------------------------------------------------------------------------------------------ 2. the same check report
CHALLENGES = [(11, 22, 33), (5, 6, 7), (9, 8, 7)]


def broken_traces(pi, cols, n):
    """-> {family: (base columns, extension edit or None)}: one cell broken per constraint family"""
    cpu = [list(col) for col in cols]
    cpu[pl.COL_RANGE_CHECK][16 * 2 + pl.Auxiliary.RES[1]] = (cpu[pl.COL_RANGE_CHECK][16 * 2 + pl.Auxiliary.RES[1]] + 1) % P
    public = [list(col) for col in cols]
    public[pl.COL_NPC][8 * 3 + pl.Npc.PUB_MEM_ADDR] = 5
    return {"clean": (cols, None), "a CPU cell": (cpu, None), "memory permutation step, coordinate 1": (cols, (1, 2 * 7, 1)),
            "rc16/perm/last at row n - 4": (cols, (0, n - 4 + 1, 1)), "public_memory_addr_zero": (public, None)}


@pytest.mark.parametrize("family", ["clean", "a CPU cell", "memory permutation step, coordinate 1", "rc16/perm/last at row n - 4", "public_memory_addr_zero"])
@pytest.mark.parametrize("name", ["example-16", "busy-128"])
def test_same_check_report_as_the_python_check_program(env, name, family):
    from sandstorm_amd import goldilocks as gs, hostlib
    c, dev = env
    pi, _, _, _, _, cols = run_of(name)
    n = 16 * pi.n_steps
    columns, edit = broken_traces(pi, cols, n)[family]
    base = tensors(columns, dev)
    ext = gs.plain_extension_on_device(c, base, CHALLENGES, check=False)[0]
    if edit is not None:
        coordinate, row, delta = edit
        ext[coordinate][row] += delta
    want = gs.check_trace(c, gs.plain_air(), base + ext, CHALLENGES, pi)
    air = hostlib.GlPlainAir(c, pi)
    assert hostlib.gl_check_trace_air(c, air, base + ext, CHALLENGES) == want
    assert (want == []) == (family == "clean")
    if family == "memory permutation step, coordinate 1":
        assert [w[1] for w in want] == ["memory/multi_column_perm/perm/step0"]
    if family == "rc16/perm/last at row n - 4":
        assert ("rc16/perm/last", n - 4) in [(w[1], w[3]) for w in want]
    if family == "public_memory_addr_zero":
        assert "public_memory_addr_zero" in [w[1] for w in want]
    air.close()


def test_validating_prove_calls_name_what_the_python_lowering_names(env):
    """the value the loop's first multiplication writes, changed in memory.bin: every validating path stops with the same message"""
    from sandstorm_amd import binary as bn, goldilocks as gs, hostlib
    from sandstorm_amd._lib import SandstormHipError
    c, dev = env
    pi, states, memory, trace_bin, _, good = run_of("example-16")
    n = 16 * pi.n_steps
    address = good[pl.COL_NPC][16 * 2 + pl.Npc.MEM_DST_ADDR]
    assert address not in [a for a, _ in pi.public_memory]
    wrong = list(memory)
    wrong[address] = (wrong[address] + 1) % P
    wrong_bin = bn.write_memory(wrong)
    opt = options()
    with pytest.raises(SandstormHipError, match="trace does not satisfy the AIR: .*cpu/") as e:
        gs.prove_files(c, trace_bin, wrong_bin, pi, SEED, opt, out=empty_columns(n, dev), validate=True)
    message = str(e.value)
    air = hostlib.GlPlainAir(c, pi)
    with pytest.raises(SandstormHipError) as e:
        gs.prove_files(c, trace_bin, wrong_bin, pi, SEED, opt, out=empty_columns(n, dev), validate=True, lowering="host")
    assert str(e.value) == message
    with pytest.raises(SandstormHipError) as e:
        hostlib.gl_prove_files_air(c, air, opt, SEED, trace_bin, wrong_bin, empty_columns(n, dev), validate=True)
    assert str(e.value) == message
    with pytest.raises(SandstormHipError) as e:
        hostlib.gl_prove_air(c, air, opt, SEED, tensors(pl.base_trace(states, wrong, pi), dev), validate=True)
    assert str(e.value) == message
    air.close()


# ------------------------------------------------------------------------------------------------------ 3. the same refusals
def refusal(call):
    from sandstorm_amd._lib import SandstormHipError
    with pytest.raises(SandstormHipError) as e:
        call()
    return str(e.value)


@pytest.mark.parametrize("name,message", [("wide-16", "range-check values do not fit the trace"), ("long-16", "public memory does not fit"),
                                          ("holes-16", "more memory holes than gap cells")])
def test_refused_files_are_refused_in_todays_words(env, name, message):
    from sandstorm_amd import goldilocks as gs
    c, dev = env
    pi, _, _, trace_bin, memory_bin, _ = run_of(name)
    for validate in (False, True):
        today = refusal(lambda: gs.prove_files(c, trace_bin, memory_bin, pi, SEED, options(), out=empty_columns(256, dev), validate=validate))
        assert message in today
        assert refusal(lambda: gs.prove_files(c, trace_bin, memory_bin, pi, SEED, options(), out=empty_columns(256, dev), validate=validate, lowering="host")) == today


def test_a_range_check_permutation_that_does_not_close_is_refused_in_todays_words(env):
    """resident columns whose ordered range-check values are not the pool's: the extension builder's refusal, before the trace check's"""
    from sandstorm_amd import goldilocks as gs, hostlib
    c, dev = env
    pi, _, _, _, _, cols = run_of("example-16")
    columns = [list(col) for col in cols]
    columns[pl.COL_RANGE_CHECK][4 * 5 + pl.RangeCheck.ORDERED] += 1
    base = tensors(columns, dev)
    air = hostlib.GlPlainAir(c, pi)
    for validate in (False, True):
        assert refusal(lambda: hostlib.gl_prove_air(c, air, options(), SEED, base, validate=validate)) == "host: the range-check permutation does not close"
    air.close()


BAD_OPTIONS = {"log_blowup 0": dict(log_blowup=0), "log_blowup 5": dict(log_blowup=5), "fold 3": dict(fold=3), "max_remainder 0": dict(max_remainder=0),
               "max_remainder 65537": dict(max_remainder=65537)}


@pytest.mark.parametrize("what", sorted(BAD_OPTIONS))
def test_blowups_and_fri_geometries_are_refused_in_todays_words_before_any_launch(env, what):
    import dataclasses
    import torch
    from sandstorm_amd import goldilocks as gs, hostlib
    c, dev = env
    opt = dataclasses.replace(options(), **BAD_OPTIONS[what])
    pi, _, _, trace_bin, memory_bin, cols = run_of("example-16")
    n = 16 * pi.n_steps
    base = tensors(cols, dev)
    air = hostlib.GlPlainAir(c, pi)
    out = [torch.full((n,), 0x5A5A5A5A, dtype=torch.int64, device=dev) for _ in range(5)]
    today = refusal(lambda: gs.prove_files(c, trace_bin, memory_bin, pi, SEED, opt, out=out))
    assert "refused" in today
    c.profile(True)
    try:
        c.profile_reset()
        assert refusal(lambda: hostlib.gl_prove_files_air(c, air, opt, SEED, trace_bin, memory_bin, out)) == today
        assert refusal(lambda: hostlib.gl_prove_files_air(c, air, opt, SEED, trace_bin, memory_bin, out, validate=True)) == today
        assert refusal(lambda: hostlib.gl_prove_air(c, air, opt, SEED, base)) == today
        assert sum(c.profile_read(kind)[1] for kind in range(8)) == 0
    finally:
        c.profile(False)
    assert all(bool((col == 0x5A5A5A5A).all()) for col in out), "a base column was written by a refused call"
    air.close()


# ------------------------------------------------------------------------------------------------------ 4. handle hygiene
def test_a_handle_of_another_trace_length_is_refused_by_name(env):
    from sandstorm_amd import goldilocks as gs, hostlib
    c, dev = env
    pi16, _, _, trace16, memory16, cols16 = run_of("example-16")
    pi128, _, _, trace128, memory128, cols128 = run_of("example-128")
    air = hostlib.GlPlainAir(c, pi128)
    base16 = tensors(cols16, dev)
    assert "the AIR handle was made for a trace of 2048 rows, the columns hold 256" in refusal(lambda: hostlib.gl_prove_air(c, air, options(), SEED, base16))
    assert "the AIR handle was made for 128 steps, the trace file holds 16" in refusal(
        lambda: hostlib.gl_prove_files_air(c, air, options(), SEED, trace16, memory16, empty_columns(256, dev)))
    ext16 = gs.plain_extension_on_device(c, base16, CHALLENGES)[0]
    assert "the AIR handle was made for a trace of 2048 rows, the columns hold 256" in refusal(lambda: hostlib.gl_check_trace_air(c, air, base16 + ext16, CHALLENGES))
    assert "columns for an AIR of 5 base and 3 extension coordinate columns" in refusal(lambda: hostlib.gl_check_trace_air(c, air, base16, CHALLENGES))
    host_only = hostlib.GlPlainAir(None, pi16)
    assert "made without a context" in refusal(lambda: hostlib.gl_prove_air(c, host_only, options(), SEED, base16))
    air.close()


def test_two_proofs_from_one_handle_are_one_proof_and_a_fresh_handles(env):
    from sandstorm_amd import goldilocks as gs, hostlib
    c, dev = env
    pi, _, _, trace_bin, memory_bin, cols = run_of("busy-128")
    n = 16 * pi.n_steps
    opt = options(lb=2, fold=2)
    air = hostlib.GlPlainAir(c, pi)
    first = gs.proof_to_arrays(hostlib.gl_prove_files_air(c, air, opt, SEED, trace_bin, memory_bin, empty_columns(n, dev))[0])
    other_seed = hostlib.gl_prove_air(c, air, opt, bytes(32), tensors(cols, dev))
    assert not np.array_equal(gs.proof_to_arrays(other_seed)["roots"][32:], first["roots"][32:])
    assert_same_arrays(hostlib.gl_prove_files_air(c, air, opt, SEED, trace_bin, memory_bin, empty_columns(n, dev), validate=True)[0], first, "the second proof")
    air.close()
    fresh = hostlib.GlPlainAir(c, pi)
    assert_same_arrays(hostlib.gl_prove_air(c, fresh, opt, SEED, tensors(cols, dev)), first, "a fresh handle")
    fresh.close()
