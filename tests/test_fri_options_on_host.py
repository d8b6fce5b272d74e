"""Every FRI folding factor and remainder bound the options offer, through the hosts - without a device.

`--fri-folding-factor` and `--fri-max-remainder-coeffs` (cli/src/main.rs:57-60) reach every prover and verifier of this library, and the
fold KERNELS are held to the oracle at 2, 4, 8 and 16; what sits around them - the bit-reversed column order of a committed layer, the
layer offsets, how positions fold, rows of 2, 4 or 16 values, the per-layer interpolation of the verifiers - ran at 8 alone.  Here:
  * the rule that says which (trace length, folding factor, max remainder) a prover takes - prover.fri_geometry, its C++ twin
    (host/prover.cpp, through hostlib.fri_geometry), verifier.fri_layer_count and both verifiers on hand-made wire bytes - accept and
    refuse together over a grid, and agree on the layers and the remainder; the same for the 64-bit field's rule;
  * a refused geometry is refused before a prover touches its context (the ones that used to end in a one-row Merkle tree or a layer
    length below zero included);
  * whole proofs at folds 2, 4 and 16 over the CPU oracle verify in both verifiers, and no tampered one does.
tests/test_gpu_fri_options.py holds the device to the proofs made here, bit for bit."""
import copy
import dataclasses

import numpy as np
import pytest

from tests import mini_air
from tests.test_verifier import cv, mini_verifier_air, pv

SEED = bytes(range(32))
LOG_NS = range(4, 13)
FOLDS = (2, 3, 4, 8, 16, 32)
MAX_REMAINDERS = (0, 1, 2, 3, 4, 8, 12, 16, 32, 128)
# the two geometries the provers used to take and the verifiers refuse: (log_n, fold, max remainder).  The first committed a third
# layer of ONE row (degree bound 256 -> 32 -> 4 > 2), the second shifted by log_len - log_fold = 3 - 4
REFUSED = [(8, 8, 2), (6, 16, 1)]
BAD_VALUES = [(8, 8, 0), (8, 8, 3), (8, 32, 4), (8, 3, 4), (8, 8, 12)]
# (fold, log_n, max remainder) of the whole proofs
WHOLE = [(2, 5, 4), (2, 6, 1), (2, 9, 4), (4, 5, 4), (4, 8, 2), (4, 10, 2), (16, 5, 4), (16, 9, 4), (16, 8, 2), (16, 7, 16)]
RULE_WORDS = ("FRI folding factor", "max remainder", "power of the folding factor", "exceed the evaluation domain")


def mont_be(v):
    from sandstorm_amd import wire
    return (v * wire._R % wire.P).to_bytes(32, "big")


def keccak_m20_leaf(vals):
    from sandstorm_amd.coin import keccak256
    return keccak256(b"".join(mont_be(v) for v in vals))[:20] + bytes(12)


def blake_m20_leaf(vals):
    from sandstorm_amd.coin import blake2s256
    return bytes(12) + blake2s256(b"".join(mont_be(v) for v in vals))[12:]


def mini_options(fold, max_remainder):
    from sandstorm_amd.prover import ProofOptions
    return ProofOptions(num_queries=12, grinding_factor=8, fri_folding_factor=fold, fri_max_remainder_coeffs=max_remainder)


def mini_proof(ctx, oracle, log_n, options, flavour="eth", seed=SEED):
    """the mini AIR's proof by the Python host over `ctx` (the CPU oracle's context, or a device's) -> (wire bytes, Proof).
    flavour "eth": Keccak-masked trees + Solidity coin; "cairo": FriendlyMerkleTree<22> + Cairo coin"""
    from sandstorm_amd import backend as be, wire
    from sandstorm_amd.coin import canonical
    from sandstorm_amd.prover import Claim, Prover
    n = 1 << log_n
    c0, c1 = mini_air.base_trace(n)
    base = be.Matrix.from_host(ctx, [oracle.to_mont(c0), oracle.to_mont(c1)])
    tree, coin, leaf = (be.FriendlyMerkleTree, be.COIN_CAIRO, blake_m20_leaf) if flavour == "cairo" else (be.LeafVariantMerkleTree, be.COIN_SOLIDITY, keccak_m20_leaf)
    claim = Claim(mini_air.make_air(oracle.to_mont), tree, coin)
    proof = Prover(ctx, claim, options).prove(seed, base, lambda ch: be.Matrix.from_host(
        ctx, [oracle.to_mont(mini_air.extension_trace(c0, canonical(ch[0])))]))
    return wire.serialize(wire.from_proof(proof, leaf)), proof


def claim_of(flavour):
    from sandstorm_amd import backend as be
    return (be.TREE_FRIENDLY, be.COIN_CAIRO) if flavour == "cairo" else (be.TREE_KECCAK_M20, be.COIN_SOLIDITY)


_oracle_proofs = {}


def oracle_mini_proof(oracle, fold, log_n, max_remainder, flavour="eth"):
    """the reference of every device-made proof: the same host code over the CPU oracle (made once per session, never changed)"""
    key = (fold, log_n, max_remainder, flavour)
    if key not in _oracle_proofs:
        from oracle.cpu_context import CpuContext
        _oracle_proofs[key] = mini_proof(CpuContext(), oracle, log_n, mini_options(fold, max_remainder), flavour)
    return _oracle_proofs[key]


# ---------------------------------------------------------------------------------------------------------------- the rule
def python_rule(n, fold, rem):
    from sandstorm_amd.prover import fri_geometry
    try:
        return fri_geometry(n, fold, rem)
    except ValueError as e:
        assert "FRI geometry refused" in str(e) and all(str(v) in str(e) for v in (n, fold, rem)), e
        return None


def cpp_rule(n, fold, rem):
    from sandstorm_amd import hostlib
    from sandstorm_amd._lib import SandstormHipError
    try:
        return hostlib.fri_geometry(n, fold, rem)
    except SandstormHipError as e:
        assert "FRI geometry refused" in str(e) and all(str(v) in str(e) for v in (n, fold, rem)), e
        return None


def layer_count_rule(n, fold, rem):
    from sandstorm_amd import verifier
    try:
        layers, bound = verifier.fri_layer_count(n, fold, rem)
        return layers, max(1, bound)
    except verifier.VerificationError:
        return None


def hand_made_wire(n, fold, rem):
    """wire bytes that carry these options and nothing a query phase could check: both verifiers replay the transcript as far as the
    FRI geometry, and either refuse it by the rule or go on to miss the layers"""
    from sandstorm_amd import wire
    w = wire.WireProof([12, 2, 8, fold, rem], n, b"\x11" * 32, b"\x22" * 32, b"\x33" * 32)
    w.ood_trace, w.ood_composition, w.remainder = [5, 6, 7, 8, 9, 10], [11, 12], [1]
    return wire.serialize(w)


def test_every_rule_accepts_and_refuses_the_same_geometries():
    """prover.fri_geometry, host/prover.cpp's fri_geometry, verifier.fri_layer_count, and verifier.py / host/verifier.cpp on hand-made
    wire bytes: one verdict per (trace length, folding factor, max remainder) of the grid, and where they accept, the same layers and
    remainder length; the layers fit the trace domain, and the last one keeps two rows at blowup 2"""
    from sandstorm_amd import backend as be, hostlib, verifier
    from sandstorm_amd._lib import SandstormHipError
    air_py, air_cpp = mini_verifier_air(), hostlib.HostAir(None, hostlib.AIR_MINI, 5)
    accepted = 0
    for log_n in LOG_NS:
        n = 1 << log_n
        for fold in FOLDS:
            for rem in MAX_REMAINDERS:
                what = "log_n %d fold %d max remainder %d" % (log_n, fold, rem)
                want = python_rule(n, fold, rem)
                assert cpp_rule(n, fold, rem) == want, what
                assert layer_count_rule(n, fold, rem) == want, what
                raw = hand_made_wire(n, fold, rem)
                for call, exc in ((lambda: verifier.verify(raw, air_py, be.TREE_KECCAK_M20, be.COIN_SOLIDITY, SEED, required_security_bits=0), verifier.VerificationError),
                                  (lambda: hostlib.verify(air_cpp, be.TREE_KECCAK_M20, be.COIN_SOLIDITY, SEED, raw, required_security_bits=0), SandstormHipError)):
                    with pytest.raises(exc) as err:
                        call()
                    by_rule = any(w in str(err.value) for w in RULE_WORDS)
                    assert by_rule == (want is None), (what, str(err.value))
                    if want is not None and want[0] > 0:
                        assert "number of FRI layers" in str(err.value), (what, str(err.value))
                if want is not None:
                    layers, rem_len = want
                    accepted += 1
                    assert rem_len * fold ** layers == n and 1 <= rem_len <= max(rem, 1) and (layers == 0 or rem_len * fold > rem), what
                    assert (fold.bit_length() - 1) * layers <= log_n, what
    air_cpp.close()
    assert python_rule(1 << 8, 8, 2) is None and python_rule(1 << 6, 16, 1) is None
    assert python_rule(1 << 9, 8, 4) == (3, 1) and python_rule(1 << 5, 8, 32) == (0, 32) and python_rule(1 << 8, 16, 2) == (2, 1)
    assert accepted == sum(1 for log_n in LOG_NS for fold in (2, 4, 8, 16) for rem in (1, 2, 4, 8, 16, 32, 128) if _reaches(1 << log_n, fold, rem))


def _reaches(n, fold, rem):
    """plain restatement of the rule for the count above: dividing by the folding factor lands at or below the bound exactly"""
    while n > rem:
        if n % fold:
            return False
        n //= fold
    return True


def gl_verifier_rule(n_lde, fold, rem):
    """goldilocks._verify's own words: the option ranges it insists on, then fri_shape"""
    from sandstorm_amd import goldilocks as gs
    if not (fold in (2, 4, 8, 16) and 1 <= rem <= 1 << 16):
        return None
    try:
        return gs.fri_shape(n_lde, gs.Options(fold=fold, max_remainder=rem))
    except ValueError:
        return None


def test_the_64_bit_fields_rules_accept_and_refuse_the_same_geometries():
    """goldilocks.fri_geometry (what Prover.prove asks first), host/goldilocks_prover.cpp's fri_shape (what gl::prove asks first) and the
    verifier's use of fri_shape: one verdict over the grid, the same layers and last length.  This field stops folding at
    max_remainder * blowup, so a bound that is no power of two is fine here"""
    from sandstorm_amd import goldilocks as gs, hostlib
    from sandstorm_amd._lib import SandstormHipError
    accepted = 0
    for log_n in LOG_NS:
        n_lde = 2 << log_n
        for fold in FOLDS:
            for rem in MAX_REMAINDERS:
                what = "log_n %d fold %d max remainder %d" % (log_n, fold, rem)
                want = gl_verifier_rule(n_lde, fold, rem)
                try:
                    got = gs.fri_geometry(n_lde, gs.Options(fold=fold, max_remainder=rem))
                except ValueError as e:
                    assert "FRI geometry refused" in str(e) and str(n_lde) in str(e), e
                    got = None
                assert got == want, what
                try:
                    got = hostlib.gl_fri_geometry(n_lde, 1, fold, rem)
                except SandstormHipError as e:
                    assert "FRI geometry refused" in str(e) and str(n_lde) in str(e), e
                    got = None
                assert got == want, what
                if want is not None:
                    accepted += 1
                    assert want[1] * fold ** want[0] == n_lde and want[1] <= 2 * rem
    assert accepted > 100
    assert gl_verifier_rule(2048, 16, 1) is None and gl_verifier_rule(2048, 16, 4) == (2, 8) and gl_verifier_rule(2048, 8, 16) == (2, 32)


# ------------------------------------------------------------------------------------------------------ refusal comes first
class Untouchable:
    """a context whose every method raises: a prover that refuses its options first never gets this far"""

    def __init__(self):
        self.touched = []

    def __getattr__(self, name):
        self.touched.append(name)
        raise AssertionError("the prover touched its context (%s) before it refused the options" % name)


@pytest.mark.parametrize("log_n,fold,max_remainder", REFUSED + BAD_VALUES)
def test_python_prover_refuses_before_it_touches_the_context(oracle, log_n, fold, max_remainder):
    from sandstorm_amd import backend as be
    from sandstorm_amd.prover import Claim, Prover
    ctx = Untouchable()
    base = be.Matrix(ctx, [None, None], 1 << log_n)
    claim = Claim(mini_air.make_air(oracle.to_mont), be.LeafVariantMerkleTree, be.COIN_SOLIDITY)
    with pytest.raises(ValueError, match="FRI geometry refused: .*trace length %d, folding factor %d, max remainder coefficients %d" % (1 << log_n, fold, max_remainder)):
        Prover(ctx, claim, mini_options(fold, max_remainder)).prove(SEED, base, lambda ch: None)
    assert ctx.touched == []


@pytest.mark.parametrize("log_n,fold,max_remainder", REFUSED + BAD_VALUES)
def test_cpp_prover_refuses_before_it_touches_the_context(log_n, fold, max_remainder):
    """ssh_prove_wire with NO context: a call that went on to the device would come back with the C ABI's refusal of a NULL context,
    not with the rule"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd._lib import SandstormHipError

    class NoContext:
        handle = None
    air = hostlib.HostAir(None, hostlib.AIR_MINI, log_n)
    cols = [0, 0]                                   # (no device, so no columns: the call must not get as far as reading them)
    try:
        with pytest.raises(SandstormHipError, match="FRI geometry refused: .*trace length %d, folding factor %d, max remainder coefficients %d" % (1 << log_n, fold, max_remainder)):
            hostlib.prove(NoContext(), air, be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY, SEED, cols, log_n, lambda ch: [], mini_options(fold, max_remainder), wire=True)
    finally:
        air.close()


GL_REFUSED = [(16, 1), (32, 16), (3, 16), (8, 0), (8, 1 << 17), (16, 2)]


@pytest.mark.parametrize("fold,max_remainder", GL_REFUSED)
def test_python_prover_of_the_64_bit_field_refuses_before_it_touches_the_context(fold, max_remainder):
    import torch
    from sandstorm_amd import goldilocks as gs
    ctx = Untouchable()
    base = [torch.zeros(1024, dtype=torch.int64) for _ in range(5)]
    with pytest.raises(ValueError, match="FRI geometry refused: .*LDE domain 2048, folding factor %d, max remainder %d" % (fold, max_remainder)):
        gs.Prover(ctx, gs.plain_air(), gs.Options(num_queries=20, grinding=8, fold=fold, max_remainder=max_remainder)).prove(SEED, base, lambda ch: [])
    assert ctx.touched == []


def test_oracle_refuses_a_tree_of_one_leaf(oracle):
    """as ss_merkle_build does: the checker used to take the process down there"""
    from sandstorm_amd import backend as be
    for leaves in (np.zeros((1, 32), dtype=np.uint8), np.zeros((0, 32), dtype=np.uint8)):
        with pytest.raises(ValueError, match="two leaves"):
            oracle.merkle_build(be.TREE_KECCAK_M20, 0, be.LEAF_DIGEST, leaves)
    nodes, _ = oracle.merkle_build(be.TREE_KECCAK_M20, 0, be.LEAF_DIGEST, np.zeros((2, 32), dtype=np.uint8))
    assert nodes.shape == (4, 32) and nodes[1].any()


# ------------------------------------------------------------------------------------------------ whole proofs, 252-bit field
def bump(lst, i):
    from sandstorm_amd import verifier
    lst[i] = (lst[i] + 1) % verifier.P


def flip(b):
    return bytes([b[0] ^ 1]) + bytes(b[1:])


def mini_tamperings(w):
    """-> [(name, mutate)] for a parsed proof: one value of an opened row in every FRI layer, one path node of the last layer, one
    remainder coefficient, the option byte changed to every other valid folding factor"""
    out = []
    for li in range(len(w.fri_layers)):
        out.append(("row value of FRI layer %d" % li, lambda t, li=li: bump(t.fri_layers[li].rows, len(t.fri_layers[li].rows) // 2)))
    if w.fri_layers:
        def node(t):
            o = t.fri_layers[-1].openings[-1]
            if o.path:                                                       # (a last layer of two rows has the sibling leaf alone)
                o.path[-1] = flip(o.path[-1])
            else:
                o.sibling = flip(o.sibling)
        out.append(("path node of the last FRI layer", node))
    out.append(("remainder coefficient", lambda t: bump(t.remainder, len(t.remainder) - 1)))
    for other in (2, 4, 8, 16):
        if other != w.options[3]:
            out.append(("folding factor byte %d" % other, lambda t, other=other: t.options.__setitem__(3, other)))
    return out


def check_mini_proof(raw, proof, log_n, options, flavour="eth", tamper=True):
    """both verifiers accept `raw` with the prover's positions and the rule's layers; neither accepts a tampered copy"""
    from sandstorm_amd import hostlib, verifier, wire
    from sandstorm_amd._lib import SandstormHipError
    from sandstorm_amd.prover import fri_geometry
    tree, coin = claim_of(flavour)
    layers, rem_len = fri_geometry(1 << log_n, options.fri_folding_factor, options.fri_max_remainder_coeffs)
    w = wire.parse(raw, tree)
    assert len(w.fri_layers) == layers and len(w.remainder) == rem_len
    assert w.options == [12, 2, 8, options.fri_folding_factor, options.fri_max_remainder_coeffs]
    assert all(len(l.rows) == options.fri_folding_factor * len(l.openings) for l in w.fri_layers)
    positions = pv(raw, mini_verifier_air(), tree, coin, SEED, expected_options=options)
    assert positions == proof.query_positions
    cpp = hostlib.HostAir(None, hostlib.AIR_MINI, log_n)
    try:
        assert cv(cpp, tree, coin, SEED, raw, expected_options=options) == positions
        for name, mutate in mini_tamperings(w) if tamper else []:
            t = wire.parse(raw, tree)
            mutate(t)
            bad = wire.serialize(t)
            assert bad != raw, name
            with pytest.raises(verifier.VerificationError):
                pv(bad, mini_verifier_air(), tree, coin, SEED)
                pytest.fail("verifier.py accepted a changed " + name)
            with pytest.raises(SandstormHipError):
                cv(cpp, tree, coin, SEED, bad)
                pytest.fail("host/verifier.cpp accepted a changed " + name)
    finally:
        cpp.close()


@pytest.mark.parametrize("fold,log_n,max_remainder", WHOLE)
def test_whole_proof_over_the_oracle_verifies_and_no_tampered_one_does(oracle, fold, log_n, max_remainder):
    raw, proof = oracle_mini_proof(oracle, fold, log_n, max_remainder)
    check_mini_proof(raw, proof, log_n, mini_options(fold, max_remainder))


def test_rows_of_sixteen_under_masked_blake2s_and_pedersen(oracle):
    """FriendlyMerkleTree<22> + Cairo coin at fold 16: rows of 16 values hashed by masked Blake2s, Pedersen nodes above them"""
    raw, proof = oracle_mini_proof(oracle, 16, 6, 4, "cairo")
    check_mini_proof(raw, proof, 6, mini_options(16, 4), "cairo")


# ------------------------------------------------------------------------------------------------- whole proofs, 64-bit field
GL_WHOLE = [(2, 16, "blake2s"), (4, 16, "blake2s"), (16, 16, "blake2s"), (16, 16, "sha256"), (2, 1, "blake2s"), (4, 2, "blake2s"), (16, 4, "blake2s")]
_gl = {}


def gl_example():
    """the 1024-row example of tests/test_goldilocks_stark.py -> (public input, base columns)"""
    from sandstorm_amd.layouts import plain as pl
    if "run" not in _gl:
        prog = pl.example_program(10)
        states, memory = pl.run(prog, 64)
        pi = pl.public_input_of(prog, states, memory)
        _gl["run"] = (pi, pl.base_trace(states, memory, pi))
    return _gl["run"]


def gl_options(fold, max_remainder, hash_name="blake2s"):
    from sandstorm_amd import goldilocks as gs
    return gs.Options(num_queries=20, grinding=8, fold=fold, max_remainder=max_remainder, hash=hash_name)


def gl_proof(ctx, options, device=None):
    """goldilocks.Prover over `ctx` (the oracle's context with CPU tensors, or a device's) on the example"""
    import torch
    from sandstorm_amd import goldilocks as gs
    pi, cols = gl_example()
    base = [torch.from_numpy(np.array(c, dtype=np.uint64).view(np.int64)).to(device or "cpu") for c in cols]
    return gs.Prover(ctx, gs.plain_air(), options).prove(SEED, base, lambda ch: gs.plain_extension_on_device(ctx, base, ch)[0], statement=pi)


def oracle_gl_proof(fold, max_remainder, hash_name="blake2s"):
    key = (fold, max_remainder, hash_name)
    if key not in _gl:
        from oracle.gl_cpu_context import GlCpuContext
        _gl[key] = gl_proof(GlCpuContext(), gl_options(fold, max_remainder, hash_name))
    return _gl[key]


def check_gl_proof(proof, options, tamper=True):
    from sandstorm_amd import goldilocks as gs
    from sandstorm_amd.layouts import plain as pl
    pi, _ = gl_example()
    air = gs.plain_air()
    layers, last = gs.fri_shape(2048, options)
    assert len(proof.fri_layers) == layers and proof.remainder.shape == (last, 3)
    assert all(fl.opening.rows.shape[1] == 3 * options.fold for fl in proof.fri_layers)
    positions = gs.verify(proof, air, SEED, statement=pi, expected_options=options, required_security_bits=28)
    assert len(positions) >= 15
    if not tamper:
        return
    cases = [("row value of FRI layer %d" % li, lambda p, li=li: p.fri_layers[li].opening.rows.__setitem__(
        (0, 3 * options.fold - 2), (int(p.fri_layers[li].opening.rows[0, 3 * options.fold - 2]) + 1) % pl.P)) for li in range(layers)]
    cases.append(("path node of the last FRI layer", lambda p: p.fri_layers[-1].opening.paths.__setitem__(
        (-1, -1, 0), int(p.fri_layers[-1].opening.paths[-1, -1, 0]) ^ 1)))
    cases.append(("remainder coefficient", lambda p: p.remainder.__setitem__((0, 2), (int(p.remainder[0, 2]) + 1) % pl.P)))
    cases += [("folding factor %d" % other, lambda p, other=other: setattr(p.options, "fold", other)) for other in (2, 4, 8, 16) if other != options.fold]
    for name, mutate in cases:
        p = copy.deepcopy(proof)
        mutate(p)
        with pytest.raises(gs.VerificationError):
            gs.verify(p, air, SEED, statement=pi, required_security_bits=28)
            pytest.fail("goldilocks.verify accepted a changed " + name)


@pytest.mark.parametrize("fold,max_remainder,hash_name", GL_WHOLE)
def test_whole_proof_of_the_64_bit_field_over_the_oracle(fold, max_remainder, hash_name):
    """rows of `fold` Fq3 values (2, 4 and 16 segments of three words: 384 bytes at 16 - six whole SHA-256 / Blake2s blocks, the
    padding's edge) through the row hash, the trees, the openings and the verifier's interpolation"""
    options = gl_options(fold, max_remainder, hash_name)
    proof = oracle_gl_proof(fold, max_remainder, hash_name)
    check_gl_proof(proof, options)
    assert dataclasses.asdict(proof.options) == dataclasses.asdict(options)
