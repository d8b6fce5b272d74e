"""Statements to prove, for the benchmark, the smoke test and the tests: seeded synthetic columns and the
reference's shipped example run (`example/` of the reference: cairo-run's trace.bin / memory.bin / public input of array-sum,
2^14 steps; kept as data under tests/golden/) re-declared for a layout and padded to any power of two of steps - the program ends
in `jmp rel 0`, so repeating its final state is a valid run.  Host-side input preparation: nothing here is on the hot path."""
import copy
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE_DIR = os.path.join(ROOT, "tests", "golden", "example")
EXAMPLE_PUBLIC_INPUT = os.path.join(ROOT, "tests", "golden", "air_public_input_array_sum.json")

MASK64 = (1 << 64) - 1
SEED0 = 0x53414E4453544F52


def splitmix64_stream(seed, count):
    """vectorised SplitMix64: `count` successive outputs for `seed`."""
    with np.errstate(over="ignore"):
        idx = np.arange(1, count + 1, dtype=np.uint64)
        z = np.uint64(seed & MASK64) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def random_column(n, column_index=0, seed=SEED0):
    """(n,4) uint64: uniformly random-ish Montgomery images < p.

    4 SplitMix64 draws per element, top limb masked to 59 bits and elements
    >= p folded by clearing the top bits (valid Montgomery images are just
    integers < p, so any value < p is a legal element)."""
    raw = splitmix64_stream(seed ^ column_index, 4 * n).reshape(n, 4).copy()
    raw[:, 3] &= np.uint64((1 << 59) - 1)          # < 2^251 < p
    return raw


def load_run(example_dir=EXAMPLE_DIR, public_input_json=EXAMPLE_PUBLIC_INPUT):
    """the example run: register states, memory, public input"""
    from sandstorm_amd import binary, public_input
    with open(os.path.join(example_dir, "trace.bin"), "rb") as f:
        states = binary.read_register_states(f.read())
    with open(os.path.join(example_dir, "memory.bin"), "rb") as f:
        memory = binary.read_memory(f.read())
    pi = public_input.AirPublicInput.from_json(public_input_json)
    return states, memory, pi


def _move_heap(memory, new_base):
    """the program's one heap segment moved to new_base (behind the re-declared builtin segments), the pointers into it with it"""
    heap = [a for a in range(len(memory)) if memory[a] is not None and a > 1000]
    mem = list(memory) + [None] * (new_base + 16 - len(memory))
    for a in heap:
        mem[a] = None
    for a in heap:
        mem[new_base + a - heap[0]] = memory[a]
    for a in range(1000):
        if a < len(memory) and mem[a] is not None and heap[0] <= mem[a] <= heap[-1] + 1:
            mem[a] += new_base - heap[0]
    return mem


def recursive_example(log_steps):
    """the example run as a 2^log_steps-step statement of the recursive layout: padded with its final state, the builtin segments
    re-declared for that step count back to back behind the execution segment, the program's one heap segment moved behind them"""
    from sandstorm_amd.layouts import recursive as rec
    states, memory, pi = load_run()
    if (1 << log_steps) == len(states):
        return states, memory, pi
    assert (1 << log_steps) > len(states)
    states = list(states) + [states[-1]] * ((1 << log_steps) - len(states))
    pi = copy.deepcopy(pi)
    pi.n_steps = 1 << log_steps
    seg = dict(pi.memory_segments)
    addr = seg["execution"][1]
    seg["output"] = (addr, addr)
    for name, ratio, cells in (("pedersen", rec.PEDERSEN_BUILTIN_RATIO, 3), ("range_check", rec.RANGE_CHECK_BUILTIN_RATIO, 1),
                               ("bitwise", rec.BITWISE_RATIO, 5)):
        seg[name] = (addr, addr)                     # begin = stop: the program uses nothing of the segment
        addr += cells * (pi.n_steps // ratio)
    pi.memory_segments = seg
    return states, _move_heap(memory, addr), pi


def starknet_example(log_steps=17):
    """the example run re-declared for the starknet layout (>= 2^17 steps: its diluted check needs them): padded with its final
    state, the builtin segments laid out after the execution segment, the heap segment moved behind them"""
    from sandstorm_amd.layouts import starknet as sk
    states, memory, pi = load_run()
    states = list(states) + [states[-1]] * ((1 << log_steps) - len(states))
    pi.n_steps = 1 << log_steps
    spi = sk.example_public_input(pi)
    new_base = spi.memory_segments["poseidon"][0] + 6 * (pi.n_steps // sk.POSEIDON_RATIO)
    return states, _move_heap(memory, new_base), spi


def pedersen_slots(layout, log_steps):
    """Pedersen builtin instances a 2^log_steps-step trace of `layout` has room for"""
    from sandstorm_amd.layouts import recursive as rec, starknet as sk
    return (1 << log_steps) // (sk.PEDERSEN_BUILTIN_RATIO if layout == "starknet" else rec.PEDERSEN_BUILTIN_RATIO)


def seeded_pedersen_instances(slots, seed=SEED0):
    """`slots` distinct Pedersen instances (index, a, b), one per slot, as air-private-input.json's `pedersen` rows: a, b < 2^251 from
    SplitMix64.  The example program does not touch the builtin's segment, so any inputs make a valid statement: a run whose Pedersen
    slots are all REAL instances (the device generator's worst case) instead of the dummy one"""
    raw = splitmix64_stream(seed ^ 0x504544, 8 * slots).reshape(slots, 8).copy()
    raw[:, 3] &= np.uint64((1 << 59) - 1)
    raw[:, 7] &= np.uint64((1 << 59) - 1)
    word = lambda r, k: sum(int(r[k + j]) << (64 * j) for j in range(4))
    return [(i, word(raw[i], 0), word(raw[i], 4)) for i in range(slots)]


def bitwise_slots(layout, log_steps):
    """bitwise builtin instances a 2^log_steps-step trace of `layout` has room for"""
    from sandstorm_amd.layouts import recursive as rec, starknet as sk
    return (1 << log_steps) // (sk.BITWISE_RATIO if layout == "starknet" else rec.BITWISE_RATIO)


def poseidon_slots(log_steps):
    """Poseidon builtin instances a 2^log_steps-step starknet trace has room for (the recursive layout has no Poseidon builtin)"""
    from sandstorm_amd.layouts import starknet as sk
    return (1 << log_steps) // sk.POSEIDON_RATIO


def _seeded_values(slots, per_instance, seed):
    """`slots` rows of `per_instance` values < 2^251 from SplitMix64, as (index, v0, v1, ...)"""
    raw = splitmix64_stream(seed, 4 * per_instance * slots).reshape(slots, 4 * per_instance).copy()
    raw[:, 3::4] &= np.uint64((1 << 59) - 1)
    word = lambda r, k: sum(int(r[k + j]) << (64 * j) for j in range(4))
    return [(i,) + tuple(word(raw[i], 4 * v) for v in range(per_instance)) for i in range(slots)]


def seeded_bitwise_instances(slots, seed=SEED0):
    """`slots` distinct bitwise instances (index, x, y), one per slot, as air-private-input.json's `bitwise` rows: x, y < 2^251 from
    SplitMix64.  The example program does not touch the builtin's segment, so any inputs make a valid statement: a run whose bitwise
    slots are all REAL instances.  Their 68 diluted cells each load the diluted pool: at most 68 * slots + 65536 ordered slots, which
    fits the statements the suite and the tools saturate (starknet 2^17 / 2^20 steps, recursive 2^14 / 2^20 steps)"""
    return _seeded_values(slots, 2, seed ^ 0x425457)


def seeded_poseidon_instances(slots, seed=SEED0):
    """`slots` distinct Poseidon instances (index, in0, in1, in2), one per slot, as air-private-input.json's `poseidon` rows: inputs
    < 2^251 from SplitMix64 (see seeded_bitwise_instances)"""
    return _seeded_values(slots, 3, seed ^ 0x504f53)


def ec_op_slots(log_steps):
    """EC-op builtin instances a 2^log_steps-step starknet trace has room for (the recursive layout has no EC-op builtin)"""
    from sandstorm_amd.layouts import starknet as sk
    return (1 << log_steps) // sk.EC_OP_BUILTIN_RATIO


def seeded_ec_op_instances(slots, seed=SEED0):
    """`slots` distinct EC-op instances (index, p_x, p_y, q_x, q_y, m), one per slot, as air-private-input.json's `ec_op` rows: P and Q
    are 2 * slots consecutive points of the walk k G, (k + 1) G, ... from a seeded k (one scalar multiplication, then one affine
    addition of G per point: the Python mirror's arithmetic, layouts/starknet.py), m < 2^251 from SplitMix64.  No two of the points
    share an x, so every instance is distinct and no P meets its Q; that no partial sum meets a doubling of Q on the way is left to
    the generators, which refuse such an instance (none of the seeds the suite and the tools use has one)"""
    from sandstorm_amd.layouts import starknet as sk
    raw = splitmix64_stream(seed ^ 0x45434f50, 4 * (slots + 1)).reshape(slots + 1, 4).copy()
    raw[:, 3] &= np.uint64((1 << 59) - 1)
    word = lambda r: sum(int(r[j]) << (64 * j) for j in range(4))
    point = sk._ec_mul(word(raw[slots]) | 1 << 200, sk.GENERATOR)
    rows = []
    for i in range(slots):
        p = point
        q = sk._ec_add(p, sk.GENERATOR)
        point = sk._ec_add(q, sk.GENERATOR)
        rows.append((i, p[0], p[1], q[0], q[1], word(raw[i])))
    return rows


def ecdsa_slots(log_steps):
    """ECDSA builtin instances a 2^log_steps-step starknet trace has room for (the recursive layout has no ECDSA builtin)"""
    from sandstorm_amd.layouts import starknet as sk
    return (1 << log_steps) // sk.ECDSA_BUILTIN_RATIO


def seeded_ecdsa_instances(slots, seed=SEED0):
    """`slots` distinct ECDSA instances (index, pubkey_x, message, r, w), one per slot, as air-private-input.json's `ecdsa` rows: honest
    signatures - private key and message from SplitMix64 (key < 2^240, message < 2^250, both nonzero), the nonces k, k + 1, ... from a
    seeded k, r = x(k G), w = k / (message + r * key) mod the group's order as the builtin takes it, the next nonce until 0 < r, w < 2^251
    (the Python mirror's arithmetic, layouts/starknet.py; one affine addition of G per nonce).  The keys, the messages and the nonces
    differ from slot to slot, and the public key's y is the larger root for about half of the slots"""
    from sandstorm_amd.layouts import starknet as sk
    raw = splitmix64_stream(seed ^ 0x45434453, 4 * (2 * slots + 1)).reshape(2 * slots + 1, 4).copy()
    word = lambda r: sum(int(r[j]) << (64 * j) for j in range(4))
    k = word(raw[2 * slots]) % (1 << 200) | 1 << 200
    point = sk._ec_mul(k, sk.GENERATOR)
    rows = []
    for i in range(slots):
        key, message = word(raw[2 * i]) % (1 << 240) | 1, word(raw[2 * i + 1]) % (1 << 250) | 1
        while True:
            k, point = k + 1, sk._ec_add(point, sk.GENERATOR)
            r = point[0]
            s = (message + r * key) % sk.CURVE_ORDER
            w = k * pow(s, -1, sk.CURVE_ORDER) % sk.CURVE_ORDER if s else 0
            if 0 < r < 1 << 251 and 0 < w < 1 << 251:
                break
        rows.append((i, sk._ec_mul(key, sk.GENERATOR)[0], message, r, w))
    return rows
