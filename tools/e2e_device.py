"""files -> proof at 2^20 steps with the base trace made ON the device, WITHOUT torch (a fresh box pays 1-2 minutes for `import torch`):
  gen        ssh_base_trace_device alone (upload of trace.bin / memory.bin, plans, kernels, the status read): wall time of the call
  prove      the proof alone on the resident columns (ssh_prove)
  total      ONE ssh_prove_files_device call from the files to the proof
and, with E2E_HOST=1, the host-generated path (ssh_prove_files: generator thread + overlapped uploads) beside it.
python tools/e2e_device.py [starknet recursive] [log_steps] [--saturate-pedersen] [--saturate-bitwise] [--saturate-poseidon] [--saturate-ec-op] [--packed] [--json FILE]; one
line per layout, flushed as it is known.
--saturate-pedersen: every Pedersen slot of the statement holds a distinct seeded instance (examples.seeded_pedersen_instances: 32768 of
them in the starknet layout at 2^20 steps) instead of the dummy one - the normal case of a real run, and the generator's worst.
--saturate-bitwise, --saturate-poseidon: the same for the bitwise builtin's slots (examples.seeded_bitwise_instances: 16384 in the starknet layout
at 2^20 steps, 131072 in the recursive one) and the Poseidon builtin's (examples.seeded_poseidon_instances: 32768, starknet only); they combine.
--saturate-ec-op: the same for the EC-op builtin's slots (examples.seeded_ec_op_instances: 1024, starknet only).
--packed: those instances handed over as packed uint64 rows (hostlib.pack_instances), converted once outside the timed calls.
--json FILE: the raw run lists (seconds) per layout, appended as one JSON line.
To time an EARLIER commit beside this one (profiles/pedersen_device_trace.json), copy this file and sandstorm_amd/examples.py (the seeded
instances) onto that commit's built tree and run it there: the tool asks for hostlib.trace_last_stats only where the package has it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sandstorm_amd import backend as be, binary, examples, hostlib, public_input   # noqa: E402
from sandstorm_amd.prover import ProofOptions                                       # noqa: E402


def main(layouts, log_steps=20, repeats=5, saturate_pedersen=False, json_path=None, packed=False, saturate_bitwise=False, saturate_poseidon=False, saturate_ec_op=False):
    log_n = log_steps + 4
    n = 1 << log_n
    ctx = be.Context(0)
    for layout in layouts:
        if layout == "starknet":
            from sandstorm_amd.layouts import starknet as sk
            states, memory, xpi = examples.starknet_example(log_steps)
            nb = 9
            aux_idx = (sk.COL_NPC, sk.COL_MEMORY, sk.COL_RANGE_CHECK)
            tree_kind, n_friendly, coin_kind = be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY
            air = hostlib.StarknetHostAir(ctx, xpi, log_n, 1)
        else:
            from sandstorm_amd.layouts import recursive as rec
            states, memory, xpi = examples.recursive_example(log_steps)
            nb = 7
            aux_idx = (rec.COL_NPC, rec.COL_MEMORY, rec.COL_RANGE_CHECK, rec.COL_DILUTED_UNORDERED, rec.COL_DILUTED_ORDERED)
            tree_kind, n_friendly, coin_kind = be.TREE_FRIENDLY, 22, be.COIN_CAIRO
            air = hostlib.RecursiveHostAir(ctx, xpi, log_n, 1)
        trace_bin, memory_bin = binary.write_register_states(states), binary.write_memory(memory)
        del states, memory
        priv = {}
        if saturate_pedersen:
            priv["pedersen"] = examples.seeded_pedersen_instances(examples.pedersen_slots(layout, log_steps))
        if saturate_bitwise:
            priv["bitwise"] = examples.seeded_bitwise_instances(examples.bitwise_slots(layout, log_steps))
        if saturate_poseidon and layout == "starknet":
            priv["poseidon"] = examples.seeded_poseidon_instances(examples.poseidon_slots(log_steps))
        if saturate_ec_op and layout == "starknet":
            priv["ec_op"] = examples.seeded_ec_op_instances(examples.ec_op_slots(log_steps))
        given = {name: len(rows) for name, rows in priv.items()}
        priv = priv or None
        # --packed: the instances converted to the generators' uint64 rows ONCE, outside the timed calls (hostlib.pack_instances), as a
        # caller that has parsed its private input does; without it every call converts the Python integers again
        if priv and packed and hasattr(hostlib, "pack_instances"):
            priv = {name: hostlib.pack_instances(name, rows) for name, rows in priv.items()}
        seed = public_input.public_coin_seed(xpi, coin_kind)
        dev = [ctx.alloc(32 * n) for _ in range(nb)]
        keep = []

        def build_extension(challenges):
            for m in keep:
                m.close()
            del keep[:]
            keep.append(hostlib.build_extension_columns(ctx, layout, [dev[c] for c in aux_idx], n, challenges))
            return keep[0].cols
        options = ProofOptions()
        gen_s, prove_s, total_s, inner = [], [], [], []
        for it in range(repeats + 1):
            ctx.sync()
            t0 = time.perf_counter()
            hostlib.device_base_trace(ctx, layout, trace_bin, memory_bin, xpi, priv, dev)
            ctx.sync()
            if it:
                gen_s.append(time.perf_counter() - t0)
        for it in range(repeats + 1):
            ctx.sync()
            t0 = time.perf_counter()
            hostlib.prove(ctx, air, tree_kind, n_friendly, coin_kind, seed, dev, log_n, build_extension, options, want_proof=False)
            ctx.sync()
            if it:
                prove_s.append(time.perf_counter() - t0)
        for it in range(repeats + 1):
            ctx.sync()
            t0 = time.perf_counter()
            _, tm = hostlib.prove_files_device(ctx, layout, trace_bin, memory_bin, xpi, priv, dev, air, tree_kind, n_friendly, coin_kind, seed, build_extension,
                                               options, want_proof=False)
            ctx.sync()
            if it:
                total_s.append(time.perf_counter() - t0)
                inner.append(tm["trace_gen_s"])
        med = lambda v: sorted(v)[len(v) // 2]
        stats = hostlib.trace_last_stats() if hasattr(hostlib, "trace_last_stats") else None
        if json_path:
            with open(json_path, "a") as f:
                f.write(json.dumps({"layout": layout, "log_steps": log_steps, "pedersen_instances": given.get("pedersen", 0), "bitwise_instances": given.get("bitwise", 0),
                                    "poseidon_instances": given.get("poseidon", 0), "ec_op_instances": given.get("ec_op", 0), "packed": bool(priv) and not any(isinstance(v, list) for v in priv.values()), "gen_s": gen_s,
                                    "prove_s": prove_s, "total_s": total_s, "trace_gen_s": inner, "last_generation": stats}) + "\n")
        print("%s 2^%d steps%s, %.1f MB of files: device generator %s s; proof alone %s s; files -> proof (device generator) %s s = %.3f x the proof "
              "(the columns final %s s into the call); last generation %s"
              % (layout, log_steps, "".join(", %d real %s instances" % (count, name) for name, count in given.items()), (len(trace_bin) + len(memory_bin)) / 1e6, " ".join("%.4f" % v for v in gen_s), " ".join("%.4f" % v for v in prove_s),
                 " ".join("%.4f" % v for v in total_s), med(total_s) / med(prove_s), " ".join("%.4f" % v for v in inner), stats), flush=True)
        for m in keep:
            m.close()
        del keep[:]
        air.close()
        for d in dev:
            d.free()
        ctx.trim()


if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if a in ("starknet", "recursive")] or ["starknet", "recursive"]
    steps = [int(a) for a in sys.argv[1:] if a.isdigit()]
    json_out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    main(names, steps[0] if steps else 20, saturate_pedersen="--saturate-pedersen" in sys.argv, json_path=json_out, packed="--packed" in sys.argv,
         saturate_bitwise="--saturate-bitwise" in sys.argv, saturate_poseidon="--saturate-poseidon" in sys.argv, saturate_ec_op="--saturate-ec-op" in sys.argv)
