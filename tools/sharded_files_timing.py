"""What files -> proof costs on the SHARDED path (host/sharded.cpp), on one MI355X with a group of one rank, WITHOUT torch: three routes
to the same proof bytes, alternated in one visit after one untimed pass each -
  (a) files_sharded   ONE hostlib.prove_files_sharded_device call: the files' bytes go up, the base trace is made in HBM, the rank keeps
                      its columns and auxiliary blocks and proves
  (b) host_route      the only route to those bytes before that entry: hostlib.*_base_trace on the host, upload of the owned columns and of
                      the auxiliary blocks, hostlib.prove_sharded with hostlib.build_extension_blocks in its callback
  (c) resident        hostlib.prove_sharded alone, columns and auxiliary blocks already in HBM
- for the padded example statements of both layouts at 2^20 steps (what bench.py's end-to-end leg proves).  Before anything is timed
the three routes must write the same proof bytes.  Writes profiles/sharded_files_to_proof.json: medians, min / max and the raw lists,
the bytes each route uploads, total(a) / total(c) and the generation's share of (a) (the entry's own trace_gen_s).
python tools/sharded_files_timing.py [starknet recursive] [log_steps] [--rounds N] [--json FILE]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sandstorm_amd import backend as be, binary, examples, hostlib, public_input   # noqa: E402
from sandstorm_amd.prover import ProofOptions                                       # noqa: E402

ESTIMATES = ("estimates made before the runs, not bars: (a) / (c) near the single-device path's 1.024 - 1.026; (b) slower than (a) by roughly "
             "what the host route cost on one device (0.31 s against 0.23 s)")


def summary(v):
    return {"median_s": sorted(v)[len(v) // 2], "min_s": min(v), "max_s": max(v), "runs_s": v}


def time_layout(ctx, layout, log_steps, rounds):
    log_n = log_steps + 4
    n = 1 << log_n
    if layout == "starknet":
        from sandstorm_amd.layouts import starknet as sk
        states, memory, pi = examples.starknet_example(log_steps)
        ncols, aux_idx = 9, (sk.COL_NPC, sk.COL_MEMORY, sk.COL_RANGE_CHECK)
        tree_kind, n_friendly, coin_kind = be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY
        air, host_trace = hostlib.StarknetHostAir(ctx, pi, log_n, 1), hostlib.starknet_base_trace
    else:
        from sandstorm_amd.layouts import recursive as rec
        states, memory, pi = examples.recursive_example(log_steps)
        ncols, aux_idx = 7, (rec.COL_NPC, rec.COL_MEMORY, rec.COL_RANGE_CHECK, rec.COL_DILUTED_UNORDERED, rec.COL_DILUTED_ORDERED)
        tree_kind, n_friendly, coin_kind = be.TREE_FRIENDLY, 22, be.COIN_CAIRO
        air, host_trace = hostlib.RecursiveHostAir(ctx, pi, log_n, 1), hostlib.recursive_base_trace
    trace_bin, memory_bin = binary.write_register_states(states), binary.write_memory(memory)
    del states, memory
    seed = public_input.public_coin_seed(pi, coin_kind)
    options = ProofOptions()
    group = hostlib.LocalGroup(1)
    host_cols = host_trace(trace_bin, memory_bin, pi)          # (b) writes these arrays again in every pass
    dev = [ctx.alloc(32 * n) for _ in range(ncols)]
    aux = [ctx.alloc(32 * n) for _ in aux_idx]                 # a group of one: a rank's block is the whole column
    keep = []

    def ext_blocks(challenges):
        for m in keep:
            m.close()
        del keep[:]
        keep.append(hostlib.build_extension_blocks(ctx, layout, aux, n, 0, 1, group, challenges))
        return keep[0].cols

    def resident():
        return hostlib.prove_sharded(ctx, air, tree_kind, n_friendly, coin_kind, seed, 0, 1, group, dict(enumerate(dev)), log_n, None, options,
                                     extension_blocks=ext_blocks)

    def host_route():
        host_trace(trace_bin, memory_bin, pi, None, host_cols)
        for c in range(ncols):
            dev[c].upload(host_cols[c])
        for k, c in enumerate(aux_idx):
            aux[k].upload(host_cols[c])
        return resident()
    gen_share = []

    def files_sharded():
        raw, tm = hostlib.prove_files_sharded_device(ctx, layout, trace_bin, memory_bin, pi, None, air, tree_kind, n_friendly, coin_kind, seed, 0, 1, group, options)
        gen_share.append(tm["trace_gen_s"])
        return raw
    routes = (("files_sharded", files_sharded), ("host_route", host_route), ("resident", resident))
    # the untimed pass: the three routes write the same bytes ((b) leaves the columns and blocks (c) proves from)
    proofs = {}
    for name in ("host_route", "resident", "files_sharded"):
        proofs[name] = dict(routes)[name]()
        ctx.sync()
    assert proofs["files_sharded"] == proofs["host_route"] == proofs["resident"] and proofs["resident"], "the three routes must write the same proof"
    del gen_share[:]
    times = {name: [] for name, _ in routes}
    for _ in range(rounds):
        for name, fn in routes:
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            times[name].append(time.perf_counter() - t0)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"layout": layout, "log_steps": log_steps, "proof_bytes": len(proofs["resident"]), "rounds": rounds,
           "uploaded_bytes": {"files_sharded": len(trace_bin) + len(memory_bin), "host_route": 32 * n * (ncols + len(aux_idx)), "resident": 0},
           "files_sharded": summary(times["files_sharded"]), "host_route": summary(times["host_route"]), "resident": summary(times["resident"]),
           "trace_gen_s": summary(gen_share),
           "files_sharded_over_resident": med(times["files_sharded"]) / med(times["resident"]),
           "host_route_over_files_sharded": med(times["host_route"]) / med(times["files_sharded"]),
           "generation_share_of_files_sharded": med(gen_share) / med(times["files_sharded"]),
           "last_generation": hostlib.trace_last_stats()}
    print("%s 2^%d steps: (a) files -> proof, sharded entry %.4f s (columns final %.4f s in); (b) host generator + uploads + prove_sharded %.4f s; "
          "(c) prove_sharded on resident columns %.4f s; (a) / (c) = %.3f" % (layout, log_steps, med(times["files_sharded"]), med(gen_share),
                                                                             med(times["host_route"]), med(times["resident"]), out["files_sharded_over_resident"]), flush=True)
    for m in keep:
        m.close()
    del keep[:]
    group.close()
    air.close()
    for d in dev + aux:
        d.free()
    del host_cols
    ctx.trim()
    return out


def main(layouts, log_steps=20, rounds=5, json_path=None):
    ctx = be.Context(0)
    results = [time_layout(ctx, layout, log_steps, rounds) for layout in layouts]
    ctx.close()
    doc = {"what": "files -> proof on the sharded path, one MI355X, a group of one rank (tools/sharded_files_timing.py): the three routes alternated "
                   "%d times in one visit after one untimed pass in which they wrote the same proof bytes" % rounds,
           "status": "measured", "estimates": ESTIMATES, "results": results}
    with open(json_path or os.path.join(ROOT, "profiles", "sharded_files_to_proof.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    names = [a for a in argv if a in ("starknet", "recursive")] or ["starknet", "recursive"]
    flagged = {argv[i + 1] for i, a in enumerate(argv[:-1]) if a in ("--rounds", "--json")}
    steps = [int(a) for a in argv if a.isdigit() and a not in flagged]
    main(names, steps[0] if steps else 20, int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 5,
         argv[argv.index("--json") + 1] if "--json" in argv else None)
