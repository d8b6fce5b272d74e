#!/usr/bin/env python3
"""What the trace check (ss_check_constraints behind ssh::check_trace, Air::validate_trace) costs on the card, for both 252-bit
layouts at 2^20 steps -> profiles/constraint_check.json:

  * the check alone on resident columns (base trace made on the device, extension columns at fixed challenges), and the check
    program's instruction, constant and slot counts beside the composition program's;
  * files -> proof (hostlib.prove_files_device) with validation on and off, alternated run by run in one process;
  * optionally (--parent ROOT: a built checkout of the commit before the check existed) files -> proof with validation off against
    that checkout's, alternated process by process in the same visit - two libraries with the same symbols cannot share a process.
    The condition: the two medians lie within each other's measured spread (min .. max).

    python tools/constraint_check_timing.py [--parent ROOT] [--log-steps 20] [--repeats 7] [--rounds 2]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2**251 + 17 * 2**192 + 1
CHALLENGES = [pow(7, 11 + 3 * i, P) for i in range(6)]


def summary(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs), "runs": len(xs)}


def worker(root, layout, log_steps, repeats, validation, check):
    """one process over one checkout: the statement bench.py's end_to_end leg proves; -> a JSON line"""
    sys.path.insert(0, root)
    import torch
    from sandstorm_amd import backend as be, binary, examples, hostlib, public_input
    from sandstorm_amd.prover import ProofOptions
    log_n = log_steps + 4
    n = 1 << log_n
    ctx = be.Context(0)
    if layout == "starknet":
        from sandstorm_amd.layouts import starknet as L
        states, memory, pi = examples.starknet_example(log_steps)
        nb, aux_idx = 9, (L.COL_NPC, L.COL_MEMORY, L.COL_RANGE_CHECK)
        tree_kind, n_friendly, coin_kind = be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY
        air = hostlib.StarknetHostAir(ctx, pi, log_n, 1)
    else:
        from sandstorm_amd.layouts import recursive as L
        states, memory, pi = examples.recursive_example(log_steps)
        nb, aux_idx = 7, (L.COL_NPC, L.COL_MEMORY, L.COL_RANGE_CHECK, L.COL_DILUTED_UNORDERED, L.COL_DILUTED_ORDERED)
        tree_kind, n_friendly, coin_kind = be.TREE_FRIENDLY, 22, be.COIN_CAIRO
        air = hostlib.RecursiveHostAir(ctx, pi, log_n, 1)
    trace_bin, memory_bin = binary.write_register_states(states), binary.write_memory(memory)
    del states, memory
    seed = public_input.public_coin_seed(pi, coin_kind)
    dev = [torch.empty((n, 4), dtype=torch.int64, device="cuda:0") for _ in range(nb)]
    keep = []

    def build_extension(challenges):
        del keep[:]
        keep.append(hostlib.build_extension_columns(ctx, layout, [dev[c] for c in aux_idx], n, challenges))
        return keep[0].cols

    def prove():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hostlib.prove_files_device(ctx, layout, trace_bin, memory_bin, pi, None, dev, air, tree_kind, n_friendly, coin_kind, seed, build_extension,
                                   ProofOptions(), want_proof=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    out = {"layout": layout, "log_steps": log_steps, "root": os.path.basename(os.path.abspath(root))}
    prove()                                              # untimed: plans and tables
    modes = ["off", "on"] if validation == "both" else [validation]
    times = {m: [] for m in modes}
    if "on" in modes:
        air.set_validation(True)
        prove()                                          # untimed: the check's tables and scratch
        air.set_validation(False)
    for _ in range(repeats):
        for m in modes:                                  # alternated run by run
            if m == "on":
                air.set_validation(True)
            times[m].append(prove())
            if m == "on":
                air.set_validation(False)
    out["files_to_proof"] = {m: summary(t) for m, t in times.items()}
    if check:
        hostlib.device_base_trace(ctx, layout, trace_bin, memory_bin, pi, None, dev)
        ch = [be.felt(c) for c in CHALLENGES]
        ext = hostlib.build_extension_columns(ctx, layout, [dev[c] for c in aux_idx], n, ch)
        cols = dev + ext.cols
        assert hostlib.check_trace(ctx, air, cols, log_n, ch) == []
        alone = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bad = hostlib.check_trace(ctx, air, cols, log_n, ch)
            torch.cuda.synchronize()
            alone.append(time.perf_counter() - t0)
            assert bad == []
        code, consts, n_slots, _, domains = air.check_program(n, ch)
        comp, _, _ = hostlib.prover_air(air).build_program(n, ch, be.felt(12345))
        out["check_alone"] = summary(alone)
        out["check_program"] = {"instructions": len(code) // 2, "constants": len(consts), "slots": n_slots, "checks": len(domains)}
        out["composition_program"] = {"instructions": len(comp.code) // 2, "constants": len(comp.consts_mont), "slots": comp.n_slots}
        ext.close()
    print("RESULT " + json.dumps(out), flush=True)
    air.close()
    ctx.close()


def run_worker(root, layout, args, validation, check):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", layout, "--root", root, "--log-steps", str(args.log_steps), "--repeats", str(args.repeats),
           "--validation", validation] + (["--check"] if check else [])
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    if out.returncode != 0 or not lines:
        raise RuntimeError("worker failed (%d): %s" % (out.returncode, (out.stdout + out.stderr)[-2000:]))
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--log-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="current / parent process pairs per layout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constraint_check.json"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--validation", default="both")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args.root, args.worker, args.log_steps, args.repeats, args.validation, args.check)
    result = {"log_steps": args.log_steps, "repeats": args.repeats, "layouts": {}}
    for layout in ("recursive", "starknet"):
        entry = run_worker(ROOT, layout, args, "both", True)
        if args.parent:
            cur, par = [], []
            for _ in range(args.rounds):                 # alternated process by process
                cur.append(run_worker(ROOT, layout, args, "off", False)["files_to_proof"]["off"])
                par.append(run_worker(args.parent, layout, args, "off", False)["files_to_proof"]["off"])
            pool = lambda rs: {"median_s": statistics.median([r["median_s"] for r in rs]), "min_s": min(r["min_s"] for r in rs),   # noqa: E731
                               "max_s": max(r["max_s"] for r in rs), "runs": sum(r["runs"] for r in rs), "processes": len(rs)}
            c, p = pool(cur), pool(par)
            entry["validation_off_against_parent"] = {"current": c, "parent": p,
                                                      "medians_within_each_others_spread": p["min_s"] <= c["median_s"] <= p["max_s"] and c["min_s"] <= p["median_s"] <= c["max_s"]}
        result["layouts"][layout] = entry
        print(json.dumps(entry), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
