#!/usr/bin/env python3
"""What the 64-bit field's trace check (ss_check_constraints_gl64x3 behind goldilocks.check_trace and `validate` in the provers) costs
on the card, for the plain layout at 2^20 steps -> profiles/gl64_constraint_check.json:

  * the check alone on resident columns (base trace made on the device from the files, extension columns at fixed challenges), and the
    check program's instruction, constant and slot counts beside the composition program's;
  * files -> proof (goldilocks.prove_files) with validation on and off, alternated run by run in one process;
  * optionally (--parent ROOT: a built checkout of the commit before the check existed) files -> proof with validation off against that
    checkout's, alternated process by process in the same visit - two libraries with the same symbols cannot share a process.
    The bar for "off changes nothing" is the parent's own run-to-run spread in that visit: the two medians lie within each other's
    measured spread (min .. max).

Every GPU step is a process of its own under a time limit; a step that fails or runs out of time ends the whole run.

    python tools/gl64_constraint_check_timing.py [--parent ROOT] [--log-steps 20] [--repeats 7] [--rounds 2]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHALLENGES = [(11, 22, 33), (5, 6, 7), (9, 8, 7)]


def summary(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs), "runs": len(xs)}


def worker(root, log_steps, repeats, validation, check):
    """one process over one checkout: the example program's run padded with its final state; -> a JSON line"""
    sys.path.insert(0, root)
    import torch
    from sandstorm_amd import air_program as ap, backend as be, binary, goldilocks as gs
    from sandstorm_amd.layouts import plain as pl
    prog = pl.example_program(10)
    states, memory = pl.run(prog, 64)
    states = list(states) + [states[-1]] * ((1 << log_steps) - len(states))
    pi = pl.public_input_of(prog, states, memory)
    trace_bin, memory_bin = binary.write_register_states(states), binary.write_memory(memory)
    del states
    n = 16 << log_steps
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = be.Context(0, stream=stream.cuda_stream)
    cols = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(pl.NUM_BASE_COLUMNS)]
    opt, seed = gs.Options(), bytes(range(32))

    def prove(on):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kw = {"validate": True} if on else {}             # (the parent's prove_files has no such keyword)
        gs.prove_files(ctx, trace_bin, memory_bin, pi, seed, opt, out=cols, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    out = {"log_steps": log_steps, "root": os.path.basename(os.path.abspath(root))}
    modes = ["off", "on"] if validation == "both" else [validation]
    for m in modes:
        prove(m == "on")                                  # untimed: plans, tables, scratch
    times = {m: [] for m in modes}
    for _ in range(repeats):
        for m in modes:                                   # alternated run by run
            times[m].append(prove(m == "on"))
    out["files_to_proof"] = {m: summary(t) for m, t in times.items()}
    if check:
        air = gs.plain_air()
        gs.plain_base_trace_on_device(ctx, trace_bin, memory_bin, pi, out=cols)
        ext, _ = gs.plain_extension_on_device(ctx, cols, CHALLENGES)
        assert gs.check_trace(ctx, air, cols + ext, CHALLENGES, pi) == []
        alone = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bad = gs.check_trace(ctx, air, cols + ext, CHALLENGES, pi)
            torch.cuda.synchronize()
            alone.append(time.perf_counter() - t0)
            assert bad == []
        chk, domains, _, _ = air.checks(n, CHALLENGES, pi)
        tables = air.make_tables(n, opt.log_blowup)
        comp = ap.lower(air.composition(n, CHALLENGES, (3, 5, 7), tables, pi), gs.P, ext=True, symbols=tables.symbols)
        out["check_alone"] = summary(alone)               # (includes lowering the 47 numerators on the host, as the provers pay it)
        out["check_program"] = {"instructions": chk.n_instr, "constants": len(chk.consts), "slots": chk.n_slots, "checks": len(domains)}
        out["composition_program"] = {"instructions": comp.n_instr, "constants": len(comp.consts), "slots": comp.n_slots}
    print("RESULT " + json.dumps(out), flush=True)
    ctx.close()


def run_worker(root, args, validation, check):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--log-steps", str(args.log_steps), "--repeats", str(args.repeats),
           "--validation", validation] + (["--check"] if check else [])
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=args.step_timeout)        # (raises on the time limit: the run ends)
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    if out.returncode != 0 or not lines:
        raise RuntimeError("worker failed (%d): %s" % (out.returncode, (out.stdout + out.stderr)[-2000:]))
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--log-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="current / parent process pairs")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one GPU step (one process) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gl64_constraint_check.json"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--validation", default="both")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args.root, args.log_steps, args.repeats, args.validation, args.check)
    result = {"log_steps": args.log_steps, "repeats": args.repeats, "plain": run_worker(ROOT, args, "both", True)}
    if args.parent:
        cur, par = [], []
        for _ in range(args.rounds):                      # alternated process by process
            cur.append(run_worker(ROOT, args, "off", False)["files_to_proof"]["off"])
            par.append(run_worker(args.parent, args, "off", False)["files_to_proof"]["off"])
        pool = lambda rs: {"median_s": statistics.median([r["median_s"] for r in rs]), "min_s": min(r["min_s"] for r in rs),   # noqa: E731
                           "max_s": max(r["max_s"] for r in rs), "runs": sum(r["runs"] for r in rs), "processes": len(rs)}
        c, p = pool(cur), pool(par)
        result["validation_off_against_parent"] = {"current": c, "parent": p,
                                                   "medians_within_each_others_spread": p["min_s"] <= c["median_s"] <= p["max_s"] and c["min_s"] <= p["median_s"] <= c["max_s"]}
    print(json.dumps(result), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
