"""What lowering the plain AIR in the C++ host buys the 64-bit field's claim, and how far files -> proof then is from the proof alone: in
ONE visit of the card and one process, on the plain layout's example run padded to 2^log_steps steps (BASELINE.json configs[4]), after a
warm-up of each, `--runs` runs of each of

  python   goldilocks.prove_files(lowering="python")     the composition program lowered by air_program.py per proof, through a callback
  host     goldilocks.prove_files(lowering="host")       the plain AIR lowered by host/air_plain.cpp: no callback; one handle for all runs
  resident hostlib.gl_prove_air                          the proof alone, on resident base columns (the same handle)

ALTERNATED run by run, the host clock around a call that ends in a device synchronise.

  python tools/gl64_host_lowering_timing.py [--log-steps 20] [--runs 5] [--out profiles/gl64_host_lowering.json]

Written to --out: the raw lists, medians and spreads (max - min), trace_gen_s of both files paths, the CPU-side cost of each lowering
(made and timed without the device), and
  host_vs_python            median(host) - median(python) beside the python runs' own spread: the expectation is that host is not slower
                            than python by more than that spread
  files_over_proof_alone    median(host) / median(resident): the share of the gap between files -> proof and the proof alone that
                            remains once Python is off the critical path (1.33 x through the Python lowering when it was last measured)
Without a GPU nothing is measured and the record says "not measured"."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lowering_cost(pi, n, reps=5):
    """the CPU side of each lowering, per proof, without a device: seconds (medians)"""
    from sandstorm_amd import air_program as ap, hostlib
    from sandstorm_amd.layouts import plain as pl
    ch, alpha = [(11, 22, 33), (5, 6, 7), (9, 8, 7)], (123, 456, 789)
    med = lambda v: sorted(v)[len(v) // 2]
    py, host = [], []
    air = hostlib.GlPlainAir(None, pi)
    for _ in range(reps):
        t0 = time.perf_counter()
        tables = pl.Tables(n, 1)
        prog = ap.lower(pl.composition(n, pl.Hints.from_public_input(pi, ch, n), ch, alpha, tables), pl.P, ext=True, symbols=tables.symbols)
        tables.device_tables()
        py.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        air.program_blob(ch, alpha)
        host.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    hostlib.GlPlainAir(None, pi).close()
    create = time.perf_counter() - t0
    air.close()
    return {"python_lower_per_proof_s": med(py), "host_constants_per_proof_s": med(host), "host_handle_once_s": create, "n_instr": len(prog.code) // 2}


def main(argv):
    opt = {"--log-steps": "20", "--runs": "5", "--out": os.path.join(ROOT, "profiles", "gl64_host_lowering.json")}
    for k in range(0, len(argv), 2):
        if argv[k] not in opt or k + 1 >= len(argv):
            print(__doc__)
            return 2
        opt[argv[k]] = argv[k + 1]
    log_steps, runs = int(opt["--log-steps"]), int(opt["--runs"])
    import torch
    from sandstorm_amd import binary as bn
    from sandstorm_amd.layouts import plain as pl
    prog = pl.example_program(10)
    states, memory = pl.run(prog, 64)
    states = list(states) + [states[-1]] * ((1 << log_steps) - len(states))
    pi = pl.public_input_of(prog, states, memory)
    n = 16 << log_steps
    record = {"log_steps": log_steps, "runs_asked": runs,
              "how": "tools/gl64_host_lowering_timing.py: one process, one warm-up of each, then python / host / resident alternated run by run, host clock "
                     "around a call that ends in a device synchronise; options: goldilocks.Options() (65 queries, blowup 2, 16 grinding bits)",
              "cpu_side": lowering_cost(pi, n)}
    if not torch.cuda.is_available():
        record["measured"] = "not measured: no GPU in this process"
    else:
        from sandstorm_amd import backend as be, goldilocks as gs, hostlib
        trace_bin, memory_bin = bn.write_register_states(states), bn.write_memory(memory)
        del states
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        torch.cuda.set_stream(stream)
        ctx = be.Context(0, stream=stream.cuda_stream)
        sync = lambda: (torch.cuda.synchronize(dev), ctx.sync())
        seed, options = bytes(range(32)), gs.Options()
        cols = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(5)]
        air = hostlib.GlPlainAir(ctx, pi)
        gen = {"python": [], "host": []}

        def files(lowering):
            _, times = gs.prove_files(ctx, trace_bin, memory_bin, pi, seed, options, out=cols, want_times=True, lowering=lowering, air=air if lowering == "host" else None)
            gen[lowering].append(times["trace_gen_s"])
        paths = {"python": lambda: files("python"), "host": lambda: files("host"), "resident": lambda: hostlib.gl_prove_air(ctx, air, options, seed, cols)}
        raw = {name: [] for name in paths}
        for rnd in range(runs + 1):                          # round 0: the warm-up (plans, tables, the pool); `cols` hold the trace from then on
            for name, call in paths.items():
                sync()
                t0 = time.perf_counter()
                call()
                sync()
                if rnd:
                    raw[name].append(round(1e3 * (time.perf_counter() - t0), 3))
        med = lambda v: sorted(v)[len(v) // 2]
        record["device"] = torch.cuda.get_device_name(0)
        record["raw_ms"] = raw
        record["median_ms"] = {k: med(v) for k, v in raw.items()}
        record["spread_ms"] = {k: round(max(v) - min(v), 3) for k, v in raw.items()}
        record["trace_gen_s"] = {k: med(v[1:]) for k, v in gen.items()}
        slower_by = record["median_ms"]["host"] - record["median_ms"]["python"]
        record["host_vs_python"] = {"host_minus_python_ms": round(slower_by, 3), "python_spread_ms": record["spread_ms"]["python"],
                                    "host_not_slower_than_python_by_more_than_its_spread": slower_by <= record["spread_ms"]["python"]}
        record["files_over_proof_alone"] = {"python": round(record["median_ms"]["python"] / record["median_ms"]["resident"], 4),
                                            "host": round(record["median_ms"]["host"] / record["median_ms"]["resident"], 4)}
        record["measured"] = "yes"
        air.close()
        ctx.close()
    with open(opt["--out"], "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": opt["--out"], "measured": record["measured"], "median_ms": record.get("median_ms"), "files_over_proof_alone": record.get("files_over_proof_alone")}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
