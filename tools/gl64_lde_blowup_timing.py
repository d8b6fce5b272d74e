"""What the 64-bit field's claim costs at LDE blowup 4, 8 and 16, and that blowup 2 costs what it did: THIS tree's build and the PARENT
commit's ALTERNATED, `--rounds` times, in one visit of the card, on the plain layout's example run padded to 2^log_steps steps
(BASELINE.json configs[4]), files -> proof in one call (goldilocks.prove_files), with the query counts that conjecture 80 bits:
(log_blowup, queries) = (1, 65), (2, 32), (3, 22), (4, 16), 16 grinding bits.

  python tools/gl64_lde_blowup_timing.py --parent DIR [--log-steps 20] [--rounds 5] [--limit 420] [--max-log-rows 27] [--out profiles/gl64_lde_blowup.json]

DIR: a checkout of the parent commit with its libraries built (DIR/sandstorm_amd/_build); it proves at log_blowup 1 only - it refuses
the rest.  Every (round, tree) is a process of its own under its own time limit; a step that fails or runs out of time ends the
measurement there, and the record says so.  Per step and log_blowup: one untimed files -> proof (plans, tables) and one timed (host
clock around a call that ends in a device synchronise), and the proof's size (the bytes of its arrays).  A log_blowup whose LDE would
exceed 2^max-log-rows rows (27: the largest the GPU suite has run through the shared commitment kernels; log_blowup 4 at 2^20 steps is
2^28) is not run at that size and the record says so; one an entry point refuses for its size, or the card's memory cannot hold, is
recorded as that factor's error - the refusal's words.  Either is then measured at `--fallback-log-steps` (18), in steps of its own,
beside log_blowup 1 at that size.  This tree's step also times the sub-sampling stage alone at each
log_blowup above 1 - ss_subsample_rows_gl64 on 8 columns of n << log_blowup rows into 8 of 2n, `--copy-reps` launches between two
synchronises - beside hipMemcpyDtoD (ss_dev_copy) of the same output bytes in the same process.

Written to --out: the raw lists and
  blowup2_total   this tree's log_blowup-1 proof vs the parent's, beside the spread (max - min) of the parent's own repeats: the bar is
                  that this tree's median lies within that spread of the parent's
  totals          files -> proof time and proof size at each log_blowup
  subsample       per log_blowup: ms per launch, bytes written per second, the same for the plain copy, and the ratio of the two

  python tools/gl64_lde_blowup_timing.py --step TREE LOG_STEPS LBS
is one such process (LBS like 1,2,3): it imports sandstorm_amd from TREE and prints one JSON line.  No fallback: without a GPU it fails."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = {1: 65, 2: 32, 3: 22, 4: 16}
TRACE_COLS = 8                                              # 5 base + 3 extension coordinate columns


def step(tree, log_steps, lbs, copy_reps):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from sandstorm_amd import backend as be, binary as bn, goldilocks as gs, hostlib
    from sandstorm_amd.layouts import plain as pl
    assert os.path.dirname(os.path.dirname(os.path.abspath(hostlib.__file__))) == os.path.abspath(tree)
    prog = pl.example_program(10)
    states, memory = pl.run(prog, 64)
    states = list(states) + [states[-1]] * ((1 << log_steps) - len(states))
    pi = pl.public_input_of(prog, states, memory)
    trace_bin, memory_bin = bn.write_register_states(states), bn.write_memory(memory)
    del states
    n = 16 << log_steps
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = be.Context(0, stream=stream.cuda_stream)
    sync = lambda: (torch.cuda.synchronize(dev), ctx.sync())
    seed = bytes(range(32))
    scratch = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(5)]
    out = {}
    for lb in lbs:
        opt = gs.Options(num_queries=QUERIES[lb], log_blowup=lb)
        rec = {}
        try:
            for timed in (False, True):
                sync()
                t0 = time.perf_counter()
                proof = gs.prove_files(ctx, trace_bin, memory_bin, pi, seed, opt, out=scratch)
                sync()
                rec = {"total_ms": 1e3 * (time.perf_counter() - t0), "proof_bytes": int(sum(np.asarray(a).nbytes for a in gs.proof_to_arrays(proof).values())),
                       "queries": QUERIES[lb]}
                del proof
        except Exception as e:                                 # noqa: BLE001
            # only a refusal for the size is a result (and the larger factors behind it are not tried); any other error - a HIP error
            # after a fault among them - ends the step with a non-zero exit and nothing more started on the device
            text = str(e).lower()
            if "out of memory" not in text and "size out of range" not in text:
                raise
            out[str(lb)] = {"error": str(e)[:300]}
            break
        out[str(lb)] = rec
        torch.cuda.empty_cache()
        ctx.trim()
    sub = {}
    if hasattr(ctx, "subsample_rows_gl64"):
        for lb in lbs:
            if lb == 1 or "error" in out.get(str(lb), {"error": 1}):
                continue
            wide = [torch.zeros(n << lb, dtype=torch.int64, device=dev) for _ in range(TRACE_COLS)]
            narrow = [torch.empty(2 * n, dtype=torch.int64, device=dev) for _ in range(TRACE_COLS)]
            written = TRACE_COLS * 2 * n * 8

            def clock(body):
                body()                                          # warm-up
                sync()
                t0 = time.perf_counter()
                for _ in range(copy_reps):
                    body()
                sync()
                return 1e3 * (time.perf_counter() - t0) / copy_reps

            def plain_copy():
                for s, d in zip(wide, narrow):
                    be.check(ctx.lib.ss_dev_copy(ctx.handle, d.data_ptr(), s.data_ptr(), 2 * n * 8))
            ms = clock(lambda: ctx.subsample_rows_gl64(wide, 2 * n, lb - 1, narrow))
            copy_ms = clock(plain_copy)
            sub[str(lb)] = {"log_stride": lb - 1, "bytes_written": written, "ms": ms, "written_GB_per_s": written / (ms * 1e-3) / 1e9,
                            "memcpy_dtod_ms": copy_ms, "memcpy_dtod_GB_per_s": written / (copy_ms * 1e-3) / 1e9, "subsample_over_memcpy": ms / copy_ms}
            del wide, narrow
            torch.cuda.empty_cache()
    print(json.dumps({"n": n, "device": torch.cuda.get_device_name(0), "lbs": out, "subsample": sub}))
    ctx.close()


def main(argv):
    if argv[:1] == ["--step"]:
        step(argv[1], int(argv[2]), [int(v) for v in argv[3].split(",")], int(argv[4]) if len(argv) > 4 else 20)
        return 0
    opt = {"--parent": None, "--log-steps": "20", "--fallback-log-steps": "18", "--rounds": "5", "--limit": "420", "--copy-reps": "20", "--max-log-rows": "27",
           "--out": os.path.join(ROOT, "profiles", "gl64_lde_blowup.json")}
    for k in range(0, len(argv), 2):
        if argv[k] not in opt or k + 1 >= len(argv):
            print(__doc__)
            return 2
        opt[argv[k]] = argv[k + 1]
    if not opt["--parent"] or not os.path.exists(os.path.join(opt["--parent"], "sandstorm_amd", "_build", "libsandstorm_host.so")):
        print("--parent DIR: a checkout of the parent commit with its libraries built")
        return 2
    log_steps, fallback, rounds, limit = int(opt["--log-steps"]), int(opt["--fallback-log-steps"]), int(opt["--rounds"]), int(opt["--limit"])
    record = {"log_steps": log_steps, "rounds_asked": rounds, "ended_early": None, "refused": {},
              "how": "tools/gl64_lde_blowup_timing.py: parent and this build alternated per round, one process per (round, tree), files -> proof "
                     "(goldilocks.prove_files), one untimed and one timed proof per log_blowup, host clock around a call that ends in a device synchronise"}
    raw = {"parent": {}, "this": {}, "this_fallback": {}, "subsample": {}}

    def run(name, tree, steps, lbs, rnd):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", tree, str(steps), ",".join(str(v) for v in lbs), opt["--copy-reps"]]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=tree)
        except subprocess.TimeoutExpired:
            record["ended_early"] = "round %d %s: time limit of %d s" % (rnd, name, limit)
            return None
        if res.returncode != 0:
            record["ended_early"] = "round %d %s: exit status %d: %s" % (rnd, name, res.returncode, res.stderr[-400:])
            return None
        return json.loads(res.stdout.strip().splitlines()[-1])

    def keep(slot, got):
        for lb, rec in got["lbs"].items():
            s = slot.setdefault(lb, {"total_ms": [], "proof_bytes": None, "queries": QUERIES[int(lb)], "errors": []})
            if "error" in rec:
                s["errors"].append(rec["error"])
            else:
                s["total_ms"].append(round(rec["total_ms"], 3))
                s["proof_bytes"] = rec["proof_bytes"]
        for lb, rec in got["subsample"].items():
            raw["subsample"].setdefault("2^%d rows, log_blowup %s" % (got["n"].bit_length() - 1, lb), []).append(rec)
    lbs = [lb for lb in (1, 2, 3, 4) if log_steps + 4 + lb <= int(opt["--max-log-rows"])]
    record["refused"] = {str(lb): "not run: 2^%d rows > 2^%s" % (log_steps + 4 + lb, opt["--max-log-rows"]) for lb in (1, 2, 3, 4) if lb not in lbs}
    for rnd in range(rounds):
        for name, tree, wanted in (("parent", os.path.abspath(opt["--parent"]), [1]), ("this", ROOT, lbs)):
            if record["ended_early"]:
                break
            got = run(name, tree, log_steps, wanted, rnd)
            if got is None:
                break
            record["device"] = got["device"]
            keep(raw[name], got)
            refused = [int(lb) for lb, rec in got["lbs"].items() if "error" in rec]
            if name == "this" and refused:                      # that factor and the ones behind it: at the smaller size from now on
                record["refused"].update({str(lb): got["lbs"].get(str(lb), {}).get("error", "not tried: a smaller factor was refused") for lb in lbs if lb >= min(refused)})
                lbs = [lb for lb in lbs if lb < min(refused)]
            print("round %d %s: %s" % (rnd, name, {b: round(r.get("total_ms", -1)) for b, r in got["lbs"].items()}), flush=True)
        if record["refused"] and not record["ended_early"]:
            got = run("this at 2^%d steps" % fallback, ROOT, fallback, [1] + sorted(int(lb) for lb in record["refused"] if int(lb) > 1), rnd)
            if got is not None:
                keep(raw["this_fallback"], got)
    med = lambda v: sorted(v)[len(v) // 2] if v else None
    record["raw"] = raw
    par, this = raw["parent"].get("1"), raw["this"].get("1")
    if par and this and par["total_ms"] and this["total_ms"]:
        spread = max(par["total_ms"]) - min(par["total_ms"])
        record["blowup2_total"] = {"parent_median_ms": med(par["total_ms"]), "this_median_ms": med(this["total_ms"]), "parent_spread_ms": round(spread, 3),
                                   "within_the_parents_spread": abs(med(this["total_ms"]) - med(par["total_ms"])) <= spread}
    record["totals"] = {"2^%d steps" % s: {lb: {"queries": v["queries"], "total_median_ms": med(v["total_ms"]), "proof_bytes": v["proof_bytes"], "errors": v["errors"]}
                                          for lb, v in sorted(slot.items())} for s, slot in ((log_steps, raw["this"]), (fallback, raw["this_fallback"])) if slot}
    record["subsample"] = {k: {"log_stride": v[0]["log_stride"], "bytes_written": v[0]["bytes_written"], "median_ms": med([r["ms"] for r in v]),
                               "written_GB_per_s": med([r["written_GB_per_s"] for r in v]), "memcpy_dtod_median_ms": med([r["memcpy_dtod_ms"] for r in v]),
                               "memcpy_dtod_GB_per_s": med([r["memcpy_dtod_GB_per_s"] for r in v]),
                               "subsample_over_memcpy": med([r["subsample_over_memcpy"] for r in v])} for k, v in raw["subsample"].items()}
    with open(opt["--out"], "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": opt["--out"], "ended_early": record["ended_early"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
