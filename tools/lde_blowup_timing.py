"""What LDE blowup factors above 2 cost, and that blowup 2 costs what it did: THIS tree's build and the PARENT commit's ALTERNATED,
`--rounds` times, in one visit of the card, at 2^log_steps steps of the starknet and the recursive statement bench.py proves, columns
resident, with the C++ prover's stage clocks (SSH_TIMING: a device sync at every stage boundary).  WITHOUT torch.

  python tools/lde_blowup_timing.py --parent DIR [--log-steps 20] [--rounds 5] [--limit 420] [--max-log-rows 27] [--out profiles/lde_blowup_factors.json]

DIR: a checkout of the parent commit with its libraries built (DIR/sandstorm_amd/_build); it proves at blowup 2 only - it refuses the
rest.  Every (round, tree, layout) is a process of its own under its own time limit; a step that fails or runs out of time ends the
measurement there, and the record says so.  Per step: the statement's base trace made on the device once, then per (blowup, queries) of
(2, 65), (4, 32), (8, 22), (16, 16) one untimed proof (plans, tables) and one timed.  A factor the card's memory cannot hold (an
out-of-memory status, nothing else) is recorded as an error of that factor and ends the step's list there; any other error fails the step; a factor whose LDE would exceed 2^max-log-rows rows (27: the largest the GPU suite has
run; blowup 16 at 2^20 steps is 2^28) is not run and the record says so - give a smaller --log-steps for it.

Written to --out: the raw lists (ms) and, against the PARENT's numbers only,
  blowup2_total       this tree's blowup-2 proof vs the parent's, beside the spread (max - min) of the parent's own repeats
  quotient_stage      blowup 4 / 8 / 16: sub-sampling + constraint kernels vs the parent's blowup-2 quotient stage at the same n (the same
                      2n points), the measured sub-sampling time and that spread being the allowance
  subsample           the sub-sampling stage per stride: ms and bytes written per second (ncols x 2n x 32 bytes)
  totals              proof time and proof size at each pair (no parent to compare with: recorded only)

  python tools/lde_blowup_timing.py --step TREE LAYOUT LOG_STEPS PAIRS
is one such process (PAIRS like 2:65,4:32): it imports sandstorm_amd from TREE and prints one JSON line."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(2, 65), (4, 32), (8, 22), (16, 16)]
STAGE = re.compile(r"\[ssh timing\] (.+?)\s+([0-9.]+) ms")


def step(tree, layout, log_steps, pairs):
    sys.path.insert(0, tree)
    from sandstorm_amd import backend as be, binary, examples, hostlib, public_input
    from sandstorm_amd.prover import ProofOptions
    assert os.path.dirname(os.path.dirname(os.path.abspath(hostlib.__file__))) == os.path.abspath(tree)
    log_n = log_steps + 4
    n = 1 << log_n
    if layout == "starknet":
        from sandstorm_amd.layouts import starknet as lay
        states, memory, pi = examples.starknet_example(log_steps)
        aux, tree_kind, nf, coin = (lay.COL_NPC, lay.COL_MEMORY, lay.COL_RANGE_CHECK), be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY
        Air = hostlib.StarknetHostAir
    else:
        from sandstorm_amd.layouts import recursive as lay
        states, memory, pi = examples.recursive_example(log_steps)
        aux = (lay.COL_NPC, lay.COL_MEMORY, lay.COL_RANGE_CHECK, lay.COL_DILUTED_UNORDERED, lay.COL_DILUTED_ORDERED)
        tree_kind, nf, coin, Air = be.TREE_FRIENDLY, 22, be.COIN_CAIRO, hostlib.RecursiveHostAir
    trace_bin, memory_bin = binary.write_register_states(states), binary.write_memory(memory)
    del states, memory
    ctx = be.Context(0)
    cols = hostlib.device_base_trace(ctx, layout, trace_bin, memory_bin, pi)
    air = Air(ctx, pi, log_n, 1)
    seed = public_input.public_coin_seed(pi, coin)
    keep = []

    def build_extension(challenges):
        for m in keep:
            m.close()
        keep[:] = [hostlib.build_extension_columns(ctx, layout, [cols[c] for c in aux], n, challenges)]
        return keep[-1].cols
    out = {}
    for blowup, queries in pairs:
        opt = ProofOptions(num_queries=queries, lde_blowup_factor=blowup)
        rec = {}
        try:
            for timed in (False, True):
                sys.stderr.write("[lde step] blowup %d %s\n" % (blowup, "timed" if timed else "warm-up"))
                sys.stderr.flush()
                ctx.sync()
                t0 = time.perf_counter()
                raw = hostlib.prove(ctx, air, tree_kind, nf, coin, seed, cols, log_n, build_extension, opt, wire=True)
                ctx.sync()
                rec = {"total_ms": 1e3 * (time.perf_counter() - t0), "proof_bytes": len(raw)}
        except Exception as e:                                 # noqa: BLE001
            # only the allocator's refusal is a result (and the larger factors behind it are not tried); any other error - a HIP
            # error after a fault among them - ends the step with a non-zero exit and nothing more started on the device
            if "out of memory" not in str(e).lower():
                raise
            out[str(blowup)] = {"error": str(e)[:300]}
            break
        out[str(blowup)] = rec
        ctx.trim()
    print(json.dumps({"ncols": len(cols) + air.num_extension_columns, "n": n, "pairs": out}))
    for m in keep:
        m.close()
    air.close()
    ctx.close()


def stages_of(stderr_text):
    """-> {blowup: {stage: ms}} of the TIMED proofs in a step's stderr"""
    out, cur = {}, None
    for line in stderr_text.splitlines():
        m = re.match(r"\[lde step\] blowup (\d+) (timed|warm-up)", line)
        if m:
            cur = out.setdefault(m.group(1), {}) if m.group(2) == "timed" else None
            continue
        m = STAGE.search(line)
        if m and cur is not None:
            cur[m.group(1).strip()] = cur.get(m.group(1).strip(), 0.0) + float(m.group(2))
    return out


def main(argv):
    if argv[:1] == ["--step"]:
        step(argv[1], argv[2], int(argv[3]), [tuple(int(v) for v in p.split(":")) for p in argv[4].split(",")])
        return 0
    opt = {"--parent": None, "--log-steps": "20", "--rounds": "5", "--limit": "420", "--max-log-rows": "27", "--out": os.path.join(ROOT, "profiles", "lde_blowup_factors.json")}
    for k in range(0, len(argv), 2):
        if argv[k] not in opt or k + 1 >= len(argv):
            print(__doc__)
            return 2
        opt[argv[k]] = argv[k + 1]
    if not opt["--parent"] or not os.path.exists(os.path.join(opt["--parent"], "sandstorm_amd", "_build", "libsandstorm_host.so")):
        print("--parent DIR: a checkout of the parent commit with its libraries built")
        return 2
    log_steps, rounds, limit = int(opt["--log-steps"]), int(opt["--rounds"]), int(opt["--limit"])
    fits = [p for p in PAIRS if log_steps + 4 + p[0].bit_length() - 1 <= int(opt["--max-log-rows"])]
    trees = (("parent", os.path.abspath(opt["--parent"]), PAIRS[:1]), ("this", ROOT, fits))
    record = {"log_steps": log_steps, "rounds_asked": rounds, "layouts": {}, "ended_early": None,
              "not_run": ["blowup %d: 2^%d rows > 2^%s" % (p[0], log_steps + 4 + p[0].bit_length() - 1, opt["--max-log-rows"]) for p in PAIRS if p not in fits],
              "how": "tools/lde_blowup_timing.py: parent and this build alternated per round, one process per (round, tree, layout), columns resident, "
                     "one untimed and one timed proof per factor, SSH_TIMING stage clocks (device sync at every boundary)"}
    raw = {lay: {name: {} for name, _, _ in trees} for lay in ("starknet", "recursive")}
    shape = {}
    for rnd in range(rounds):
        for layout in ("starknet", "recursive"):
            for name, tree, pairs in trees:
                if record["ended_early"]:
                    break
                cmd = [sys.executable, os.path.abspath(__file__), "--step", tree, layout, str(log_steps), ",".join("%d:%d" % p for p in pairs)]
                try:
                    res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=dict(os.environ, SSH_TIMING="1"), cwd=tree)
                except subprocess.TimeoutExpired:
                    record["ended_early"] = "round %d %s %s: time limit of %d s" % (rnd, name, layout, limit)
                    break
                if res.returncode != 0:
                    record["ended_early"] = "round %d %s %s: exit status %d: %s" % (rnd, name, layout, res.returncode, res.stderr[-400:])
                    break
                got = json.loads(res.stdout.strip().splitlines()[-1])
                shape[layout] = {"ncols": got["ncols"], "n": got["n"]}
                stages = stages_of(res.stderr)
                for blowup, rec in got["pairs"].items():
                    slot = raw[layout][name].setdefault(blowup, {"total_ms": [], "proof_bytes": None, "stages_ms": {}, "errors": []})
                    if "error" in rec:
                        slot["errors"].append(rec["error"])
                        continue
                    slot["total_ms"].append(round(rec["total_ms"], 3))
                    slot["proof_bytes"] = rec["proof_bytes"]
                    for st, ms in stages.get(blowup, {}).items():
                        slot["stages_ms"].setdefault(st, []).append(ms)
                print("round %d %s %s: %s" % (rnd, layout, name, {b: round(r.get("total_ms", -1)) for b, r in got["pairs"].items()}), flush=True)
    med = lambda v: sorted(v)[len(v) // 2] if v else None
    for layout, by_tree in raw.items():
        par, this = by_tree["parent"].get("2"), by_tree["this"]
        summary = {"raw": by_tree}
        if par and par["total_ms"] and this.get("2", {}).get("total_ms"):
            spread = max(par["total_ms"]) - min(par["total_ms"])
            q_par = par["stages_ms"].get("quotient", [])
            q_spread = max(q_par) - min(q_par) if q_par else None
            summary["blowup2_total"] = {"parent_median_ms": med(par["total_ms"]), "this_median_ms": med(this["2"]["total_ms"]), "parent_spread_ms": round(spread, 3),
                                        "no_slower_beyond_the_spread": med(this["2"]["total_ms"]) <= med(par["total_ms"]) + spread}
            summary["quotient_stage"], summary["subsample"], summary["totals"] = {}, {}, {}
            for blowup, slot in sorted(this.items(), key=lambda kv: int(kv[0])):
                if not slot["total_ms"]:
                    summary["totals"][blowup] = {"errors": slot["errors"]}
                    continue
                summary["totals"][blowup] = {"queries": dict(PAIRS)[int(blowup)], "total_median_ms": med(slot["total_ms"]), "proof_bytes": slot["proof_bytes"]}
                if blowup == "2" or not q_par:
                    continue
                sub, quo = slot["stages_ms"].get("subsample", []), slot["stages_ms"].get("quotient", [])
                allowed = med(q_par) + med(sub) + q_spread
                summary["quotient_stage"][blowup] = {"parent_blowup2_quotient_median_ms": med(q_par), "parent_spread_ms": round(q_spread, 3), "subsample_median_ms": med(sub),
                                                     "constraint_kernels_median_ms": med(quo), "subsample_plus_kernels_ms": round(med(sub) + med(quo), 3),
                                                     "within_allowance": med(sub) + med(quo) <= allowed}
                written = shape[layout]["ncols"] * 2 * shape[layout]["n"] * 32
                summary["subsample"][blowup] = {"log_stride": int(blowup).bit_length() - 2, "median_ms": med(sub), "bytes_written": written,
                                                "written_GB_per_s": round(written / (med(sub) * 1e-3) / 1e9, 1) if med(sub) else None,
                                                "share_of_proof": round(med(sub) / med(slot["total_ms"]), 4)}
        record["layouts"][layout] = summary
    with open(opt["--out"], "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": opt["--out"], "ended_early": record["ended_early"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
