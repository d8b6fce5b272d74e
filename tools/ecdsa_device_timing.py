"""What the ECDSA builtin's device path (hostlib.trace_ecdsa_on_device) costs and saves on a starknet statement whose ECDSA slots all hold
a distinct honest signature (examples.seeded_ecdsa_instances: 64 at 2^17 steps, 512 at 2^20): the switch off and on ALTERNATED, `rounds`
times, in one visit of the card - per round and setting `proofs` calls of the device generator alone and of prove_files_device (files ->
proof), the proof alone on the resident columns once per round, and the host's share for the keys' square roots as SSH_TRACE_TIMING
reports it.  WITHOUT torch.
  python tools/ecdsa_device_timing.py [log_steps ...] [--rounds 3] [--proofs 10] [--limit SECONDS]
prints ONE JSON line: per log_steps the raw lists (seconds) and their medians.  Every round runs in a process of its own under its own
time limit (--limit, 600 s); a round that fails or runs out of time ends the measurement there, and the line says so.
  python tools/ecdsa_device_timing.py --generate LOG_STEPS
one device generation with the switch on and nothing else: what to put behind `rocprofv3 --kernel-trace --stats --` for
trace_ecdsa_kernel's own time."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def statement(log_steps):
    from sandstorm_amd import binary, examples, hostlib
    states, memory, xpi = examples.starknet_example(log_steps)
    trace_bin, memory_bin = binary.write_register_states(states), binary.write_memory(memory)
    rows = examples.seeded_ecdsa_instances(examples.ecdsa_slots(log_steps))
    return trace_bin, memory_bin, xpi, {"ecdsa": hostlib.pack_instances("ecdsa", rows)}, len(rows)


def generate(log_steps):
    from sandstorm_amd import backend as be, hostlib
    trace_bin, memory_bin, xpi, priv, count = statement(log_steps)
    ctx = be.Context(0)
    hostlib.trace_ecdsa_on_device(True)
    cols = hostlib.device_base_trace(ctx, "starknet", trace_bin, memory_bin, xpi, priv)
    ctx.sync()
    stats = hostlib.trace_last_stats()
    assert stats["ecdsa_on_device"] == count, stats
    for c in cols:
        c.free()
    ctx.close()


def one_round(log_steps, proofs):
    """the switch off, then on: -> {"off": {...}, "on": {...}, "prove_s": [...]} as one JSON line on stdout"""
    from sandstorm_amd import backend as be, hostlib, public_input
    from sandstorm_amd.layouts import starknet as sk
    from sandstorm_amd.prover import ProofOptions
    trace_bin, memory_bin, xpi, priv, count = statement(log_steps)
    log_n = log_steps + 4
    n = 1 << log_n
    ctx = be.Context(0)
    air = hostlib.StarknetHostAir(ctx, xpi, log_n, 1)
    seed = public_input.public_coin_seed(xpi, be.COIN_SOLIDITY)
    dev = [ctx.alloc(32 * n) for _ in range(9)]
    keep = []

    def build_extension(challenges):
        for m in keep:
            m.close()
        del keep[:]
        keep.append(hostlib.build_extension_columns(ctx, "starknet", [dev[c] for c in (sk.COL_NPC, sk.COL_MEMORY, sk.COL_RANGE_CHECK)], n, challenges))
        return keep[0].cols
    options = ProofOptions()
    args = (be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY, seed)
    out = {"instances": count}
    for name, on in (("off", False), ("on", True)):
        hostlib.trace_ecdsa_on_device(on)
        gen_s, total_s, inner = [], [], []
        for it in range(proofs + 1):                                  # (the first call of each loop warms up and is dropped)
            ctx.sync()
            t0 = time.perf_counter()
            hostlib.device_base_trace(ctx, "starknet", trace_bin, memory_bin, xpi, priv, dev)
            ctx.sync()
            if it:
                gen_s.append(time.perf_counter() - t0)
        stats = hostlib.trace_last_stats()
        assert stats["ecdsa_on_device"] == (count if on else 0) and stats["ecdsa_on_host"] == (0 if on else count), stats
        for it in range(proofs + 1):
            ctx.sync()
            t0 = time.perf_counter()
            _, tm = hostlib.prove_files_device(ctx, "starknet", trace_bin, memory_bin, xpi, priv, dev, air, *args, build_extension, options, want_proof=False)
            ctx.sync()
            if it:
                total_s.append(time.perf_counter() - t0)
                inner.append(tm["trace_gen_s"])
        out[name] = {"gen_s": gen_s, "total_s": total_s, "trace_gen_s": inner, "bytes_uploaded": stats["bytes_uploaded"], "templates_uploaded": stats["templates_uploaded"]}
        if on:                                                        # the host's steps of three more generations on stderr, for the caller to read
            os.environ["SSH_TRACE_TIMING"] = "1"
            for _ in range(3):
                hostlib.device_base_trace(ctx, "starknet", trace_bin, memory_bin, xpi, priv, dev)
                ctx.sync()
            del os.environ["SSH_TRACE_TIMING"]
    prove_s = []
    for it in range(proofs + 1):
        ctx.sync()
        t0 = time.perf_counter()
        hostlib.prove(ctx, air, *args, dev, log_n, build_extension, options, want_proof=False)
        ctx.sync()
        if it:
            prove_s.append(time.perf_counter() - t0)
    out["prove_s"] = prove_s
    for m in keep:
        m.close()
    air.close()
    for d in dev:
        d.free()
    ctx.close()
    print(json.dumps(out), flush=True)


def median(v):
    return sorted(v)[len(v) // 2] if v else None


def main(sizes, rounds, proofs, limit):
    result = {"rounds": rounds, "proofs_per_round_and_setting": proofs, "sizes": {}}
    for log_steps in sizes:
        acc = {"off": {"gen_s": [], "total_s": [], "trace_gen_s": []}, "on": {"gen_s": [], "total_s": [], "trace_gen_s": []}, "prove_s": [], "roots_ms": []}
        for r in range(rounds):
            try:
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--round", str(log_steps), str(proofs)], capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                result["stopped"] = "2^%d steps, round %d: ran out of its %d s" % (log_steps, r, limit)
                break
            if child.returncode != 0:
                result["stopped"] = "2^%d steps, round %d: exit status %d: %s" % (log_steps, r, child.returncode, child.stderr[-400:])
                break
            got = json.loads(child.stdout.strip().splitlines()[-1])
            for name in ("off", "on"):
                for key in ("gen_s", "total_s", "trace_gen_s"):
                    acc[name][key] += got[name][key]
                acc[name]["bytes_uploaded"], acc[name]["templates_uploaded"] = got[name]["bytes_uploaded"], got[name]["templates_uploaded"]
            acc["prove_s"] += got["prove_s"]
            acc["instances"] = got["instances"]
            acc["roots_ms"] += [float(v) for v in re.findall(r"\[device trace\] ecdsa roots\s+([0-9.]+) ms", child.stderr)]
        acc["median"] = {"gen_off_s": median(acc["off"]["gen_s"]), "gen_on_s": median(acc["on"]["gen_s"]), "total_off_s": median(acc["off"]["total_s"]),
                         "total_on_s": median(acc["on"]["total_s"]), "prove_s": median(acc["prove_s"]), "roots_ms": median(acc["roots_ms"])}
        if acc["median"]["prove_s"]:
            acc["median"]["total_over_prove_off"] = acc["median"]["total_off_s"] / acc["median"]["prove_s"]
            acc["median"]["total_over_prove_on"] = acc["median"]["total_on_s"] / acc["median"]["prove_s"]
        result["sizes"][str(log_steps)] = acc
        if "stopped" in result:
            break
    print(json.dumps(result), flush=True)
    return 1 if "stopped" in result else 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--generate"]:
        generate(int(argv[1]))
    elif argv[:1] == ["--round"]:
        one_round(int(argv[1]), int(argv[2]))
    else:
        opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
        skip = {i + 1 for i, a in enumerate(argv) if a in ("--rounds", "--proofs", "--limit")}
        sizes = [int(a) for i, a in enumerate(argv) if a.isdigit() and i not in skip] or [17, 20]
        sys.exit(main(sizes, opt("--rounds", 3), opt("--proofs", 10), opt("--limit", 600)))
