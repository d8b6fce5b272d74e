"""What the host-made base trace of the 64-bit field's claim costs next to its proof, and what making it on the device leaves of that: the
plain layout's example run padded to 2^log_steps steps (BASELINE.json configs[4]; 2^20 by default), CLI-default options, one visit of
the card.  After asserting that the device's five columns equal layouts/plain.py base_trace_np's cell for cell, and one warm-up of
each path, the three paths ALTERNATE `reps` times (host clock around work that ends in a device synchronise):
  (a) host_path_s    the path before this tool existed: base_trace_np on the host (from the parsed run), the upload of its five columns,
                     goldilocks.Prover.prove; its three parts are listed too
  (b) files_s        goldilocks.prove_files: ONE call from the bytes of trace.bin / memory.bin to the proof (ssh_gl_prove_files_device)
  (c) proof_s        the proof alone, columns resident: hostlib.gl_prove (the C++ host (b) proves with); python_proof_s is
                     Prover.prove alone, the prover of (a)
and the bytes each uploads.  (b) / (c) is the figure to read beside the 252-bit path's 1.024 - 1.026 (files -> proof over the proof alone).
  python tools/gl64_device_trace_timing.py [--log-steps 20] [--reps 5] [--out profiles/gl64_plain_device_trace.json]
prints ONE JSON line (medians, spread, the raw lists) and writes it to --out.  No fallback: without a GPU it fails."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}


def main(log_steps, reps, out_path):
    import numpy as np
    import torch
    from sandstorm_amd import backend as be, binary as bn, goldilocks as gs, hostlib
    from sandstorm_amd.layouts import plain as pl
    prog = pl.example_program(10)
    states, memory = pl.run(prog, 64)
    states = list(states) + [states[-1]] * ((1 << log_steps) - len(states))
    pi = pl.public_input_of(prog, states, memory)
    trace_bin, memory_bin = bn.write_register_states(states), bn.write_memory(memory)
    n = 16 << log_steps
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = be.Context(0, stream=stream.cuda_stream)
    air, opt, seed = gs.plain_air(), gs.Options(), bytes(range(32))
    sync = lambda: (torch.cuda.synchronize(dev), ctx.sync())

    # the device's columns are the host's, cell for cell
    want = pl.base_trace_np(states, memory, pi)
    resident = gs.plain_base_trace_on_device(ctx, trace_bin, memory_bin, pi)
    device_bytes = hostlib.gl_trace_last_stats()["bytes_uploaded"]
    for c, w in zip(resident, want):
        assert np.array_equal(c.cpu().numpy().view(np.uint64), w), "the device's columns are not base_trace_np's"
    del want

    def host_path():
        t0 = time.perf_counter()
        cols = pl.base_trace_np(states, memory, pi)
        t1 = time.perf_counter()
        base = [torch.from_numpy(c.view(np.int64)).to(dev) for c in cols]
        sync()
        t2 = time.perf_counter()
        gs.Prover(ctx, air, opt).prove(seed, base, lambda ch: gs.plain_extension_on_device(ctx, base, ch)[0], statement=pi)
        sync()
        t3 = time.perf_counter()
        return {"host_path_s": t3 - t0, "host_trace_s": t1 - t0, "upload_s": t2 - t1, "python_prove_after_upload_s": t3 - t2}

    scratch = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(5)]

    def files_path():
        sync()
        t0 = time.perf_counter()
        _, times = gs.prove_files(ctx, trace_bin, memory_bin, pi, seed, opt, out=scratch, want_times=True)
        sync()
        return {"files_s": time.perf_counter() - t0, "files_trace_gen_s": times["trace_gen_s"]}

    def proof_alone():
        sync()
        t0 = time.perf_counter()
        hostlib.gl_prove(ctx, air, opt, seed, resident, lambda ch: gs.plain_extension_on_device(ctx, resident, ch)[0], statement=pi)
        sync()
        t1 = time.perf_counter()
        gs.Prover(ctx, air, opt).prove(seed, resident, lambda ch: gs.plain_extension_on_device(ctx, resident, ch)[0], statement=pi)
        sync()
        return {"proof_s": t1 - t0, "python_proof_s": time.perf_counter() - t1}

    raw = {}
    for it in range(reps + 1):                                        # (the first pass warms every path up and is dropped)
        for path in (host_path, files_path, proof_alone):
            for k, v in path().items():
                if it:
                    raw.setdefault(k, []).append(v)
    result = {"workload": "plain layout, example run padded to 2^%d steps (n = 2^%d rows), CLI-default options" % (log_steps, log_steps + 4),
              "reps": reps, "device": torch.cuda.get_device_name(0),
              "bytes_uploaded": {"host_path_columns": 5 * 8 * n, "files_path": device_bytes, "trace_bin": len(trace_bin), "memory_bin": len(memory_bin)},
              "seconds": {k: spread(v) for k, v in raw.items()}, "raw_seconds": raw}
    m = lambda k: result["seconds"][k]["median"]
    result["files_over_proof"] = m("files_s") / m("proof_s")
    result["host_path_over_python_proof"] = m("host_path_s") / m("python_proof_s")
    ctx.close()
    line = json.dumps(result)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    opt = lambda name, default, kind=int: kind(argv[argv.index(name) + 1]) if name in argv else default
    sys.exit(main(opt("--log-steps", 20), opt("--reps", 5), opt("--out", os.path.join(ROOT, "profiles", "gl64_plain_device_trace.json"), str)))
