"""One rank = one PROCESS of a files -> proof call sharded by the C++ host (host_capi.cpp ssh_prove_files_sharded_device): launched under
torch.distributed.run by tests/test_gpu_sharded_files.py.  Every process reads the reference's example run (tests/golden/example, 2^14
steps) itself, makes the base trace on its device and meets the others in the driver's CallbackTransport over gloo; the claim is the
CLI's for the recursive layout (FriendlyMerkleTree<22> + the Cairo coin).

argv: out_path - rank 0 writes the proof (reference wire format) there."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_path = sys.argv[1]
    world = int(os.environ["WORLD_SIZE"])
    emulated = os.environ.get("SS_TEST_HIPEMU") == "1"
    if emulated:
        # the emulator spreads a launch's workgroups over OS threads: the ranks are the parallelism here
        os.environ.setdefault("HIPEMU_THREADS", str(max(1, (os.cpu_count() or 1) // world)))
        os.environ.setdefault("SS_PED_WINDOW", "16")
        os.environ.setdefault("SS_PED_SMALL_MAX", "128")
    import torch                                             # noqa: F401 - before the library: one HIP runtime per process
    import torch.distributed as dist
    from sandstorm_amd import _lib
    if emulated:
        _lib.LIB_PATH = os.environ.get("SS_TEST_HIPEMU_LIB", os.path.join(ROOT, "tests", "hipemu", "_build", "libsandstorm_hipemu.so"))
    from sandstorm_amd import backend as be, hostlib, public_input
    dist.init_process_group(backend="gloo")
    rank = dist.get_rank()
    assert dist.get_world_size() == world
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "example", "trace.bin"), "rb") as f:
        trace_bin = f.read()
    with open(os.path.join(gold, "example", "memory.bin"), "rb") as f:
        memory_bin = f.read()
    pi = public_input.AirPublicInput.from_json(os.path.join(gold, "air_public_input_array_sum.json"))
    log_n = (len(trace_bin) // 24).bit_length() - 1 + 4
    ctx = be.Context(0)
    air = hostlib.RecursiveHostAir(ctx, pi, log_n, 1)
    group = hostlib.torch_dist_group()
    try:
        proof, times = hostlib.prove_files_sharded_device(ctx, "recursive", trace_bin, memory_bin, pi, None, air, be.TREE_FRIENDLY, 22, be.COIN_CAIRO,
                                                          public_input.public_coin_seed(pi, be.COIN_CAIRO), rank, world, group)
        assert (proof is not None) == (rank == 0) and 0 < times["trace_gen_s"] <= times["total_s"]
    finally:
        group.close()
        air.close()
    if rank == 0:
        with open(out_path, "wb") as f:
            f.write(proof)
        print("SHARDED_PROOF_WRITTEN")
    dist.barrier()
    ctx.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
