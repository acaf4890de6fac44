"""The N > 1 paths on hardware: reads shard by index, each rank (or device) works on a full index replica,
the only exchange is one all-reduce (sum) of the per-site counters, min(63, .) afterwards.

What a one-GPU box can run: RCCL itself through the library's multi-device entry point with one device (the identity, but
it goes through dlopen, ncclCommInitAll, ncclAllReduce with the library's data type / operator and the handle's stream);
two RANKS sharing the GPU over gloo through GenoIndex.counts_tensor() / all_reduce_counts(); bench.py --gpus 2 starting its
own ranks.  With two or more GPUs visible the same tests run over RCCL proper (ranks on distinct devices; the CLI with
VARGENO_GPUS=2)."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import BIN, GOLDEN, ROOT
from oracle import oracle as O
from vargeno_amd.api import GenoIndex, all_reduce_devices

pytestmark = pytest.mark.gpu


def _oracle(prefix, r, times=1):
    ox = O.OracleIndex.load(prefix)
    for _ in range(times):
        ox.process(r.bases, r.quals, r.offsets)
    return ox.sites()


def test_rccl_allreduce_over_one_device_is_the_identity(ftiny_dir, ftiny_reads):
    prefix = os.path.join(ftiny_dir, "idx")
    so = _oracle(prefix, ftiny_reads)
    with GenoIndex.open(prefix) as gx:
        gx.submit(ftiny_reads.bases, ftiny_reads.quals, ftiny_reads.offsets)
        before = gx.counts_tensor().clone()
        all_reduce_devices([gx])
        assert torch.equal(gx.counts_tensor(), before)
        rc, ac = gx.counts()
    assert np.array_equal(rc, so["ref_cnt"]) and np.array_equal(ac, so["alt_cnt"])


def test_replicas_sharing_a_device_sum_like_one(ftiny_dir, ftiny_reads):
    """Two replicas of the index (each holds the 80 GiB of jump + direct tables whatever the genome's size, so two is what a
    288 GB device takes), uneven shards of the reads, seven passes each (the exact sums pass 63): after
    vg_counts_allreduce_devices every replica holds the counters of one replica on all reads.  With one GPU the two share it
    (summed on the device, the first goes through RCCL alone); with two they sit on both (RCCL proper)."""
    prefix = os.path.join(ftiny_dir, "idx")
    so = _oracle(prefix, ftiny_reads, times=7)
    ndev = torch.cuda.device_count()
    r = ftiny_reads
    cuts = [0, r.n // 3, r.n]
    gxs = [GenoIndex.open(prefix, device=k % ndev) for k in range(2)]
    try:
        for k, gx in enumerate(gxs):
            sub = r.slice(cuts[k], cuts[k + 1])
            for _ in range(7):
                gx.submit(sub.bases, sub.quals, sub.offsets)
        all_reduce_devices(gxs)
        raw0 = gxs[0].counts_tensor().clone().cpu()
        assert int(raw0.max()) > 63
        for gx in gxs:
            assert torch.equal(gx.counts_tensor().cpu(), raw0)
            rc, ac = gx.counts()
            assert np.array_equal(rc, so["ref_cnt"]) and np.array_equal(ac, so["alt_cnt"])
    finally:
        for gx in gxs:
            gx.close()


@pytest.mark.parametrize("replicas", [1, 2])
def test_cli_counters_through_rccl_give_the_golden_vcf(ftiny_dir, tmp_path, replicas):
    """`vargeno geno` with VARGENO_GPUS replicas: chunks of the FASTQ go round robin, the counters meet in one all-reduce.  On a
    one-GPU box the replicas share the device (VARGENO_SHARE_DEVICES), with more they sit on distinct ones."""
    env = dict(os.environ, VARGENO_GPUS=str(replicas), VARGENO_SHARE_DEVICES="1", VARGENO_FORCE_RCCL="1", VARGENO_BATCH="500", VARGENO_CHUNK_MB="1")
    p = subprocess.run([BIN, "geno", os.path.join(ftiny_dir, "idx"), os.path.join(ftiny_dir, "reads.fq"), os.path.join(ftiny_dir, "snps.vcf"), str(tmp_path / "out.vcf")],
                       env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert open(tmp_path / "out.vcf", "rb").read() == gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read()


_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
rank, world, prefix, out, backend, times = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5])
import numpy as np, torch, torch.distributed as dist
from vargeno_amd import synth
from vargeno_amd.api import GenoIndex, all_reduce_counts, shard_range
dev = rank % torch.cuda.device_count() if backend == "nccl" else 0
torch.cuda.set_device(dev)
if backend == "nccl":
    dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
else:
    dist.init_process_group(backend)
r = synth.f_tiny()[2]
lo, hi = shard_range(r.n, rank, world)
sub = r.slice(lo, hi)
with GenoIndex.open(prefix, device=dev) as gx:
    gx.set_stats(False)
    for _ in range(times):
        gx.submit(sub.bases, sub.quals, sub.offsets)
    gx.sync()
    import time
    t0 = time.perf_counter()
    all_reduce_counts(gx)
    # (so that the first run on a box with two GPUs explains itself: what the exchange moved, how long it took, over what)
    print("rank %d of %d on cuda:%d, backend %s: all-reduce of %d bytes in %.3f ms" % (rank, dist.get_world_size(), dev, backend, gx.counts_tensor().numel() * 4, 1e3 * (time.perf_counter() - t0)), flush=True)
    rc, ac = gx.counts()
    raw = gx.counts_tensor().clone().cpu().numpy()
np.savez(os.path.join(out, "rank%d.npz" % rank), rc=rc, ac=ac, raw=raw)
dist.barrier()
dist.destroy_process_group()
'''


def _run_ranks(tmp_path, prefix, backend, times):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    port = 29600 + os.getpid() % 1500
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           str(script), ROOT, prefix, str(tmp_path), backend, str(times)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    print(p.stdout[-1500:])
    assert p.stdout.count("all-reduce of") == 2
    return [np.load(tmp_path / ("rank%d.npz" % k)) for k in range(2)]


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_two_ranks_shard_and_all_reduce_equal_one_rank(backend, ftiny_dir, ftiny_reads, tmp_path):
    """Two processes, each with its own index replica, each on its shard of the reads, 7 passes so that the 6-bit clamp
    matters; after GenoIndex.counts_tensor() / all_reduce_counts() every rank holds the counters of one rank on all
    reads.  gloo: both ranks share GPU 0 (any box); nccl = RCCL: needs two GPUs."""
    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs, found %d (RCCL refuses two ranks on one device)" % torch.cuda.device_count())
    prefix = os.path.join(ftiny_dir, "idx")
    so = _oracle(prefix, ftiny_reads, times=7)
    got = _run_ranks(tmp_path, prefix, backend, 7)
    for g in got:
        assert np.array_equal(g["rc"], so["ref_cnt"]) and np.array_equal(g["ac"], so["alt_cnt"])
        assert np.array_equal(g["raw"], got[0]["raw"])
    assert got[0]["rc"].max() == 63 and got[0]["raw"].max() > 63           # exact sums cross the ranks, the clamp comes after


def test_bench_starts_its_own_ranks(tmp_path):
    """`bench.py --gpus 2` with no launcher around it must run two ranks (not one), check the sharded path against one
    rank, and report the rank count the collective saw.  Two GPUs: RCCL; one GPU: the ranks share it over gloo."""
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    env = dict(os.environ, VG_BENCH_BACKEND=backend, VG_BENCH_DIR=str(tmp_path), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--workload", "chr22", "--genome", "3000000", "--snps", "30000",
                        "--reads", "20000", "--batches", "2", "--steps", "3", "--warmup", "1", "--cpu-sample", "0", "--no-gather-probe"],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stderr[-4000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["steps"] == 3
    v = line["multi_gpu_verification"]
    assert v["sharded_equals_single_rank"] and v["increments"] > 0 and v["timed_region_increments"] > 0
    assert line["value"] > 0 and line["roofline"]["frac"] > 0
    pr = line["multi_gpu_per_rank"]                                      # what every rank saw: a scaling run explains itself
    assert len(pr["kernel_ms"]) == 2 and len(pr["all_reduce_ms"]) == 2 and pr["all_reduce_bytes"] > 0 and pr["ranks_seen_by_the_collective"] == 2


def test_allreduce_with_the_callers_own_communicator(ftiny_dir, ftiny_reads):
    """vg_counts_allreduce(handle, ncclComm_t): a caller that owns its RCCL communicator (one process per GPU without torch).
    One rank is all a one-GPU box can host: ncclCommInitRank(nranks = 1) through ctypes, the all-reduce is the identity."""
    import ctypes as C

    from vargeno_amd._lib import check, lib

    rccl = None
    for name in ("librccl.so.1", "librccl.so", os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")):
        try:
            rccl = C.CDLL(name, mode=C.RTLD_GLOBAL)
            break
        except OSError:
            continue
    if rccl is None:
        pytest.skip("librccl not found")

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]

    uid = UniqueId()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    prefix = os.path.join(ftiny_dir, "idx")
    with GenoIndex.open(prefix) as gx:
        assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
        gx.submit(ftiny_reads.bases, ftiny_reads.quals, ftiny_reads.offsets)
        before = gx.counts_tensor().clone()
        assert int(before.sum()) > 0
        check(lib().vg_counts_allreduce(gx._h, comm))
        assert torch.equal(gx.counts_tensor(), before)
        rccl.ncclCommDestroy.argtypes = [C.c_void_p]
        rccl.ncclCommDestroy(comm)


# ---- rehearsal of the target's rank count on whatever the box has -------------------------------------------------------------------
# Eight replicas of an index fit one 288 GB device once the optional views are off (what stays is the 16 GiB jump table of the
# reference dictionary + scratch, ~20 GB per replica): the 8-way shard arithmetic, rank 0's index build with the others waiting
# for its marker, eight vg_index_open of the same files at once and the CLI's eight-range cut of the FASTQ file all run.
# With 8 GPUs visible the same tests take RCCL (one rank / replica per device) without a change.
LEAN = {"VG_NO_MX": "1", "VG_NO_SNP_JG32": "1", "VG_NO_SEC": "1", "VG_NO_PROBE_VIEW": "1"}


def test_bench_with_eight_ranks(tmp_path):
    backend = "nccl" if torch.cuda.device_count() >= 8 else "gloo"
    env = dict(os.environ, VG_BENCH_BACKEND=backend, VG_BENCH_DIR=str(tmp_path), HSA_ENABLE_IPC_MODE_LEGACY="0", **LEAN)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "8", "--workload", "chr22", "--genome", "3000000", "--snps", "30000",
                        "--reads", "20000", "--batches", "2", "--steps", "3", "--warmup", "1", "--cpu-sample", "0", "--no-gather-probe"],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stderr[-4000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 8 and line["steps"] == 3
    v = line["multi_gpu_verification"]
    assert v["sharded_equals_single_rank"] and v["increments"] > 0 and v["timed_region_increments"] > 0
    assert line["value"] > 0
    # every replica's start-up, as it ran beside the seven others: wall and host CPU seconds (round-4 verdict, item 8a)
    pr = line["multi_gpu_per_rank"]
    assert len(pr["index_open_s"]) == 8 and len(pr["index_open_cpu_s"]) == 8 and min(pr["index_open_s"]) > 0
    print("eight replicas, vg_index_open wall s: %s | host CPU s: %s | device GB: %s" % (["%.2f" % x for x in pr["index_open_s"]], ["%.2f" % x for x in pr["index_open_cpu_s"]], ["%.1f" % x for x in pr["index_device_GB"]]))


def test_cli_with_eight_replicas_gives_the_golden_vcf(ftiny_dir, tmp_path):
    """Eight contiguous record-aligned ranges of the FASTQ file, one per replica, all streamed at once; one all-reduce."""
    env = dict(os.environ, VARGENO_GPUS="8", VARGENO_SHARE_DEVICES="1", VARGENO_CHUNK_MB="1", **LEAN)
    p = subprocess.run([BIN, "geno", os.path.join(ftiny_dir, "idx"), os.path.join(ftiny_dir, "reads.fq"), os.path.join(ftiny_dir, "snps.vcf"), str(tmp_path / "out.vcf")],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr
    assert "framed on the host" not in p.stderr, p.stderr            # the eight ranges went through the device-side framing
    assert open(tmp_path / "out.vcf", "rb").read() == gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read()


def test_cli_with_four_full_replicas_sharing_one_device(ftiny_dir, tmp_path):
    """Replicas that share a device share its memory: without a budget of its own each gets an equal part (vg_share_budget) and
    plans its views for that -- four replicas with every optional view on used to plan for the whole device each, and the third
    or fourth one failed with VG_ENOMEM (round 4's advisor).  Same VCF as one replica."""
    if torch.cuda.device_count() >= 4:
        pytest.skip("needs replicas that SHARE a device")
    # (r06: a small index gets small tables -- four F-tiny replicas would all fit whole; the 2^32-entry forms of an hg38-scale index,
    # ~90 GB per replica, are forced so that the shares bite)
    env = dict(os.environ, VARGENO_GPUS="4", VARGENO_SHARE_DEVICES="1", VARGENO_CHUNK_MB="1", VARGENO_VERBOSE="1", VG_DX_BITS="32", VG_REF_JG_BITS="32")
    p = subprocess.run([BIN, "geno", os.path.join(ftiny_dir, "idx"), os.path.join(ftiny_dir, "reads.fq"), os.path.join(ftiny_dir, "snps.vcf"), str(tmp_path / "out.vcf")],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr
    assert "vg_index_open_ex" in p.stderr and "LEFT OUT for the budget" in p.stderr, p.stderr      # each replica planned within its share
    assert open(tmp_path / "out.vcf", "rb").read() == gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read()
