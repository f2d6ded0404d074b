#!/usr/bin/env python3
"""bench.py — headers/sec of header_range witness generation on MI355X (BASELINE.json metric).

A "step" = one pass of the whole hot path (header hashing + hint assembly + prove_subchain + reduce + final
asserts + target-commit verification + Goldilocks witness expansion) over one batch of R synthetic header_range_2048
instances (32 map jobs x 64 headers, 100 validators, mode F = one commit per range, exactly what one reference proof
does) whose inputs are already resident in HBM.  The timed object is the C-ABI pipeline (`bsx_pipeline_step`,
csrc/pipeline.hip) — Python only calls it.  value = N * R * 2048 headers / step time, all ranks, max over ranks.

N > 1 (launched by torch.distributed.run, one rank per GPU over RCCL): every rank computes its 32/N-job slice of all
ranges, one all-gather of 128-byte records per pipelined chunk, the owner finishes its ranges.  --scaling weak (default):
R ranges per GPU (N * R in total); --scaling strong: R ranges in total, i.e. BASELINE config #4 literally (each
header_range_2048 split into N sub-ranges of 2048 / N headers).  Every rank re-proves a sample of its owned ranges with
an un-sharded pipeline on its own GPU and compares outputs, statuses, commit results, map-job records and a sampled
witness, so a wrong collective cannot go unnoticed.  --mode S: a commit on EVERY header (BASELINE config #5), the commits
sharded with their headers, one all-gather of 128-byte folds.

Every `peak` of an ALU-bound roofline is measured in THIS process on THIS device (`bsx_calibrate`, ~50 ms at start-up):
no constants carried over from another box.

stdout carries TWO lines (bench_legs/line.py; VERDICT r5 #1: round 5's single ~28 KB line could not be parsed by the driver):
    DETAIL {...}      the full object: every leg below with its notes (profiles/r6_bench_n1.json is this object)
    {...}             the LAST line, < 6 KB: the contract's keys, `config`, `roofline`, `cpu_baseline`, `long_run` and one or two numbers
                      per leg under `legs` (tests/test_bench_line.py holds its size and schema)
Progress goes to stderr.  The legs live in bench_legs/*.py (latency, stress, sweeps, commitment, cpu); this file keeps the headline path.

Objects of the full object beside the contract's keys (N = 1 unless noted):
  roofline            dominant kernel of the headline (witness expansion, HBM-write bound); also at N > 1
  calibration         the device ceilings measured at start-up
  kernels             the SHA kernels' compact-byte rates (never mixed with the expanded figure)
  cpu_baseline        the C oracle timed on this box's host cores on a bounded sample (rank 0; also at N > 1); also the
                      checker of the timed pipeline's outputs AND of the full Goldilocks witness of sampled ranges
                      (config.witness_checked_ranges).  oracle/ is imported only by the cpu_baseline* functions and the
                      `cpu_baseline` legs of stress / fused_commitment — always as the checker / CPU timing, never on the
                      measured GPU path
  compact_only        the same step without the Goldilocks expansion (fresh process): the ALU-bound rate of the SHA path
  stress              mode S: Ed25519 + SHA-512 bound, with its own `roofline` (bound "valu") and `cpu_baseline`
  latency             ONE range through the host tier (bsx_header_range, host pointers in, 64 B out)
  with_input_upload   the headline step with the headers streamed from pinned host memory every step (PCIe inclusive)
  fused_commitment    Poseidon Merkle caps of the witness straight from the compact bytes (no 64x image): the pipeline's
                      BSX_PIPE_CAPS mode (headers/s) and the kernel alone vs the materialised form
  header_range_1024   the metric's other production shape
"""
import argparse
import csv
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch
from bench_legs.common import *  # noqa: F401,F403,E402  (tools/*.py reach the legs through `bench.<name>`)
from bench_legs.common import HBM_PEAK_GBS, calibrate, log, memory_partition_mode, pmc_traffic  # noqa: E402
from bench_legs.cpu import cpu_baseline, cpu_baseline_witness_check  # noqa: E402
from bench_legs.stress import stress  # noqa: E402
from bench_legs.latency import latency_leg, concurrent_leg, hint_concurrent_leg, _concdrive  # noqa: E402,F401
from bench_legs.sweeps import range_sweep_leg, keyset_churn_leg, upload_leg  # noqa: E402
from bench_legs.commitment import commitment_leg  # noqa: E402
from bench_legs.line import DETAIL_PREFIX, compact_line, emit, detail_of  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-autotune", action="store_true", help="keep the pipeline's default stream assignment")
    ap.add_argument("--ranges", type=int, default=256, help="header_range instances per GPU per step (R); with --scaling strong: in total")
    ap.add_argument("--jobs", type=int, default=32)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--validators", type=int, default=100)
    ap.add_argument("--engines", type=int, default=2, help="chunks of the step pipelined on separate HIP streams inside the library (the "
                    "ALU-bound hashing of one chunk beside the HBM-bound expansion of the other)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--mode", choices=["F", "S"], default="F", help="F: one commit per range (a reference proof); S: a commit on every header")
    ap.add_argument("--wide-tables", choices=["auto", "0", "1"], default="auto", help="mode S: 16-bit digits in the key tables (BSX_COMMITS_KEYTABLE_WIDE; "
                    "auto = on)")
    ap.add_argument("--no-witness", action="store_true", help="skip the Goldilocks expansion (reported as such)")
    ap.add_argument("--caps", action="store_true", help="Poseidon Merkle caps of the map-job witnesses from the compact bytes (with --no-witness: instead of the expansion)")
    ap.add_argument("--alternate", type=int, default=1, help="K buffer sets inside the pipeline, step i on set i mod K (pipelining across steps; the compact-only leg uses 2)")
    ap.add_argument("--merkle-wgs", type=int, default=0, help="bsx_pipeline_config.tune_merkle_workgroups (experiments; 0 = automatic)")
    ap.add_argument("--subchain-form", type=int, default=0, help="bsx_pipeline_config.tune_subchain (experiments; 0 = automatic)")
    ap.add_argument("--no-commit", action="store_true", help="experiments: no target-commit verification (not a valid headline)")
    ap.add_argument("--no-units", action="store_true", help="A/B: do not materialise the COMMIT / SKIP units (BSX_PIPE_NO_UNITS: round 3's witness)")
    ap.add_argument("--only-leg", choices=["coalescing"], default=None, help="run ONE secondary leg in this (fresh) process and print its JSON: "
                    "`coalescing` = latency.concurrent + hint_concurrent (the parent runs it as a subprocess before it creates its own queues)")
    ap.add_argument("--long-steps", type=int, default=200, help="steps of the second, longer timed loop reported as `long_run` (0 = none)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-stress", action="store_true")
    ap.add_argument("--no-legs", action="store_true", help="headline only: none of the secondary objects")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--dry-run", action="store_true", help="launcher check only: spawn / join the ranks, one all-gather over the process group, "
                    "ONE JSON line with the world that really ran — no GPU work (CPU-only boxes: BSX_DIST_BACKEND=gloo)")
    ap.add_argument("--collective", choices=["rccl-c", "torch"], default="rccl-c", help="N > 1: the all-gather of the data path is ncclAllGather "
                    "called by the library (bsx_pipeline_set_rccl; default) or torch.distributed through a callback")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step computed "
                    "(rank 0: the pipeline's results, a fixed sample of every witness section) as DIR/<name>.npy, float32 / float64, <= 64 MB")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and (args.mode != "F" or args.only_leg or args.dry_run):
        ap.error("--dump-outputs dumps the headline path: mode F, no --only-leg / --dry-run")
    return args


def self_launch(args):
    """`python bench.py --gpus N` WITHOUT a launcher (no WORLD_SIZE in the environment): re-run this very command under
    torch.distributed.run with N ranks on this node, one per GPU, and hand its exit code on — so that the multi-GPU bench cannot
    silently run as N = 1.  Returns only when nothing had to be launched."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    if not args.dry_run and os.environ.get("BSX_BENCH_DEVICE") is None:
        n_dev = torch.cuda.device_count()
        if n_dev < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {n_dev} GPU(s) visible on this node")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"bench.py: no launcher in the environment — starting {args.gpus} ranks: {' '.join(cmd[1:9])} ...", file=sys.stderr, flush=True)
    raise SystemExit(subprocess.run(cmd, env=dict(os.environ, BSX_BENCH_SELF_LAUNCHED="1")).returncode)


def dry_run(args, rank, world):
    """--dry-run: the launcher contract without a GPU — every rank joins the process group, one all-gather of (rank, pid), rank 0
    prints what really ran."""
    import torch.distributed as dist
    ranks = [(rank, os.getpid())]
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(os.environ.get("BSX_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
        got = [None] * world
        dist.all_gather_object(got, (rank, os.getpid()))
        ranks = got
    assert world == args.gpus, f"--gpus {args.gpus} but {world} rank(s) are running"
    assert sorted(r for r, _ in ranks) == list(range(world)) and len({p for _, p in ranks}) == world
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "ranks": [r for r, _ in ranks], "processes": len({p for _, p in ranks}),
                          "launched_by": "bench.py itself" if os.environ.get("BSX_BENCH_SELF_LAUNCHED") else "the caller / an external launcher"}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()

def subprocess_leg(args, extra, timeout=900):
    cmd = [sys.executable, os.path.abspath(__file__), "--jobs", str(args.jobs), "--batch", str(args.batch), "--validators", str(args.validators),
           "--ranges", str(args.ranges), "--engines", str(args.engines), "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--no-legs"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        return None, out.stderr[-500:]
    return detail_of(out.stdout), None


def subprocess_legs(args):
    """The legs that run in processes of their own — BEFORE this process creates its first HIP queue: a parent that still holds its
    pipelines', contexts' and torch's streams (a hundred queues after the concurrency leg) makes the firmware time-slice the
    processes' queue sets, and the compact step measured beside it came out 12 % slow (372 M headers/s against 425-433 M alone)."""
    out = {}
    J, B = args.jobs, args.batch
    log("leg: compact_only (subprocess)")
    # one chunk per step: without an expansion to run beside there is nothing to pipeline against, and a chunk of 256
    # ranges quantises better (8196 header groups on 4096 wave slots) than two of 128
    # ... and two pipelines stepped in turn: step i + 1 starts while step i's chain of small kernels drains
    # 200 steps (0.26 s): a step's chain of dependent kernels spans two to three steps of the pipelined loop, so a 20-step
    # loop would spend a tenth of its time filling and draining (405 M headers/s at 20 steps, 423 M at 200 .. 6000)
    d, err = subprocess_leg(args, ["--no-witness", "--engines", "1", "--alternate", "2", "--steps", str(max(args.steps, 200))])
    out["compact_only"] = {"error": err} if d is None else {
        "workload": d["config"]["workload"], "value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"], "steps": d["steps"],
        "prove_subchain_ms": d["kernels"][0]["avg_launch_ms"], "sha256_compressions_per_s_prove_subchain": d["kernels"][0]["sha256_compressions_per_s"],
        "frac_of_measured_alu_peak_prove_subchain": d["kernels"][0]["frac_of_measured_alu_peak"],
        **d["compact_step"],
        "reference_equivalent_compressions_per_s_whole_step": d["value"] * (41 + 23),
        "note": "no Goldilocks expansion, one chunk per step, two buffer sets stepped in turn inside the pipeline (one header hashing at a time): header hashing (41 compressions/header) + prove_subchain + commit check "
                "(Ed25519, SHA-512) on the side stream; fractions are of the SHA-256 ceiling measured in that process"}
    log("leg: coalescing = latency.concurrent + hint_concurrent (subprocess)")
    # the callers' threads and the batcher's lanes in a process of their own: beside the parent's pipelines, sixteen contexts and torch's
    # streams the same legs measured 20 % lower (K = 16: 37 M against 46 M headers/s; the 32 hints 0.44 against 0.33 ms)
    d, err = subprocess_leg(args, ["--only-leg", "coalescing"])
    out["coalescing"] = {"error": err} if d is None else d
    if not args.no_witness:
        # A/B on THIS box: the headline step with and without the COMMIT / SKIP units (two more expansion launches per chunk, the field
        # proofs and the unit stores of the commit chain on the side stream) — VERDICT r4 weak #8 asked what they cost the big expansion
        log("leg: units_ab (2 subprocesses)")
        ab = {}
        for key, extra in (("with_units", []), ("without_units", ["--no-units"])):
            d, err = subprocess_leg(args, ["--long-steps", "0"] + extra)
            ab[key] = {"error": err} if d is None else {
                "value": d["value"], "ms_per_step": d["ms_per_step"], "expand_map_avg_launch_ms": d["roofline"]["avg_launch_ms"],
                "frac_of_measured_store_ceiling": d["roofline"]["frac_of_measured_store_ceiling"],
                "stored_bytes_per_step": d["roofline_whole_step"]["stored_bytes_per_step"], "whole_step_store_GBps": d["roofline_whole_step"]["achieved"]}
        ab["note"] = ("same process shape, same box, back to back: `without_units` = BSX_PIPE_NO_UNITS (round 3's witness: map jobs + reduce nodes); the "
                      "difference in expand_map_avg_launch_ms is what the units' side-stream work costs the large launch")
        out["units_ab"] = ab
    if (J, B) == (32, 64):
        log("leg: header_range_1024 (subprocess)")
        a1024 = argparse.Namespace(**vars(args))
        a1024.batch = 32
        d, err = subprocess_leg(a1024, [])
        out["header_range_1024"] = {"error": err} if d is None else {
            "workload": d["config"]["workload"], "value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"],
            "steps": d["steps"], "roofline_frac": d["roofline"]["frac"], "witness_checked_ranges": d["config"]["witness_checked_ranges"],
            # BASELINE config #3 ("header_range_1024 ... with rocprof HBM-GB/s counters"): the leg's own roofline object, `traffic` from the
            # committed PMC passes of THIS shape (profiles/r5_1024_pmc_hbm_traffic.csv)
            "roofline": d["roofline"]}
    return out

def sharded_self_check(eng, w, J, B, V, R, rank, dev, res):
    """N > 1 must prove itself: re-prove a sample of the owned ranges with an UN-SHARDED pipeline (world = 1, all map jobs,
    no collective) on this rank's own GPU and compare public output, final status, commit result, this rank's map-job
    records and — for one range — this rank's slice of the Goldilocks witness."""
    from blobstreamx_amd import engine as E
    from blobstreamx_amd import types as T
    ks = sorted({0, R // 2, R - 1})
    solo = E.HeaderRangeEngine(J, B, V, len(ks), device=dev, with_witness=eng.with_witness)
    solo.upload_workload(w, np.array([rank * R + k for k in ks]))
    solo.step()
    sres = solo.download()
    for i, k in enumerate(ks):
        assert sres["output64"][i].tobytes() == res["output64"][k].tobytes(), f"rank {rank}: sharded output of owned range {k} differs from the un-sharded pipeline"
        assert sres["range_status"][i] == res["range_status"][k] and sres["skip_status"][i] == res["skip_status"][k]
        a, b = np.array(sres["commit"][i]).copy(), np.array(res["commit"][k]).copy()
        a["_pad"] = 0; b["_pad"] = 0
        assert a.tobytes() == b.tobytes()
        mine = res["records"][rank * R + k].copy()
        ref = sres["records"][i][eng.jf:eng.jf + eng.jc].copy()
        mine["_pad"] = 0; ref["_pad"] = 0
        assert mine.tobytes() == ref.tobytes(), f"rank {rank}: map-job records of owned range {k} differ from the un-sharded pipeline"
    checked_w = 0
    if eng.with_witness:
        nel = int(T.map_layout(B)["n_elements"])
        sw = solo.witness_map[eng.jf * nel:(eng.jf + eng.jc) * nel]          # un-sharded range ks[0], jobs of this rank's slice
        i0 = eng.rank * eng.Rc                                               # owned range 0 = chunk 0, position rank*Rc
        mw = eng.buffer(0, E.BUF_WITNESS_MAP, i64=True)[i0 * eng.jc * nel:(i0 + 1) * eng.jc * nel]
        assert torch.equal(sw, mw), f"rank {rank}: sharded map-job witness of owned range 0 differs from the un-sharded pipeline"
        checked_w = 1
    del solo
    return {"ranges": len(ks), "fields": "output64, statuses, commit result, map-job records", "witness_ranges": checked_w}


DUMP_LIMIT_BYTES = 64 << 20
DUMP_SAMPLE_PER_CHUNK = 1 << 16          # sampled Goldilocks elements per witness / tree section per chunk


def dump_outputs(eng, d):
    """--dump-outputs DIR: what the caller of the timed path receives from its last step, as DIR/<name>.npy — byte arrays as
    float32, integers as float64, every uint64 split into [low 32 bits, high 32 bits] so that each value is exact.  The results
    (bsx_pipeline_get_results) are written whole; of every witness / Poseidon tree section a fixed sample (seeded, the same from
    run to run) of DUMP_SAMPLE_PER_CHUNK elements per chunk, beside its [chunk, element] index.  The inputs are synth's seeded
    workload, so two builds run with the same arguments can be compared file by file."""
    from blobstreamx_amd import engine as E
    eng.join()
    res = eng.download()
    out = {"output64": res["output64"].astype(np.float32),
           "range_status": res["range_status"].astype(np.float64),
           "header_status": np.array([res["header_status"]], np.float64),
           "assemble_status": np.array([res["assemble_status"]], np.float64)}
    for key in ("commit", "records"):              # structured records: their bytes, padding zeroed
        if key in res:
            a = res[key].copy()
            a["_pad"] = 0
            out[key + "_bytes"] = a.view(np.uint8).reshape(a.shape[0], -1).astype(np.float32)
    if "skip_status" in res:
        out["skip_status"] = res["skip_status"].astype(np.float64)
    sections = []
    if eng.with_witness:
        sections += [("witness_map", E.BUF_WITNESS_MAP), ("witness_reduce_local", E.BUF_WITNESS_REDUCE_LOCAL),
                     ("witness_reduce_top", E.BUF_WITNESS_REDUCE_TOP), ("witness_commit_units", E.BUF_WITNESS_COMMIT),
                     ("witness_skip_units", E.BUF_WITNESS_SKIP)]
    if eng.with_caps:
        sections += [("caps_trees", E.BUF_TREES), ("caps_trees_commit_units", E.BUF_TREES_COMMIT), ("caps_trees_skip_units", E.BUF_TREES_SKIP)]
    if eng.K > 1 and sections:
        # with buffer sets the last step's set is the library's to know: no sample rather than one of another step
        log(f"--dump-outputs: {eng.K} buffer sets, witness / tree sections not sampled")
        sections = []
    torch.cuda.synchronize(eng.dev)
    for s, (name, which) in enumerate(sections):
        vals, idx = [], []
        for e in range(eng.E):
            buf = eng.buffer(e, which, i64=True)
            if buf.numel() == 0:
                continue
            rng = np.random.default_rng([0xB5A, s, e])
            pick = np.unique(rng.integers(0, buf.numel(), min(DUMP_SAMPLE_PER_CHUNK, buf.numel()), dtype=np.int64))
            v = buf[torch.from_numpy(pick).to(eng.dev)].cpu().numpy().view(np.uint64)
            vals.append(np.stack([v & 0xFFFFFFFF, v >> 32], axis=1).astype(np.float64))
            idx.append(np.stack([np.full(pick.size, e), pick], axis=1).astype(np.float64))
        if vals:
            out[name] = np.concatenate(vals)
            out[name + "_index"] = np.concatenate(idx)
    total = sum(a.nbytes for a in out.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} bytes > {DUMP_LIMIT_BYTES}"
    os.makedirs(d, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(d, name + ".npy"), a)
    log(f"--dump-outputs: {len(out)} arrays, {total / 2**20:.1f} MB -> {d}")


# ---------------------------------------------------------------------------------------------------------------- main
def main():
    args = parse()
    self_launch(args)                                   # --gpus N without a launcher: spawns the N ranks and exits with their code
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.dry_run:
        return dry_run(args, rank, world)
    # the line's n_gpus is the world that RUNS: a launcher's WORLD_SIZE wins over a stale --gpus, and N ranks need N GPUs
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s); reporting n_gpus = {world}", file=sys.stderr)
        args.gpus = world
    if os.environ.get("BSX_BENCH_DEVICE") is None:
        assert torch.cuda.device_count() >= world, f"{world} ranks on this node need {world} GPUs, {torch.cuda.device_count()} visible"
    # test hooks (tests/test_gpu_engine.py runs the N > 1 code path with two ranks on ONE GPU): device override and a
    # gloo process group; the driver's multi-GPU runs use neither (one rank per GPU over RCCL)
    if os.environ.get("BSX_BENCH_DEVICE") is not None:
        local = int(os.environ["BSX_BENCH_DEVICE"])
    pre_legs = subprocess_legs(args) if (world == 1 and args.mode == "F" and not args.no_legs) else {}
    from blobstreamx_amd import _lib
    _lib.lib()                     # loads libbsx.so (after torch: one HIP runtime) before the first HIP call
    torch.cuda.set_device(local)
    dev = torch.device(f"cuda:{local}")
    backend = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("BSX_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    import synth
    from blobstreamx_amd import engine as E
    from blobstreamx_amd import types as T

    if args.only_leg == "coalescing":
        J, B, V = args.jobs, args.batch, args.validators
        print(DETAIL_PREFIX + json.dumps({"concurrent": concurrent_leg(dev, J, B, V), "hint_concurrent": hint_concurrent_leg(dev, J, B, V)}))
        return
    cal = calibrate(dev)
    J, B, V = args.jobs, args.batch, args.validators
    if args.mode == "S":
        # mode S as the primary object: commits sharded with their headers across the ranks
        out = stress(args, dev, V, args.cpu_seconds, cal, rank=rank, world=world)
        if rank == 0:
            emit({"metric": "headers/sec, mode S (a commit on every header)", "value": out["headers_per_s"], "unit": "headers/s",
                              "n_gpus": world, "steps": 5, "warmup": 1, "ms_per_step": out["ms"], "higher_is_better": True, "scaling": "strong",
                              "vs_baseline": None, "dtype": "u32", "data": "synthetic",
                              "config": {"workload": out["workload"], "nccl_ranks": world, "dist_backend": backend,
                                         "parallelism": f"{world} x {args.jobs * args.batch // world} commits, 1 all-gather of 128-byte folds per step"},
                              "roofline": out["roofline"], "cpu_baseline": out.get("cpu_baseline"), "calibration": cal, "stress": out})
        if world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        return
    strong = args.scaling == "strong" and world > 1
    R = args.ranges // world if strong else args.ranges          # ranges OWNED per rank
    assert R >= args.engines and R % args.engines == 0, "ranges per rank must be a multiple of the pipelined chunks"
    t0 = time.perf_counter()
    w = synth.Workload(4, R * world, J, B, v=V)          # config #4 seed; identical on every rank
    t_gen = time.perf_counter() - t0
    Ech = args.engines
    kw = dict(n_engines=Ech, rank=rank, world=world, device=dev, with_witness=not args.no_witness, with_caps=args.caps, merkle_workgroups=args.merkle_wgs,
              with_commit=not args.no_commit, subchain_form=args.subchain_form, units=not args.no_units)
    eng = E.AlternatingPipelines(args.alternate, J, B, V, R, **kw) if args.alternate > 1 else E.PipelinedEngines(J, B, V, R, **kw)
    eng.upload_workload(w)
    p0 = eng
    collective = None
    if world > 1:
        # The one collective of the path.  Default: ncclAllGather called by the LIBRARY on its exchange stream, on a communicator made
        # through the C ABI (rank 0's unique id goes over the torch.distributed group: control plane only) — no Python between the
        # local fold and the top fold.  Every rank must take the same branch: the availability probe is agreed on first, and
        # bsx_pipeline_check_allgather proves the collective end to end before the first step.
        import torch.distributed as dist
        collective = "torch.distributed all_gather_into_tensor through the bsx_pipeline_set_allgather callback"
        if args.collective == "rccl-c" and backend == "nccl":
            probe = np.zeros(128, np.uint8)
            ok = torch.tensor([1 if _lib.lib().bsx_rccl_get_unique_id(_lib.p(probe)) == 0 else 0], device=dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 1:
                # every step of the set-up is agreed on by all ranks before the next (a rank that fails alone would leave the others in a
                # collective): communicator, then the library's own all-gather proven end to end; any failure anywhere -> the callback
                def agreed(flag):
                    t = torch.tensor([1 if flag else 0], device=dev)
                    dist.all_reduce(t, op=dist.ReduceOp.MIN)
                    return int(t.item()) == 1
                comm, err = None, None
                try:
                    comm = E.c_rccl_comm(eng.ctx, rank, world)
                except Exception as e:                                   # noqa: BLE001 (reported below, then the fallback)
                    err = e
                if agreed(comm is not None):
                    try:
                        eng.set_rccl(comm)
                    except Exception as e:                               # noqa: BLE001
                        err = e
                    if agreed(err is None):
                        collective = "ncclAllGather called by libbsx (bsx_pipeline_set_rccl), communicator from bsx_rccl_comm_init_rank"
                if not collective.startswith("ncclAllGather"):
                    if rank == 0:
                        print(f"bench.py: RCCL from the C tier not usable here ({err}); using the torch.distributed callback", file=sys.stderr)
                    eng.set_allgather(E.torch_allgather(eng.dev, world))

    # correctness gate before timing: statuses clean, public output = (target header hash, commitment) for every owned range
    eng.step()
    res = eng.download()
    own = slice(rank * R, (rank + 1) * R)
    assert res["header_status"] == 0 and res["assemble_status"] == 0, res
    assert not res["range_status"].any() and (args.no_commit or not res["skip_status"].any()), (res["range_status"], res.get("skip_status"))
    assert args.no_commit or (res["output64"][:, :32] == w.hashes[own, w.n_blocks]).all(), "target header hash mismatch"
    gpu_out64 = res["output64"].copy()
    self_check = sharded_self_check(p0, w, J, B, V, R, rank, dev, res) if world > 1 else None

    def barrier():
        eng.join()
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    # one-time, before the warm-up: which hardware queues the chunks' streams overlap best on (bsx_pipeline_autotune; real steps)
    tune = eng.autotune(0) if not args.no_autotune else None
    for _ in range(args.warmup):
        eng.step()
    barrier()
    eng.set_timing(True)             # HIP events on the launch streams, inside the library
    t0 = time.perf_counter()
    for i in range(args.steps):
        eng.step()
    barrier()
    elapsed = time.perf_counter() - t0
    tm = eng.timing()
    eng.set_timing(False)
    t_sub, t_exp = tm["prove_subchain_ms"], tm["expand_map_ms"]
    multi_gpu = None
    if world > 1:
        # what the first hardware scaling run needs to be diagnosable: every rank's own step time and the all-gather as the library
        # timed it on its exchange stream (HIP events), gathered to rank 0; `value` uses the MAX over ranks
        mine = torch.tensor([elapsed / args.steps * 1e3, tm["allgather_us"]["avg"], tm["allgather_us"]["min"], tm["allgather_us"]["median"],
                             tm["allgather_us"]["max"], float(tm["exchanges"])], device=dev, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        torch.distributed.all_gather(allr, mine)
        rows = [[float(x) for x in t.tolist()] for t in allr]
        multi_gpu = {"per_rank_ms_per_step": [r[0] for r in rows],
                     "allgather_us_per_chunk": {"avg": [r[1] for r in rows], "min": [r[2] for r in rows], "median": [r[3] for r in rows],
                                                "max": [r[4] for r in rows]},
                     "allgathers_timed_per_rank": [int(r[5]) for r in rows],
                     "note": "all-gather of one 128-byte record per (range, rank) per chunk, timed with HIP events on the library's exchange stream from "
                             "'this rank's folded records are ready' to 'every rank's have arrived' (includes waiting for the slowest rank); it is "
                             "issued behind the local fold and joined behind the chunk's expansion, so it is hidden unless it outlasts the expansion"}
        tmax = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(tmax.item())
        assert torch.distributed.get_world_size() == world == args.gpus, (torch.distributed.get_world_size(), world, args.gpus)
    ms_per_step = elapsed / args.steps * 1e3
    headers_per_step = world * R * J * B
    value = headers_per_step / (elapsed / args.steps)
    if args.dump_outputs and rank == 0:
        dump_outputs(eng, args.dump_outputs)     # the last timed step's results, before anything steps the pipeline again
    # a second, longer loop (20 steps are 0.12 s — SURVEY §8(d)'s 100 ms with no margin): same steps, `long_run`
    long_run = None
    if args.long_steps > 0 and world == 1:
        torch.cuda.synchronize(dev)
        t0l = time.perf_counter()
        for i in range(args.long_steps):
            eng.step()
        eng.join()
        el = time.perf_counter() - t0l
        long_run = {"steps": args.long_steps, "seconds": el, "ms_per_step": el / args.long_steps * 1e3, "value": headers_per_step / (el / args.long_steps),
                    "unit": "headers/s"}
    # the witness the TIMED loop left in HBM, against the oracle (every rank checks its own buffers)
    n_checked = cpu_baseline_witness_check(p0, w, J, B) if not args.no_witness else 0
    res2 = eng.download()
    assert (res2["output64"] == gpu_out64).all() and not res2["range_status"].any() and (args.no_commit or not res2["skip_status"].any()), "outputs changed during the timed loop"

    if rank == 0:
        ml = p0.ml
        n_jobs = p0.RT * p0.jc           # map jobs per launch (one chunk = 1/E of the step)
        # algorithmic bytes: expansion reads the compact witness once and writes 8 B per element
        exp_bytes = n_jobs * (int(ml["n_bytes"]) + 4 * int(ml["n_words"]) + int(ml["n_bools"]) + 8 * int(ml["n_elements"]))
        slots = n_jobs * B
        sub_bytes = slots * (362 + 352 + 64 + 32 + 64)      # per slot: proofs read; paths+curr, tuple, leaf hash, 2 tree nodes written
        # every Goldilocks element the step stores (8 B each), by section: map jobs, reduce nodes (local + top levels), and — with the
        # commit check on — the COMMIT + SKIP unit of every owned range (the units were missing from this figure)
        rl_, cl_, sl_ = T.reduce_layout(), T.commit_layout(V), T.skip_layout(V)
        units_on = bool(getattr(p0, "units", False))
        step_sections = {"map_jobs": Ech * n_jobs * 8 * int(ml["n_elements"]),
                         "reduce_nodes": Ech * (p0.RT * max(p0.jc - 1, 0) + p0.Rc * (world - 1)) * 8 * int(rl_["n_elements"]),
                         "commit_units": (R * 8 * int(cl_["n_elements"])) if units_on else 0,
                         "skip_units": (R * 8 * int(sl_["n_elements"])) if units_on else 0}
        step_store_bytes = sum(step_sections.values())
        out = {
            "metric": f"headers/sec witness-gen, header_range_{J * B} (SHA HBM GB/s vs roofline in `roofline`/`kernels`)",
            "value": value, "unit": "headers/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "long_run": long_run,
            "dtype": "u32", "data": "synthetic",
            "config": {"workload": f"header_range_{J * B} ({J} map jobs x {B} headers), {V} validators, mode F (one target commit per range), "
                                   f"{R} ranges per GPU per step, Goldilocks witness {'off' if args.no_witness else 'materialised'}"
                                   + (", Poseidon caps from the compact bytes" if args.caps else ""),
                       "timed_entry": "bsx_pipeline_step (C ABI, csrc/pipeline.hip)",
                       "ranges_per_gpu": R, "headers_per_step": headers_per_step, "pipelined_chunks": Ech, "buffer_sets": args.alternate,
                       "parallelism": (f"{world} x ({J // world} of {J} map jobs = {J * B // world} headers of every range), 1 all-gather of 128-B "
                                       f"records per chunk; {'strong: ' + str(R * world) + ' ranges in total' if strong else 'weak: ' + str(R) + ' ranges per GPU'}")
                       if world > 1 else "1 GPU",
                       "nccl_ranks": torch.distributed.get_world_size() if world > 1 else 1, "dist_backend": backend, "collective": collective,
                       "multi_gpu": multi_gpu,
                       "sharded_vs_unsharded_self_check_per_rank": self_check,
                       "witness_checked_ranges": n_checked,
                       "witness_bytes_per_step_per_gpu": int(step_store_bytes) if not args.no_witness else 0,
                       "witness_bytes_per_step_per_gpu_by_section": step_sections if not args.no_witness else None,
                       "input_generation_s": round(t_gen, 2), "stream_autotune": tune,
                       "ed25519_path": p0.ed_path, "commit_beside": p0.commit_with, "memory_partition": memory_partition_mode()},
            "calibration": cal,
        }
        if not args.no_witness:
            # the same kernel alone on an idle GPU (after the timed region): what the overlap with the other chunk's hashing costs it
            iso = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            compact, wmap = p0.buffer(0, E.BUF_COMPACT), p0.buffer(0, E.BUF_WITNESS_MAP, i64=True)
            t_iso = 0.0
            for _ in range(5):
                iso[0].record()
                _lib.check(p0.L.bsx_dev_expand_witness(p0.ctx, st, _lib.p(p0._ml), C.c_uint32(n_jobs), _lib.dp(compact), _lib.dp(wmap)))
                iso[1].record()
                torch.cuda.synchronize(dev)
                t_iso += iso[0].elapsed_time(iso[1]) / 5
            traffic, traffic_src = pmc_traffic(n_jobs, {"batch": B})
            # SURVEY §8(d)'s LITERAL per-slot figure (362 B read + (362 + 384) x 64 B written = 48,106 B per header slot) beside the
            # layout's own count (every variable bsx_witness_manifest lists: 57,124 B per slot at B = 64) — VERDICT r3 weak #8
            survey_bytes = slots * 48106
            out["roofline"] = {"kernel": "k_expand_witness (map-job section)", "bound": "hbm", "achieved": exp_bytes / t_exp / 1e6,
                               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": exp_bytes / t_exp / 1e6 / HBM_PEAK_GBS,
                               "byte_accounting": {"layout_bytes_per_slot": exp_bytes / slots, "frac_layout_bytes": exp_bytes / t_exp / 1e6 / HBM_PEAK_GBS,
                                                   "survey_8d_bytes_per_slot": 48106, "achieved_survey_8d": survey_bytes / t_exp / 1e6,
                                                   "frac_survey_8d": survey_bytes / t_exp / 1e6 / HBM_PEAK_GBS,
                                                   "note": "`frac` prices the bytes the kernel really moves (the layout's variables, = PMC traffic 1.00x); "
                                                           "SURVEY §8(d)'s literal figure counts 12 digests per slot where the layout holds the 10 path digests, "
                                                           "curr_header, the tuple, leaf hash, two tree nodes, words and bools"},
                               "traffic": traffic, "traffic_source": traffic_src,
                               "avg_launch_ms": t_exp, "algorithmic_bytes_per_launch": exp_bytes, "launches_timed": tm["launches"],
                               "measured_store_ceiling_GBps": cal["hbm_store_bytes_per_s"] / 1e9,
                               "frac_of_measured_store_ceiling": min(1.0, exp_bytes / t_exp * 1e3 / cal["hbm_store_bytes_per_s"]),
                               "isolated": {"avg_launch_ms": t_iso, "achieved": exp_bytes / t_iso / 1e6, "frac": exp_bytes / t_iso / 1e6 / HBM_PEAK_GBS},
                               "note": "expanded (witness-emitting) byte count: 8 B written per Goldilocks element + the compact read; "
                                       "`achieved` is measured with HIP events on the launch stream inside the timed region where the kernel "
                                       "co-runs with the other chunk's ALU-bound hashing; `isolated` is the same launch alone; `traffic` = PMC "
                                       "bytes per launch read from the committed profile at run time (null when no profile of this shape exists)"}
            # the same bound priced over the WHOLE step: every byte stored (map jobs + reduce nodes + COMMIT / SKIP units) over the step's
            # wall time — what `headers/s` does not credit (the units are 1.2 GB of the 30.7 GB per step)
            out["roofline_whole_step"] = {"kernel": "every k_expand_witness launch of a step (map jobs, reduce nodes, COMMIT + SKIP units)", "bound": "hbm",
                                          "achieved": step_store_bytes / ms_per_step / 1e6, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                          "frac": step_store_bytes / ms_per_step / 1e6 / HBM_PEAK_GBS, "stored_bytes_per_step": int(step_store_bytes),
                                          "sections": step_sections, "ms_per_step": ms_per_step,
                                          "frac_of_measured_store_ceiling": min(1.0, step_store_bytes / ms_per_step * 1e3 / cal["hbm_store_bytes_per_s"]),
                                          "traffic": None, "note": "stores only (the compact reads are 1.6 % of the traffic); wall time of the step, so the "
                                                                   "hashing / commit phases that run beside the expansions are inside it"}
        else:
            out["roofline"] = None
        fused = bool(p0.fused_hint)
        exec_per_slot = (2 + 2 * (B - 1) / B) if fused else (21 + 2 * (B - 1) / B)     # tuple leaf + tree (+ both proof paths)
        comp_s = slots * exec_per_slot / t_sub * 1e3
        one_launch = fused and not (p0.with_witness and p0.E > 1)
        out["kernels"] = [{"kernel": "prove_subchain (k_batch_finish<fused>: tuple leaf hashes + every tree level + predicates in one launch)" if one_launch
                           else "prove_subchain (k_slot_hashes + k_tree_level x n + k_batch_finish)", "avg_launch_ms": t_sub, "slots_per_launch": slots,
                           "compact_bytes_per_slot": 874, "achieved_GBps": sub_bytes / t_sub / 1e6,
                           "frac_of_hbm_peak": sub_bytes / t_sub / 1e6 / HBM_PEAK_GBS,
                           "fused_hint": fused, "sha256_compressions_executed_per_slot": exec_per_slot,
                           "sha256_compressions_per_s": comp_s, "frac_of_measured_alu_peak": min(1.0, comp_s / cal["sha256_compress_per_s"]),
                           "reference_equivalent_compressions_per_s": slots * 23 / t_sub * 1e3,
                           "note": "compact bytes (362 B proofs in + 512 B digests/tuple out per slot); integer-ALU bound; peak = the SHA-256 compression "
                                   "rate measured in this run.  With the fused hint the 19 path compressions per slot the reference's circuit performs "
                                   "(builder.rs:189-199) are NOT executed: their digests are nodes of the header trees k_header_merkle hashed (41 "
                                   "compressions/header) and are copied, so `reference_equivalent` counts the reference's 23/slot over the same time; "
                                   "in-region = beside the other chunk's expansion"}]
        if args.no_witness:
            per_header = 41 + exec_per_slot
            out["compact_step"] = {"sha256_compressions_executed_per_header": per_header, "sha256_compressions_per_s_whole_step": value * per_header,
                                   "frac_of_measured_alu_peak_whole_step": min(1.0, value * per_header / cal["sha256_compress_per_s"]),
                                   "measured_sha256_ceiling_per_s": cal["sha256_compress_per_s"]}
        # rank 0 keeps the CPU baseline at every N (north_star: GPU throughput next to the CPU path, core count stated);
        # the other legs are N = 1 only
        log("headline timed; cpu_baseline")
        if not args.no_legs and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(w, J, B, V, args.cpu_seconds, gpu_out64, min(R, 256), first=rank * R)
        legs = world == 1 and not args.no_legs
        if legs and not args.no_witness:
            log("leg: with_input_upload")
            out["with_input_upload"] = upload_leg(p0, args, max(5, args.steps // 2))
        del eng, p0
        torch.cuda.empty_cache()
        if legs:
            log("leg: latency")
            out["latency"] = latency_leg(dev, J, B, V)
            co = pre_legs.pop("coalescing", None) or {}
            out["latency"]["concurrent"] = co.get("concurrent", co)
            out["hint_concurrent"] = co.get("hint_concurrent", co)
            log("leg: keyset_churn")
            out["keyset_churn"] = keyset_churn_leg(dev, J, B, V)
            log("leg: range_sweep")
            out["range_sweep"] = {"compact": range_sweep_leg(dev, J, B, V), "witness": range_sweep_leg(dev, J, B, V, rs=(1, 4, 16, 64), witness=True)}
            log("leg: fused_commitment")
            out["fused_commitment"] = commitment_leg(dev, J, B, V, cal)
            if not args.no_stress:
                log("leg: stress v100")
                sv100 = stress(args, dev, 100, 6.0, cal)
                log("leg: stress v512")
                out["stress"] = {"v100": sv100, "v512": stress(args, dev, 512, 6.0, cal)}
            out.update(pre_legs)
        emit(out)                      # DETAIL {...full...} then the compact line (bench_legs/line.py) — the LAST stdout line, < 6 KB
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
