#!/usr/bin/env python3
"""bench.py - Mvoxels/s of SDF extraction (BASELINE.json metric).

A "step" is one pass of the hot path (r2s_plan_run_dev: mesh prep -> work items -> tile bins
-> sentinel sweep -> projection/sign kernel, then the Z-slab all-gather when N > 1) over the
north-star workload of BASELINE.md section 4 ("NS"): synthetic jittered HEX8 46^3 = 97 336
elements, 512^3 grid (N_max = 505), rho_t = 0.5.  Inputs are resident in HBM before the
timed region; the output SDF stays in HBM.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--grid 512] [--mesh 46] [--full] [--dump-outputs DIR]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the result line (`value`, `ms_per_step`, and the
stage times, work counts and roofline figures derived from the timed steps themselves).  --full adds what takes work
of its own: the host-pointer end-to-end leg (N = 1), the CPU oracle baseline and the `max|err| vs ref` check below.
--dump-outputs DIR writes the volume of the last timed step as float64 samples: DIR/sdf_planes.npy (every
`stride`-th Z plane in full, at most 32 MB) and DIR/sdf_sample.npy (voxels at sorted indices drawn with
numpy.random.default_rng(DUMP_SEED) over the flat x-fastest volume, 2^21 of them).

With N > 1 the fixed 512^3 grid is partitioned along Z (one rank per GPU; default: interleaved
4-plane tile layers, balanced) and stitched over RCCL/xGMI so that every rank holds the whole volume
("scaling": "strong"): by default only the 4x4x4 tiles that can differ from the sentinel travel
(one padded all_gather_into_tensor of counts + tile payloads + ids per step; --stitch dense
gathers the full Float64 volume instead).

With --full, at N = 1 rank 0 also times the CPU oracle ("cpu_baseline", kind "port") on a plane sample of the same workload:
up to 16 single-thread worker processes, worker w on the Z planes k % --cpu-stride == w (about 25 s of CPU work);
--check compares worker 0's planes with the GPU result bit for bit.
"""
import argparse
import json
import os
import sys
import time

# The CPU share of a GPU box is a cgroup quota (16 CPUs) on a host with 256 visible ones: libgomp / OpenBLAS under torch and
# numpy start one thread per VISIBLE CPU, and their idle spinning after any parallel region uses the quota up - the whole
# process is then throttled for tens of ms, which the host threads of the e2e legs (16 of them: fill, scatter, staged
# copies) pay for (tools/throttle_check.sh: nr_throttled in cpu.stat, e2e 13-16 ms -> 9 ms with this setting).  Nothing in
# this script needs OpenMP.
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "4")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
ALG_BYTES_PER_VOXEL = 8.0      # one Float64 store per voxel; + mesh bytes / ngp
FP64_VALU_PEAK_TFLOPS = 78.6   # MI355X FP64 vector peak (256 CUs x 4 SIMDs x 16 lanes x 2 FLOP x 2.4 GHz)
DOMINANT_KERNEL = {"HEX8": "iso_project_hex_pl_kernel", "TET4": "iso_project_kernel"}
PROFILE_ROUND = "r04"          # profiles/<round>_traffic.json, <round>_valu_counters.json (tools/collect_traffic.py)
DUMP_SEED = 20241015           # --dump-outputs: the voxel sample is the same for every build and run of a workload
DUMP_SAMPLE = 1 << 21          # sampled voxels (16 MB of float64)
DUMP_PLANES_BYTES = 32 << 20   # full Z planes, at most this many bytes


def dump_outputs(vol, out_dir):
    """write the stitched (nz, ny, nx) float64 volume of the last timed step as two fixed samples (whole volume > 64 MB):
    every stride-th Z plane (contiguous surface band; k % stride == 0 are all first planes of a 4-plane tile layer) and
    seeded scattered voxels (every plane and tile position).  Returns {name: shape}."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    nz, ny, nx = vol.shape
    row_bytes = nx * vol.element_size()
    n_planes = max(1, min(nz, DUMP_PLANES_BYTES // (ny * row_bytes)))
    stride = -(-nz // n_planes)                               # ceil: at most n_planes planes
    rows = min(ny, max(1, DUMP_PLANES_BYTES // row_bytes))    # (a single plane over the budget: its first rows)
    planes = vol[::stride, :rows].cpu().numpy()
    rng = np.random.default_rng(DUMP_SEED)
    idx = np.sort(rng.integers(0, vol.numel(), size=min(DUMP_SAMPLE, vol.numel()), dtype=np.int64))
    sample = vol.reshape(-1)[torch.from_numpy(idx).to(vol.device)].cpu().numpy()
    res = {}
    for name, a in (("sdf_planes", planes), ("sdf_sample", sample)):
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
        res[name] = list(a.shape)
    res["plane_stride"] = stride
    return res


def load_committed_profile(kernel):
    """PMC figures of the dominant kernel from the committed rocprofv3 passes of this same command (separate --pmc runs,
    tools/collect_traffic.py): they are NOT measured in the timed run and are labelled so.  None when absent."""
    for rnd in (PROFILE_ROUND, "r03", "r02"):
        tfile = os.path.join(ROOT, "profiles", f"{rnd}_traffic.json")
        vfile = os.path.join(ROOT, "profiles", f"{rnd}_valu_counters.json")
        if not (os.path.exists(tfile) and os.path.exists(vfile)):
            continue
        def pick(d):   # templated kernels appear as name<args>: the instantiation with the most launches
            c = [(k, x) for k, x in d.items() if k == kernel or k.startswith(kernel + "<")]
            return max(c, key=lambda kx: kx[1].get("launches", 0))[1] if c else None
        t = pick(json.load(open(tfile))["kernels"])
        v = pick(json.load(open(vfile)))
        if not t or not v:
            continue
        traffic = None
        if t.get("FETCH_SIZE_KB") is not None and t.get("WRITE_SIZE_KB") is not None:
            traffic = (t["FETCH_SIZE_KB"] + t["WRITE_SIZE_KB"]) * 1024.0
        fp = {"source": f"committed profile profiles/{rnd}_valu_counters.json (not measured in this run)",
              "valu_insts_per_launch": v.get("SQ_INSTS_VALU"),
              "lane_utilisation": (v["SQ_THREAD_CYCLES_VALU"] / (64.0 * v["SQ_ACTIVE_INST_VALU"])
                                   if v.get("SQ_ACTIVE_INST_VALU") else None)}
        # FP64 FLOP per launch from the per-type instruction counters (wave64 instructions x 64 lanes x lane
        # utilisation; FMA = 2 FLOP) when they were collected
        if all(v.get(k) is not None for k in ("SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_MUL_F64", "SQ_INSTS_VALU_ADD_F64")):
            lu = fp["lane_utilisation"] or 1.0
            fp["fp64_insts_per_launch"] = {k[14:]: v[k] for k in ("SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_MUL_F64",
                                                                   "SQ_INSTS_VALU_ADD_F64", "SQ_INSTS_VALU_TRANS_F64")
                                           if v.get(k) is not None}
            fp["flop_per_launch"] = 64.0 * lu * (2.0 * v["SQ_INSTS_VALU_FMA_F64"] + v["SQ_INSTS_VALU_MUL_F64"]
                                                 + v["SQ_INSTS_VALU_ADD_F64"])
        # the whole step: sum of (FETCH + WRITE) over every kernel of one call (same file)
        step_traffic = None
        try:
            ks = json.load(open(tfile))["kernels"]
            step_traffic = sum((k.get("FETCH_SIZE_KB") or 0.0) * k.get("launches_per_step", 1) +
                               (k.get("WRITE_SIZE_KB") or 0.0) * k.get("launches_per_step", 1) for k in ks.values()) * 1024.0
        except Exception:
            pass
        return {"traffic": traffic, "step_traffic": step_traffic,
                "traffic_source": f"committed profile profiles/{rnd}_traffic.json (separate --pmc passes, "
                                  "not measured in this run)", "fp64": fp}
    return None


def e2e_leg(pkg, X, IEN, rho_n, rho_t, grid, dev_index, sg):
    """SURVEY 8(d)'s end-to-end figure through the drop-in entry point the Julia binding ccalls (r2s_sdf on host
    pointers: H2D of the mesh + all kernels + D2H of the Float64 volume), once into ordinary pageable memory and once
    into a buffer from r2s_host_alloc (pinned; what the Julia wrapper allocates its result arrays from)."""
    import ctypes
    mesh = pkg.Mesh(X, IEN)
    res = {}
    names = ("upload", "run", "pack_and_issue", "wait_fill", "wait_copies", "scatter", "call", "threads")
    for kind in ("pageable", "pinned"):
        out = pkg.host_array(grid.ngp) if kind == "pinned" else np.empty(grid.ngp)
        times, phases = [], []
        for _ in range(9):   # (the first call allocates; the host side of the sparse download varies from call to call on a shared box)
            t0 = time.perf_counter()
            pkg.sdf_fused(mesh, grid, rho_n, rho_t, device=dev_index, out=out)
            times.append(time.perf_counter() - t0)
            ph = (ctypes.c_double * 8)()
            pkg._lib.lib().r2s_last_host_phases(ph)
            phases.append({k: round(float(v), 2) for k, v in zip(names, ph)})
        order = sorted(range(1, 9), key=lambda q: times[q])
        best, med = order[0], order[len(order) // 2]
        res[kind] = {"ms_per_call": times[best] * 1e3, "Mvoxels_per_s": grid.ngp / times[best] / 1e6,
                     "ms_per_call_median": times[med] * 1e3, "Mvoxels_per_s_median": grid.ngp / times[med] / 1e6,
                     "first_call_ms": times[0] * 1e3, "calls": 8,
                     "host_phases_ms_best": phases[best], "host_phases_ms_median": phases[med]}
        same = np.array_equal(out.reshape(sg.nz, sg.ny, sg.nx)[::32], sg.volume()[::32].cpu().numpy())
        res[kind]["equals_device_path"] = bool(same)
        del out
    res["default_leg"] = "pageable"   # what a Julia caller gets: ordinary arrays (Rho2sdfHIP.jl: PINNED[] = false)
    res["note"] = ("r2s_sdf(host pointers): H2D mesh + kernels + the field in the caller's array (sparse download: sentinel written by "
                   "host threads, non-sentinel tiles over PCIe; R2S_HOST_SPARSE=0: dense 8 B/voxel transfer); never `value`")
    # the whole rho2sdf() with the reference's default options (rbf_interp = true, rbf_grid = :same, artifact removal) in
    # ONE call (r2s_rho2sdf): element densities = mean of the nodal field, threshold 0.5, same grid
    rho_e = np.ascontiguousarray(rho_n[IEN - 1].mean(axis=1))
    opts = pkg.Rho2sdfOptions(threshold_density=float(rho_t))
    info = {}
    pkg.rho2sdf("bench", X, IEN, rho_e, options=opts, sdf_grid=grid, device=dev_index, pinned_results=False)     # warm-up
    t0 = time.perf_counter()
    result = pkg.rho2sdf("bench", X, IEN, rho_e, options=opts, sdf_grid=grid, device=dev_index, info=info, pinned_results=False)
    wall = time.perf_counter() - t0   # (the results stay alive: unmapping 1.6 GB of them afterwards costs the OS another 60-90 ms)
    del result
    res["rho2sdf_default_options"] = {"ms_wall": wall * 1e3, "Mvoxels_per_s": grid.ngp / wall / 1e6, "cg_iters": info["cg_iters"],
                                      "n_flipped": info["n_flipped"],
                                      "stages_ms": {k[3:]: round(v, 2) for k, v in info.items() if k.startswith("ms_")}}
    pkg._lib.lib().r2s_release_cache()
    return res




def make_workload(args):
    """the named workload -> (X, IEN (1-based), rho_n, rho_t, n_max, label).  All deterministic; chapadlo256 reads the
    committed fixture tests/golden/chapadlo.npz (nodal densities by the product's own DenseInNodes would need the GPU,
    so the fixture's element densities are projected with the library in main() and with the oracle in the CPU workers -
    both are compared bit for bit by tests/test_stages_gpu.py)."""
    from rho2sdf_jl_amd import synthetic
    if args.workload == "ns":
        X, IEN, rho_n = synthetic.hex_mesh(args.mesh or 46)
        n_max = synthetic.grid_n_max_for_points(args.grid or 512)
        return X, IEN, rho_n, 0.5, n_max, f"NS: synthetic jittered HEX8 {args.mesh or 46}^3"
    if args.workload == "tet5":
        X, IEN, rho_n = synthetic.tet_mesh(args.mesh or 55)
        n_max = synthetic.grid_n_max_for_points(args.grid or 1024)
        return X, IEN, rho_n, 0.5, n_max, f"config 5: synthetic jittered Schlafli TET4 6x{args.mesh or 55}^3"
    if args.workload == "chapadlo256":
        d = np.load(os.path.join(ROOT, "tests", "golden", "chapadlo.npz"))
        X, IEN, rho = d["X"], d["IEN"].astype(np.int64), d["rho"]
        return X, IEN, rho, 0.5, 249, "config 4: chapadlo.mat HEX8 (element densities -> DenseInNodes)"
    raise SystemExit(f"unknown workload {args.workload}")


def _oracle_planes(X, IEN, rho_n, rho_t, n_max, stride, phase):
    """the oracle on the Z planes k % stride == phase of the grid (one thread); returns (seconds, sdf of those planes)"""
    O = graft.load_oracle()
    og = O.grid_make(X.min(0), X.max(0), n_max, 3)
    O.set_k_sampling(stride, phase)
    t0 = time.perf_counter()
    dist, _, st = O.eval_distances(X, IEN, rho_n, rho_t, og, 1.1, want_xp=False)
    sign = O.sign_detection(X, IEN, rho_n, rho_t, og)
    nx, ny, nz = og.dims
    sdf = dist.reshape(nz, ny, nx)[phase::stride] * sign.reshape(nz, ny, nx)[phase::stride]   # RhoToSDF.jl:171
    dt = time.perf_counter() - t0
    O.set_k_sampling(1, 0)
    return dt, sdf, og.dims


def cpu_worker(args):
    """child process of cpu_baseline (never touches torch or the GPU): one phase of the plane sample"""
    graft.load_package()
    X, IEN, rho_n, rho_t, n_max, _ = make_workload(args)
    if args.workload == "chapadlo256":
        rho_n = graft.load_oracle().dense_in_nodes(X, IEN, rho_n)
    dt, sdf, dims = _oracle_planes(X, IEN, rho_n, rho_t, n_max, args.cpu_stride, args.cpu_worker)
    nx, ny, nz = dims
    if args.cpu_save:
        np.save(args.cpu_save, sdf)
    print(json.dumps({"seconds": dt, "planes": len(range(args.cpu_worker, nz, args.cpu_stride)), "dims": [nx, ny, nz]}))


def cpu_baseline(args, threads):
    """The oracle (CPU restatement, kind "port") on a bounded sample of the SAME workload, on `threads` host
    cores: worker w (its own process, one thread) computes the Z planes k % stride == w of the same grid over
    the same mesh - the reference's threading is also a static split of independent work with a merge at the
    end (sdfOnDensityField.jl:183-184, 457-461).  Throughput = sampled voxels / slowest worker's oracle time.
    Returns (record, sdf planes of worker 0 = planes [::stride])."""
    import subprocess
    import tempfile
    threads = max(1, min(threads, args.cpu_stride))
    with tempfile.TemporaryDirectory() as tmp:
        save = os.path.join(tmp, "planes0.npy")
        base = [sys.executable, os.path.abspath(__file__), "--workload", args.workload, "--grid", str(args.grid),
                "--mesh", str(args.mesh), "--cpu-stride", str(args.cpu_stride)]
        procs = [subprocess.Popen(base + ["--cpu-worker", str(w)] + (["--cpu-save", save] if w == 0 else []),
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for w in range(threads)]
        outs = []
        for p in procs:
            o, e = p.communicate()
            if p.returncode != 0:
                raise RuntimeError("cpu baseline worker failed: " + e[-400:])
            outs.append(json.loads(o.strip().splitlines()[-1]))
        ref = np.load(save)
    nx, ny, nz = outs[0]["dims"]
    planes = sum(o["planes"] for o in outs)
    nvox = planes * nx * ny
    dt = max(o["seconds"] for o in outs)
    cpu_s = sum(o["seconds"] for o in outs)
    return {"value": nvox / dt / 1e6, "unit": "Mvoxels/s", "cores": threads, "kind": "port",
            "sample": f"{planes} of {nz} Z planes ({nvox} voxels; plane k belongs to worker k % {args.cpu_stride}, "
                      f"workers 0..{threads - 1}) of the same {nx}x{ny}x{nz} grid over the same mesh; {threads} "
                      f"single-thread processes, slowest {dt:.1f} s, {cpu_s:.0f} s of CPU work in all",
            "seconds": dt}, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["ns", "tet5", "chapadlo256"], default="ns",
                    help="ns: north star (BASELINE metric); tet5: config 5 (998 250 TET4, 1024^3); chapadlo256: config 4")
    ap.add_argument("--grid", type=int, default=0, help="grid points per axis (default 512 for ns, 1024 for tet5)")
    ap.add_argument("--mesh", type=int, default=0, help="hex cells per axis (default 46 for ns, 55 for tet5)")
    ap.add_argument("--cpu-stride", type=int, default=0, help="CPU baseline: worker w takes the Z planes k %% stride == w "
                                                              "(default 32; 64 for tet5; 16 for chapadlo256)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="CPU baseline processes (0: host cores available, at most 16)")
    ap.add_argument("--cpu-worker", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-save", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--full", action="store_true",
                    help="also run the host-pointer end-to-end leg, the CPU oracle baseline and the check against it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write samples of the last timed step's volume to DIR/*.npy (float64, < 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU oracle leg (and with it the check)")
    ap.add_argument("--check", action="store_true", help="(kept for compatibility: with --full the check runs whenever the oracle planes exist)")
    ap.add_argument("--no-e2e", action="store_true", help="--full: skip the host-pointer end-to-end leg (r2s_sdf: H2D + kernels + D2H)")
    ap.add_argument("--no-build", action="store_true",
                    help="load the built library as it is and exit non-zero when it is missing or stale (runs under "
                         "rocprofv3 must not spawn make / hipcc: the profiler's preloaded library has initialised the GPU)")
    ap.add_argument("--partition", choices=["interleaved", "contiguous"], default="interleaved",
                    help="Z partition across GPUs (N > 1): interleaved 4-plane tile layers (balanced) or slabs")
    ap.add_argument("--stitch", choices=["sparse", "dense"], default="sparse",
                    help="N > 1: all-gather only the non-sentinel 4x4x4 tiles (sparse, interleaved partition) "
                         "or the whole Float64 volume (dense)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.cpu_stride:
        args.cpu_stride = {"ns": 32, "tet5": 64, "chapadlo256": 16}[args.workload]
    if args.cpu_worker is not None:
        return cpu_worker(args)

    # before anything initialises the HIP runtime (the host driver only supports dmabuf IPC)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    pkg = graft.load_built() if args.no_build else graft.build()

    # R2S_BENCH_REHEARSAL=1: functional rehearsal of the N > 1 path on ONE GPU (all ranks on cuda:0, gloo);
    # never used for reported numbers
    rehearsal = os.environ.get("R2S_BENCH_REHEARSAL", "0") == "1"
    dev_index = 0 if rehearsal else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    # ---- workload (deterministic) ----
    X, IEN, rho_n, rho_t, n_max, label = make_workload(args)
    if args.workload == "chapadlo256":
        rho_n = pkg.DenseInNodes(pkg.Mesh(X, IEN), rho_n, device=dev_index)   # element densities -> nodal (GPU)
    elem = "HEX8" if IEN.shape[1] == 8 else "TET4"
    grid = pkg.Grid(X.min(0), X.max(0), n_max, 3)
    nx, ny, nz = grid.dims
    ngp = grid.ngp
    dX, dI, dR = (torch.from_numpy(a).to(dev) for a in (X, IEN, rho_n))
    from rho2sdf_jl_amd import slabs
    plan = pkg.DevicePlan(dev_index)

    class TileOps:   # HIP kernels behind the sparse stitching (r2s_plan_pack_tiles_dev & co.)
        pack2 = staticmethod(lambda local, payload, ids, masks, mids: plan.pack_tiles2(local, payload, ids, masks, mids))
        unpack = staticmethod(lambda payload, ids, n, vol: plan.unpack_tiles(payload, ids, n, grid, vol))
        unpack_masks = staticmethod(lambda masks, mids, n, vol: plan.unpack_masks(masks, mids, n, grid, vol))
        unpack_all = staticmethod(lambda buf, world_, seglen, mf, mm, vol: plan.unpack_segments(buf, world_, seglen, mf, mm, grid, vol))
        fill = staticmethod(lambda t, v: plan.fill(t, v))

    sg = slabs.SlabGather((nx, ny, nz), rank, world, dev,
                          interleaved=(args.partition == "interleaved"),
                          sparse=(args.stitch == "sparse"), ops=TileOps)
    plane = sg.plane
    stats_acc = []

    def compute_slab(a, b, out, zstride, zphase):
        return plan.run(dX, dI, dR, rho_t, grid, k_begin=a, k_end=b, sdf=out, zstride=zstride, zphase=zphase)

    def step():
        st = slabs.run_step(sg, compute_slab)
        sg.volume()          # interleaved partition: put the gathered tile layers back in lattice order
        return st

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    t_first = time.perf_counter()
    step()                      # the first call of the plan API: allocations, first touches, sizes read back (no speculation)
    sync()
    first_call_ms = (time.perf_counter() - t_first) * 1e3
    for _ in range(max(args.warmup - 1, 0)):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        stats_acc.append(step())
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = elapsed / args.steps * 1e3
    value = ngp / (elapsed / args.steps) / 1e6
    dumped = dump_outputs(sg.volume(), args.dump_outputs) if args.dump_outputs and rank == 0 else None

    if rank == 0:
        sts = [s for s in stats_acc if s]
        avg = {k: float(np.mean([s[k] for s in sts])) for k in ("ms_prep", "ms_bins", "ms_fill", "ms_main", "ms_iso_fast", "ms_gather", "ms_sign")}
        st0 = sts[-1]
        nvox_rank = sg.my_planes * plane
        mesh_bytes = X.nbytes + IEN.nbytes + rho_n.nbytes
        alg_bytes = ALG_BYTES_PER_VOXEL * nvox_rank + mesh_bytes
        dominant = DOMINANT_KERNEL[elem]
        # HEX8: the dominant kernel alone (its own pair of events); ms_main also spans the straggler and sweep kernels
        kernel_ms = avg["ms_iso_fast"] if avg["ms_iso_fast"] > 0 else avg["ms_main"]
        main_s = kernel_ms * 1e-3
        achieved = alg_bytes / main_s / 1e9 if main_s > 0 else 0.0
        default_ns = args.workload == "ns" and not args.grid and not args.mesh and world == 1
        prof = load_committed_profile(dominant) if default_ns else None
        roof = {"bound": "hbm", "kernel": dominant,
                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS, "traffic": prof["traffic"] if prof else None,
                "alg_bytes_per_launch": alg_bytes, "avg_launch_ms": kernel_ms,
                # the same bytes over the whole projection (fast kernel + complete solver on the stragglers + overflow sweep)
                "achieved_over_ms_main": alg_bytes / (avg["ms_main"] * 1e-3) / 1e9 if avg["ms_main"] > 0 else None,
                "frac_over_ms_main": alg_bytes / (avg["ms_main"] * 1e-3) / 1e9 / HBM_PEAK_GBS if avg["ms_main"] > 0 else None,
                "avg_launch_ms_source": "HIP events around the kernel on its launch stream, this run",
                "real_limiter": "fp64-valu",
                "note": "the dominant kernel is FP64-VALU bound (SURVEY.md 0.7), not HBM bound: achieved/peak/frac are the "
                        "contract's algorithmic-bytes figures (8 B/voxel of the slab + mesh bytes over the kernel's measured "
                        "duration); the kernel's own roofline is `fp64` below; the HBM-bound kernel of the path is `fill_kernel`"}
        if prof:
            roof["traffic_source"] = prof["traffic_source"]
            if prof.get("step_traffic"):
                roof["step_traffic"] = prof["step_traffic"]
                roof["note"] += (f"; counter traffic of the WHOLE step (all kernels, committed profile): {prof['step_traffic'] / 1e9:.2f} GB = "
                                 f"{prof['step_traffic'] / alg_bytes:.1f} x the algorithmic bytes = "
                                 f"{prof['step_traffic'] / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS * 100:.0f} % of the HBM peak over the step")
            fp = dict(prof["fp64"])
            if fp.get("flop_per_launch") and main_s > 0:
                fp["achieved"] = fp["flop_per_launch"] / main_s / 1e12
                fp["peak"] = FP64_VALU_PEAK_TFLOPS
                fp["unit"] = "TFLOP/s"
                fp["frac"] = fp["achieved"] / FP64_VALU_PEAK_TFLOPS
            roof["fp64"] = fp
        out = {
            "metric": "Mvoxels/s SDF extract on 512^3 grid over 100k HEX8; max|err| vs ref",
            "value": value, "unit": "Mvoxels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "first_call_ms": first_call_ms,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic" if args.workload != "chapadlo256" else "reference fixture chapadlo.mat",
            "config": {"workload": f"{label} = {len(IEN)} {elem} elements, {nx}x{ny}x{nz} grid (N_max={n_max}), "
                                   f"rho_t={rho_t}, band factor 1.1, fused dist*sign, Z partition over {world} GPU(s)",
                       "name": args.workload, "elements": int(len(IEN)), "voxels": int(ngp),
                       "parallelism": (f"z-{args.partition}-{'sparse' if sg.sparse else 'dense'}-allgather-{world}"
                                       if world > 1 else "single-gpu")},
            "roofline": roof,
            "stages_ms": avg,
            "fill_kernel": {"GBps": (8.0 * nvox_rank) / (avg["ms_fill"] * 1e-3) / 1e9 if avg["ms_fill"] > 0 else None,
                            "frac_of_hbm_peak": (8.0 * nvox_rank) / (avg["ms_fill"] * 1e-3) / 1e9 / HBM_PEAK_GBS
                            if avg["ms_fill"] > 0 else None},
            "work": {k: int(st0[k]) for k in ("n_items", "n_band_entries", "n_sign_entries", "n_tiles", "n_active_tiles", "n_active_sign_tiles")},
        }
        if dumped:
            out["outputs"] = {"dir": args.dump_outputs, "dtype": "float64", "seed": DUMP_SEED, **dumped}
        if args.full and world == 1 and not args.no_e2e:
            out["e2e"] = e2e_leg(pkg, X, IEN, rho_n, rho_t, grid, dev_index, sg)
            # SURVEY 8(d)'s contract figure (H2D of the mesh + kernels + D2H of the volume) beside `value` (kernels only,
            # inputs and output resident in HBM, steady state with the sizes of the previous identical call)
            leg = out["e2e"][out["e2e"]["default_leg"]]
            out["e2e_Mvoxels_per_s"] = leg["Mvoxels_per_s_median"]
            out["e2e_Mvoxels_per_s_best"] = leg["Mvoxels_per_s"]
            out["value_note"] = ("`value` = kernels only, HBM-resident, steady state, mean over the timed steps; e2e_Mvoxels_per_s = "
                                 "r2s_sdf on host pointers into an ordinary (pageable) array - what the Julia binding allocates by "
                                 "default - PCIe-inclusive (SURVEY 8(d)), MEDIAN of 8 calls (e2e_Mvoxels_per_s_best: the fastest; "
                                 "e2e.*.host_phases_ms_*: where a call's time went); e2e.rho2sdf_default_options = the whole rho2sdf()")
        if args.full and not args.no_cpu_baseline:
            threads = args.cpu_threads or min(16, len(os.sched_getaffinity(0)))
            cb, ref = cpu_baseline(args, threads)
            if world == 1:
                out["cpu_baseline"] = cb      # timed on rank 0 at N = 1 only
            # the `max|err| vs ref` half of the metric: worker 0's planes against the stitched GPU volume
            got = sg.volume()[::args.cpu_stride].cpu().numpy().ravel()
            want = ref.ravel()
            sent = np.abs(want) > 1e9
            real = ~sent
            rel = np.abs(got[real] - want[real]) / np.maximum(np.abs(want[real]), 1e-300)
            out["check"] = {"against": f"CPU oracle (oracle/r2s_oracle.c), Z planes k % {args.cpu_stride} == 0",
                            "voxels": int(want.size), "sentinel_mismatch": int((sent != (np.abs(got) > 1e9)).sum()),
                            "sign_mismatch": int((np.sign(got) != np.sign(want)).sum()),
                            "max_rel_err": float(rel.max()) if rel.size else 0.0,
                            "max_abs_err": float(np.abs(got[real] - want[real]).max()) if rel.size else 0.0,
                            "bit_equal": int((got == want).sum())}
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
