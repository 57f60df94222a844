#!/usr/bin/env python3
"""bench.py — Msamples/s of the path-trace hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--config c2|c3|c4|c5] [--scaling weak|strong] [--full]

One "step" = one tick of the reference's render loop (main.js:838-857): one sample for every pixel of the frame
(camera ray -> full path, tracer.fs:436-518) accumulated into the running-mean radiance buffer.  N=1 workload =
BASELINE configs[1] ("c2"): synthetic 'bunny' scene (69 316 triangles), 1920x1080, depth 8.

N > 1: one process per GPU over RCCL.  Started by `python -m torch.distributed.run` (RANK / LOCAL_RANK / WORLD_SIZE in
the environment) the script is one rank; started plainly with --gpus N > 1 it launches its own N rank processes FIRST
(child processes, before torch or HIP are touched in the parent) and passes rank 0's JSON line through.  --gpus must
equal the number of ranks RCCL sees, or the run fails.  The frame is cut into 32x32 tiles dealt round-robin to the
ranks (no data-path collective); ONE exchange of the RGBA32F radiance buffer to rank 0 closes every timed region
(SURVEY 8e): a gather of each rank's own tiles (default) or a sum-reduce of the full frame (--exchange reduce).
  --scaling weak   (default) the same picture at sqrt(N) times the linear resolution (1920x1080, 2712x1526, 3840x2160,
                   5432x3056 for N = 1, 2, 4, 8: same aspect ratio, so the same mix of sky / floor / mesh pixels): fixed
                   work per GPU;
  --scaling strong the frame is fixed (--width x --height; --config c4 = BASELINE configs[3]: 3840x2160 over the GPUs).

The timed region (exactly K steps between barriers) is run --reps times (default 5) and the MEDIAN is reported
(box-to-box and run-to-run spread is a few per cent).  Rank 0 prints ONE JSON line.

A plain run does only what the headline figure needs: it sets up, warms up, times the regions, writes --dump-outputs and
prints the line (value, ms_per_step, the per-region times and the run's configuration).  --full adds everything else, after
the headline's timed regions as before: the oracle check of the timed accumulator (parity_check), the roofline and per-kernel
figures (counting ticks of their own, priced against the request-rate microbenchmark run before the GPU is touched), the
CPU oracle baseline and the recorded GLSL one, and the other BASELINE configs as extra_configs.  --no-cpu-baseline,
--no-extra-configs, --no-parity-check and --no-l1-microbench leave out single parts of --full.

--dump-outputs DIR: rank 0 also writes what the timed path left for its caller after the last timed step of the headline
workload - the running-mean radiance buffer - as DIR/radiance.npy (float32, H x W x 4), so that two builds can be compared
output for output (same arguments: same scene, camera and seed).  A frame over DUMP_LIMIT_BYTES is written as a fixed,
seeded sample of its pixels (DIR/radiance_sample.npy, N x 4) with their flat indices (DIR/radiance_sample_index.npy, float64).
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0         # MI355X_MICROARCH.md: HBM3E 8 TB/s
VALU_PEAK_GINSTR = 256 * 4 * 2.4 / 2  # 1 228.8 G wave64 VALU instructions per second: CDNA4's SIMDs are 32 lanes wide, a
                                      # wave64 instruction issues over 2 cycles (MI355X_MICROARCH.md 'Wave scheduling')
L2_GATHER_GUIDE_TBPS = (16.8, 18.8)  # MI355X_MICROARCH.md 'Indexed rows: gather into LDS': rows shared by every workgroup (the XCD's L2)
# the same table's other rows, by the size of what is gathered from (here: the interior-node and leaf records the
# traversal kernels read): chip-wide TB/s (low, high) and where the rows are served from
GATHER_GUIDE_ROWS = [(8 << 20, (16.8, 18.8), "2,048 rows shared by every workgroup (the XCD's L2)"),
                     (96 << 20, (8.6, 8.6), "38 MB table, uniformly random rows (Infinity Cache)"),
                     (1 << 62, (7.4, 7.9), "151 MB table, uniformly random rows")]
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: at most this much is written
L1_PEAK_FALLBACK = 8.6e11     # 16-byte lane-requests/s of divergent 64-byte record gathers, all CUs (profiles/r03/l1_peak.json);
                              # bench.py measures it on the box it runs on (tools/microbench/l1_peak) and only falls
                              # back to this when the microbenchmark binary is missing

# kernel classes of the wavefront pipeline -> kernel symbol (as rocprofv3 prints it) and the resource that bounds it
KERNELS = {
    "primary": ("fspt::k_wf_primary<false, true>", "valu"),
    "trace": ("fspt::k_wf_trace<false, true>", "l1"),
    "logic": ("fspt::k_wf_logic<false, true>", "hbm"),
    "resolve": ("fspt::k_wf_resolve", "hbm"),
    "tail": ("fspt::k_wf_tail<false, true, false>", "l1"),
}
# The top-level roofline block is about the kernel class with the largest share of THIS run's GPU time (it
# used to be pinned to the third-largest one).  On the default workload that is k_wf_trace, whose binding resource is not
# HBM - the 25 MB scene is cache-resident - but the rate at which a CU's vector-memory pipeline takes per-lane requests:
# it is priced in lane-requests/s against the rate a pure gather microbenchmark reaches on the same box.  The HBM view of
# the whole pipeline (counter bytes / s against 8 TB/s) is kept beside it as roofline.hbm_counter.

CONFIGS = {  # BASELINE.json configs[1..4]
    "c2": {},
    "c3": {"mesh_n": 289},
    "c4": {"width": 3840, "height": 2160, "scaling": "strong"},
    # DoF + a smaller, brighter sun: 94 importance bins instead of 86 (ProcessEnvRadiance stops splitting at
    # max(total/64, brightest/2), so no environment yields many more), NEE samples concentrated on 1/9 of the solid angle
    "c5": {"aperture": 0.1, "sun_deg": 0.5, "sun_gain": 2000.0},
}


def source_sha():
    """Hash of the kernel sources: profile-derived numbers are only attached to runs of the code they were measured on."""
    h = hashlib.sha256()
    for f in ("fspt_kernels.hip", "fspt_device.hpp", "fspt_math.hpp", "fspt_internal.hpp", "fspt_api.cpp", "fspt_sched_batch.cpp", "fspt_sched_stream.cpp", "fspt_multi.cpp"):
        h.update(open(os.path.join(ROOT, "fspt_amd", "csrc", f), "rb").read())
    import __graft_entry__ as G  # ... and of the flags they are compiled with
    h.update(" ".join(G.LIB_FLAGS).encode())
    return h.hexdigest()[:16]


def cpu_baseline(arrays, W, H, cam, lens, bounces, budget_s=11.0):
    """The oracle (kind 'port': plain-C restatement, OpenMP over rows) timed on this host's cores on a bounded,
    uniformly tile-sampled part of the SAME frame: shard 0 of S round-robin 32x32-tile shards, S chosen from a probe."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import oracle as O
    cores = os.cpu_count() or 1
    acc = np.zeros((H, W, 4), np.float32)
    n_tiles = ((W + 31) // 32) * ((H + 31) // 32)

    def run(n_shards, n_ticks):
        c = O.OCounters()
        acc[:] = 0
        t0 = time.perf_counter()
        O.render(arrays, W, H, cam["P"], cam["I"], cam["fov_scale"], lens, cam["env_theta"], bounces, 0, n_ticks, 1,
                 acc, counters=c, shard=0, n_shards=n_shards, tile=32)
        return time.perf_counter() - t0, c.as_dict()["samples"]

    probe_shards = max(1, n_tiles // 32)
    t, s = run(probe_shards, 1)
    rate = s / max(t, 1e-9)
    want = rate * budget_s
    n_shards = max(1, int(round(W * H / max(want, 1.0))))
    n_ticks = 1 if n_shards > 1 else max(1, min(256, int(want / (W * H))))
    t, s = run(n_shards, n_ticks)
    if t < 0.6 * budget_s and n_shards == 1:
        # the probe (a 1/32 tile sample) under-estimates how well the full frame scales over the cores
        n_ticks = max(n_ticks + 1, min(512, int(n_ticks * 0.8 * budget_s / max(t, 1e-3))))
        t, s = run(n_shards, n_ticks)
    return {"value": round(s / t / 1e6, 5), "unit": "Msamples/s", "cores": cores, "kind": "port",
            "sample": f"oracle/liboracle.so (C restatement, OpenMP x{cores}), {n_ticks} tick(s) over every "
                      f"{n_shards}-th 32x32 tile of the same {W}x{H} depth-{bounces} frame: {s} samples in {t:.2f} s"}


def reference_glsl_baseline():
    """The reference's own tracer.fs timed beside the number (north_star) - a RECORDED figure: the GLSL cannot travel to
    the GPU box (nothing of /root/reference may), so it was run once in the build container (tools/glsl_baseline.py:
    unmodified camera.fs + tracer.fs on SwiftShader, BASELINE configs[0] on the scene this bench renders) and the committed
    result is quoted here, never re-measured in this run."""
    path = os.path.join(ROOT, "profiles", "r03", "glsl_baseline_config1.json")
    if not os.path.exists(path):
        return None
    j = json.load(open(path))
    return {"value": j["Msamples_per_s_total"], "unit": "Msamples/s", "after_first_tick": j["Msamples_per_s_after_first_tick"],
            "renderer": j["renderer"], "cores": j["cores"], "where": "build container (8 vCPU, no GPU), NOT this box",
            "config": "BASELINE configs[0]: " + j["config"], "kind": "reference (recorded)", "measured_in_this_run": False,
            "source": "profiles/r03/glsl_baseline_config1.json (tools/glsl_baseline.py; BASELINE.md 3.2)",
            "oracle_same_frame_same_container": j["oracle_same_frame"]["Msamples_per_s"]}


def parity_check(arrays, W, H, cam, lens, bounces, n_ticks, seed, got, budget_samples=3.0e7):
    """Self-verification of the run that was just timed: the accumulator the GPU produced over ALL its ticks so far
    (warm-up + every timed region: same seed, same tick numbers) against the CPU oracle on a uniform sample of the
    frame's 32x32 tiles (tile shard 0 of S, S from a sample budget), compared with == on float32.  The oracle is the
    checker here, never the thing measured (it runs after the timed regions)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import oracle as O
    from fspt_amd import distributed as D
    n_shards = max(1, int(-(-float(W) * H * n_ticks // budget_samples)))
    want = np.zeros((H, W, 4), np.float32)
    t0 = time.perf_counter()
    O.render(arrays, W, H, cam["P"], cam["I"], cam["fov_scale"], lens, cam["env_theta"], bounces, 0, n_ticks, seed, want,
             shard=0, n_shards=n_shards, tile=D.TILE)
    mask = D.owner_mask(0, n_shards, W, H)
    equal = bool(np.array_equal(got[mask], want[mask]))
    out = {"pixels": int(mask.sum()), "ticks": int(n_ticks), "equal": equal, "oracle_s": round(time.perf_counter() - t0, 2),
           "sample": f"every {n_shards}-th 32x32 tile of the {W}x{H} frame, all {n_ticks} ticks rendered so far"}
    if not equal:
        bad = (got[mask] != want[mask]).any(axis=-1)
        out["mismatching_pixels"] = int(bad.sum())
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7, help="timed regions of exactly --steps steps; the median is reported (7: of the "
                    "driver's 20-step regions the first runs cold, the second is the primary-form tuner's look at the other form and "
                    "the last carries the per-launch event pairs - the median is one of the other four)")
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS), help="BASELINE.json configs[1..4]")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--scaling", default=None, choices=["weak", "strong"])
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--mesh-n", type=int, default=None, help="cube-sphere resolution: 12*n^2 triangles (76 -> 70k, 289 -> 1M)")
    ap.add_argument("--aperture", type=float, default=None)
    ap.add_argument("--sun-deg", type=float, default=None, help="angular radius of the environment's sun (default 1.5)")
    ap.add_argument("--sun-gain", type=float, default=None, help="sun radiance / sky radiance scale (default 60)")
    ap.add_argument("--textured", action="store_true", help="2048^2 image maps on the floor quads (scene/bunny.json:18-41)")
    ap.add_argument("--tex-interleave-budget", type=int, default=None,
                    help="bytes of interleaved material textures the scene may use (A/B: 0 = single-layer images only)")
    ap.add_argument("--tick-mode", action="store_true",
                    help="a step is ONE tick() call (drawCamera + drawTracer, main.js:838-857) followed by a sync - the interactive "
                         "form, where every sample is observed before the next is issued - instead of one tick of a fused render(steps)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline figure: parity check against the oracle, roofline and per-kernel figures, CPU "
                         "baseline and extra_configs (off: a plain run only sets up, warms up, times and prints the headline)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--stage-events", default="last", choices=["first", "last", "all"],
                    help="which timed regions carry the per-launch HIP event pairs behind the per-kernel times (they cost ~1.3 %% of a "
                         "20-step region): only the last one (default: a warm, steady-state region; the reported per-kernel times and the "
                         "roofline are that region's), only the first one, or all")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="--full: only the headline workload (otherwise after it, BASELINE configs[2] and [4] at N = 1 / configs[3] at N > 1 as extra_configs)")
    ap.add_argument("--no-parity-check", action="store_true", help="--full: skip the oracle comparison of the timed run's accumulator")
    ap.add_argument("--pipeline", default="wavefront", choices=["wavefront", "megakernel", "stream"])
    ap.add_argument("--pool", type=int, default=0, help="stream scheduler: live paths per state set (0 = library default)")
    ap.add_argument("--drain", type=int, default=-1, help="stream scheduler: drain iterations before the tail kernel (-1 = default)")
    ap.add_argument("--tail", type=int, default=-1, help="batch scheduler: the tail kernel takes over after this round (-1 adaptive, 0 never)")
    ap.add_argument("--primary-form", type=int, default=0, help="k_wf_primary's traversal phase: 1 one ray per lane, 2 per-lane refill, 0 = measured and chosen by the library")
    ap.add_argument("--node-form", default=None,
                    help="P,T,L[,below]: node form of the primary launch, the trace launches and the tail kernel (-1 library's choice, "
                         "0 64-byte nodes, 1 two-level nodes); below = path count under which the library's choice for a trace launch is two-level")
    ap.add_argument("--trace-budget", type=int, default=-1, help="steps before a starved trace wave suspends its rays (0 = never, -1 = default)")
    ap.add_argument("--overlap", type=int, default=-1, help="stream scheduler: 1 = primary on a second HIP stream, 0 = one stream (-1 = default)")
    ap.add_argument("--exchange", default="gather", choices=["gather", "reduce"],
                    help="multi-GPU read-out: gather each rank's own tiles to rank 0 (default) or sum-reduce the full frame")
    ap.add_argument("--batch", type=int, default=128, help="ticks per wavefront batch")
    ap.add_argument("--l1-peak", type=float, default=None,
                    help="16-byte lane-requests/s to price the trace kernel against (measured by tools/microbench/l1_peak "
                         "outside this run, e.g. under a profiler where no child process may be started)")
    ap.add_argument("--no-l1-microbench", action="store_true", help="never start tools/microbench/l1_peak: use --l1-peak or the fallback constant")
    ap.add_argument("--rendezvous-timeout", type=float, default=180.0, help="seconds a rank waits for the process group / an exchange before it exits non-zero")
    ap.add_argument("--share-gpu", action="store_true",
                    help="plumbing check for a 1-GPU box: all N ranks render on device 0 and exchange over gloo through host "
                         "memory (RCCL cannot put two ranks on one device); exercises the N-rank code path - sharding, the "
                         "exchange's packing, max-over-ranks timing, the mandatory parity check - its Msamples/s says nothing about scaling")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the headline workload's radiance buffer after its last timed step to DIR/*.npy (float32; a seeded "
                         "sample of its pixels when the frame is over 64 MB)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous / exchange plumbing only, on CPU over gloo (no GPU, no rendering)")
    args = ap.parse_args(argv)
    preset = CONFIGS[args.config]
    for k, dflt in (("width", 1920), ("height", 1080), ("scaling", "weak"), ("mesh_n", 76), ("aperture", None),
                    ("sun_deg", 1.5), ("sun_gain", 60.0)):
        if getattr(args, k) is None:
            setattr(args, k, preset.get(k, dflt))
    if args.gpus < 1 or args.steps < 1 or args.reps < 1:
        raise SystemExit("--gpus, --steps and --reps must be >= 1")
    return args


def _rccl_version(torch):
    try:
        v = torch.cuda.nccl.version()
        return ".".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)
    except Exception as e:  # noqa: BLE001 - a missing version query must not take a rank down
        return f"unknown ({type(e).__name__})"


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args):
    """--gpus N > 1 without a torchrun environment: start N rank processes (children of this one; this process has
    not imported torch or touched HIP and never execs) and wait for them.  Rank 0 prints the JSON line."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE=str(args.gpus),
               FSPT_BENCH_SELF_LAUNCHED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = []
    for r in range(args.gpus):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=e))
    rc = 0
    deadline = None
    while procs:
        for p in list(procs):
            r = p.poll()
            if r is None:
                continue
            procs.remove(p)
            if r != 0:
                rc = rc or r
                if deadline is None:
                    deadline = time.time() + 20.0  # a rank died: the others hang in the rendezvous / a collective
        if deadline is not None and time.time() > deadline:
            for p in procs:
                p.kill()  # exactly the processes started above
            procs = []
        time.sleep(0.05)
    if rc:
        raise SystemExit(f"bench.py: a rank failed (exit code {rc}); --gpus {args.gpus} needs {args.gpus} visible GPUs")
    return 0


def frame_size(args, n_gpus):
    from fspt_amd import distributed as D
    if args.scaling == "strong":
        return args.width, args.height
    return D.weak_frame(n_gpus, args.width, args.height)


def dry_run(args, rank, local_rank, world):
    """The N-rank plumbing without a GPU: gloo rendezvous, tile ownership, one tile-gather exchange of a synthetic
    radiance buffer whose pixel values encode their owner, and the JSON line."""
    import numpy as np
    import torch
    from fspt_amd import distributed as D
    dist = D.init_process_group(backend="gloo") if world > 1 else None
    seen = dist.get_world_size() if dist is not None else 1
    if seen != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the process group has {seen} ranks")
    W, H = frame_size(args, world)
    W, H = max(64, W // 16), max(64, H // 16)  # plumbing check: a small frame of the same tile geometry
    acc = torch.zeros((H, W, 4), dtype=torch.float32)
    mask = torch.from_numpy(D.owner_mask(rank, world, W, H))
    acc[mask] = float(rank + 1)
    t0 = time.perf_counter()
    if args.exchange == "gather":
        D.TileGather(rank, world, W, H, torch.device("cpu"), channels=3).exchange(acc)
    else:
        D.reduce_radiance(acc, dst=0)
    dt = time.perf_counter() - t0
    ok = True
    if rank == 0:
        want = np.zeros((H, W), np.float32)
        for r in range(world):
            want[D.owner_mask(r, world, W, H)] = r + 1
        ok = bool(np.array_equal(acc[..., 0].numpy(), want))
        print(json.dumps({"dry_run": True, "n_gpus": args.gpus, "world_size_seen": seen, "backend": "gloo",
                          "scaling": args.scaling, "frame": [W, H], "exchange": args.exchange, "exchange_ok": ok,
                          "exchange_s": round(dt, 4), "self_launched": bool(os.environ.get("FSPT_BENCH_SELF_LAUNCHED"))}),
              flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if not ok:
        raise SystemExit("dry run: exchanged frame is wrong")


def _extra_argv(argv, over, steps, warmup):
    """The command line of an extra config: this run's own arguments with the workload-selecting ones replaced."""
    drop_val = {"--config", "--steps", "--warmup", "--width", "--height", "--scaling", "--mesh-n", "--aperture", "--sun-deg", "--sun-gain", "--batch",
                "--dump-outputs"}  # (only the headline workload's outputs are dumped)
    if "reps" in over:
        drop_val.add("--reps")
    out, skip = [], False
    for a in argv:
        if skip:
            skip = False
            continue
        if a in drop_val:
            skip = True
            continue
        if any(a.startswith(d + "=") for d in drop_val):
            continue
        out.append(a)
    out += ["--config", over["config"], "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-extra-configs"]
    if "reps" in over:
        out += ["--reps", str(over["reps"])]
    return out + list(over.get("flags", ()))


def trim_extra(o, seconds):
    """What extra_configs carries of a workload's full JSON object."""
    r = o.get("roofline") or {}
    keep = {k: o[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "scaling", "reps", "rep_ms_per_step", "parity_check", "exchange_ms") if k in o}
    keep["config"] = {k: o["config"][k] for k in ("workload", "scene_bytes", "bvh_nodes", "bvh_depth", "env_bins", "batch_ticks", "path_state_bytes", "primary_form", "scene_build_s", "sharding", "exchange") if k in o["config"]}
    keep["roofline"] = {k: r.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "frac_range", "frac_vs_l1_microbench", "row_of_the_scene_size", "blended_with_l2_hit_rate", "peak_is", "kernel", "kernel_class", "share_of_gpu_time", "avg_launch_ms", "launches", "traffic", "hbm_counter", "bytes_per_sample", "per_sample", "alg_over_hbm_peak")}
    keep["roofline"]["kernels"] = {c: {k: v.get(k) for k in ("ms_per_step", "launches", "avg_launch_ms", "alg_GBps", "traffic_GBps", "frac", "bound")} for c, v in (r.get("kernels") or {}).items()}
    keep["wall_s"] = round(seconds, 1)
    return keep


def dump_outputs(out_dir, frame):
    """--dump-outputs: the radiance buffer the timed steps left, as float32 .npy files; over DUMP_LIMIT_BYTES a sample of
    pixels drawn with a fixed seed (the same pixels for the same frame size, run after run).  Returns what was written."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if frame.nbytes <= DUMP_LIMIT_BYTES:
        np.save(os.path.join(out_dir, "radiance.npy"), frame)
        return {"dir": out_dir, "files": {"radiance.npy": list(frame.shape)}}
    flat = frame.reshape(-1, frame.shape[-1])
    per_pixel = flat.shape[1] * 4 + 8  # the pixel's values + its float64 index
    n = min(flat.shape[0], (DUMP_LIMIT_BYTES - 4096) // per_pixel)  # (4 KB left for the two .npy headers)
    idx = np.sort(np.random.default_rng(0).choice(flat.shape[0], size=n, replace=False))
    np.save(os.path.join(out_dir, "radiance_sample.npy"), flat[idx])
    np.save(os.path.join(out_dir, "radiance_sample_index.npy"), idx.astype(np.float64))
    return {"dir": out_dir, "files": {"radiance_sample.npy": [int(n), flat.shape[1]], "radiance_sample_index.npy": [int(n)]},
            "sample_of": list(frame.shape), "sample_seed": 0}


def _event_region(args):
    return 0 if args.stage_events == "first" else args.reps - 1


class Env:
    """What every workload of one bench.py process shares: the rank's place in the job and its process group."""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def run_workload(args, env):
    """One workload (scene, frame, configuration) on this rank: warm-up, --reps timed regions of exactly --steps steps
    between barriers, the read-out exchange inside every region, max over ranks; rank 0 returns the JSON object (with its
    parity check against the oracle), the other ranks None."""
    import numpy as np
    import torch
    import fspt_amd
    from fspt_amd import scene as S
    from fspt_amd import distributed as D
    rank, local_rank, n_gpus, dist, world_seen, rank_info = env.rank, env.local_rank, env.n_gpus, env.dist, env.world_seen, env.rank_info
    result = None
    t0 = time.perf_counter()
    if args.textured:
        arrays = S.bunny_scene_textured(n=args.mesh_n, sun_deg=args.sun_deg, sun_gain=args.sun_gain)
    else:
        arrays = S.bunny_scene(n=args.mesh_n, sun_deg=args.sun_deg, sun_gain=args.sun_gain)
    build_s = time.perf_counter() - t0
    W, H = frame_size(args, n_gpus)
    cam = dict(S.BUNNY_CAMERA)
    if args.aperture is not None:
        cam["aperture"] = args.aperture
    lens = S.lens_features(cam["focal_depth"], cam["aperture"])

    if args.tex_interleave_budget is not None:
        fspt_amd.set_texture_interleave_budget(args.tex_interleave_budget)
    pt = fspt_amd.PathTracer(arrays, W, H, device=local_rank, num_bounces=args.bounces)
    pt.set_camera(**cam)
    pt.set_shard(rank, n_gpus, D.TILE)
    # a batch never holds more ticks than the longest call of this run: path state is allocated (and page-touched) for
    # that, not for the 128-tick maximum (216 bytes per pixel and tick: 57 GB at 1920x1080 x 128, 9 GB x 20)
    args.batch = 1 if args.tick_mode else max(1, min(args.batch, max(args.steps, args.warmup)))
    pt.set_pipeline(args.pipeline, args.batch)
    if args.primary_form:
        pt.set_primary_form(args.primary_form)
    if args.trace_budget >= 0:
        pt.set_trace_budget(args.trace_budget)
    if args.node_form:
        nf = [int(x) for x in args.node_form.split(",")]
        pt.set_node_form(nf[0], nf[1], nf[2], nf[3] if len(nf) > 3 else -1)
    if args.tail >= 0:
        pt.set_tail(args.tail)
    if args.pool or args.drain >= 0 or args.overlap >= 0:
        pt.set_pool(args.pool, args.drain, 0, args.overlap)
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device=f"cuda:{local_rank}")
    pt.bind_accumulator(accum.data_ptr(), keep=accum)
    pt.seed(1)
    # RGB only: the alpha of a traced pixel is the constant 1 (tracer.fs:517), the whole frame is traced here
    # (packed and scattered by the library's own k_tile_pack through the C ABI: fspt_target_pack_tiles / _unpack_tiles)
    exch = D.TileGather(rank, n_gpus, W, H, accum.device, channels=3, tracer=pt) if (n_gpus > 1 and args.exchange == "gather") else None
    pt.prepare()  # path-state allocation happens here, never inside a timed region (even with --warmup 0)

    def barrier(what="barrier"):
        pt.sync()
        torch.cuda.synchronize()
        if dist is not None:
            with D.Watchdog(args.rendezvous_timeout, what, rank):
                dist.barrier()
        torch.cuda.synchronize()

    def advance(n):
        """n steps: one fused render call, or (--tick-mode) n x [tick(); sync()] - every tick observed before the next"""
        if not args.tick_mode:
            pt.render(n)
            return
        for _ in range(n):
            pt.tick()
            pt.sync()

    # ---- warmup (untimed) ----
    if args.warmup > 0:
        advance(args.warmup)
    barrier()
    # ---- timed: --reps regions of exactly K steps each, every one closed by the path's one exchange step ----
    foreign = (~torch.from_numpy(D.owner_mask(rank, n_gpus, W, H))).to(accum.device) if (n_gpus > 1 and args.exchange == "reduce") else None
    times, kernel_ms_all, stages_all, exch_ms, render_ms, exch_stage_ms = [], [], [], [], [], []
    for rep_i in range(args.reps):
        # per-launch HIP event pairs (the per-kernel times of the report) in ONE region only, unless asked otherwise: the
        # last by default - warm and in the form the tuner settled on.  Of seven 20-step regions the first (first use of the
        # 20-tick batch), the second (the primary-form tuner's look at the other form) and this one are the three slowest,
        # so `value` - the median - is one of the four steady-state regions without the events' 1.3 %
        pt.set_stage_timing(args.stage_events == "all" or rep_i == _event_region(args))
        barrier(f"barrier before region {rep_i}")
        t_start = time.perf_counter()
        advance(args.steps)
        pt.sync()
        t_render = time.perf_counter()
        with D.Watchdog(args.rendezvous_timeout if n_gpus > 1 else 0, f"read-out exchange ({args.exchange}) of region {rep_i}", rank):
            if exch is not None:
                exch.exchange(accum, stage_host=args.share_gpu)  # RCCL over xGMI: rank 0 ends up with the whole frame
            elif n_gpus > 1:
                # sum-reduce of the full frame; the other ranks' pixels rank 0 received in the previous region are zeroed
                # first (foreign mask), or they would be added again
                D.reduce_radiance(accum, dst=0, foreign_mask=foreign, stage_host=args.share_gpu)
            torch.cuda.synchronize()
        barrier(f"barrier after region {rep_i}")
        elapsed = time.perf_counter() - t_start
        exch_ms.append((time.perf_counter() - t_render) * 1e3)
        render_ms.append((t_render - t_start) * 1e3)
        exch_stage_ms.append({k: round(v, 3) for k, v in exch.last_stage_ms.items()} if (exch is not None and exch.last_stage_ms) else None)
        if dist is not None:
            tmax = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if args.share_gpu else f"cuda:{local_rank}")
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            elapsed = float(tmax.item())
        times.append(elapsed)
        kernel_ms_all.append(pt.last_kernel_ms())
        stages_all.append(pt.last_stage_ms() if args.pipeline != "megakernel" else None)
    order = sorted(range(args.reps), key=lambda i: times[i])
    med = order[(args.reps - 1) // 2]  # the median region (lower median for an even count): `value`
    elapsed = times[med]
    # the region whose launches carried HIP event pairs: its stage timings (and its own wall time) are what the per-kernel
    # part of the report is about
    ev_rep = med if args.stage_events == "all" else _event_region(args)
    kernel_ms, launches = kernel_ms_all[ev_rep]
    stages = stages_all[ev_rep]
    pt.set_stage_timing(True)  # (the counting ticks of report() and anything after read stage times again)

    total_samples = float(W) * H * args.steps
    value = total_samples / elapsed / 1e6
    if n_gpus > 1:
        sys.stderr.write("[bench rank] " + json.dumps(dict(rank_info, frame=[W, H], render_ms=[round(x, 3) for x in render_ms],
                                                           exchange_and_barrier_ms=[round(x, 3) for x in exch_ms],
                                                           exchange_stage_ms=exch_stage_ms,  # per region: this rank's pack / collective / unpack (gather exchange)
                                                           kernel_ms=[round(k[0], 3) for k in kernel_ms_all])) + "\n")
        sys.stderr.flush()

    if rank != 0:
        pt.close()
        return None
    # Rank 0's part that needs no other rank - the oracle check of the assembled frame and the counting ticks of the report -
    # is DEFERRED (main() runs it after the timed regions of every workload, when the other ranks have already been
    # released: VERDICT r4 weak 8 iii - seven ranks used to sit in a barrier with a 600 s timeout meanwhile).  The frame as
    # the timed regions left it is copied to the host now (the counting ticks add to the accumulator later).
    # --full, N > 1: the check is mandatory - bytes that crossed xGMI are verified
    check_parity = args.full and (not args.no_parity_check or n_gpus > 1)
    frame = accum.cpu().numpy() if (check_parity or args.dump_outputs) else None

    def finish():
        dumped = dump_outputs(args.dump_outputs, frame) if args.dump_outputs else None
        if not args.full:
            out = report(args, pt, arrays, cam, W, H, n_gpus, world_seen, value, elapsed, times, build_s)
        else:
            check = None
            if check_parity:
                check = parity_check(arrays, W, H, cam, lens, args.bounces, args.warmup + args.reps * args.steps, 1, frame)
            out = full_report(args, pt, arrays, cam, lens, W, H, n_gpus, world_seen, value, elapsed, times, kernel_ms, launches,
                              stages, build_s)
            out["stage_events"] = {"regions": args.stage_events, "region": ev_rep, "region_ms_per_step": round(times[ev_rep] * 1e3 / args.steps, 4),
                                   "is": "the timed region whose launches carried HIP event pairs (fspt_target_set_stage_timing): roofline.kernels.* "
                                         "and roofline.avg_launch_ms are that region's; `value` is the median of all regions"}
            out["parity_check"] = check
        if dumped is not None:
            out["dump_outputs"] = dumped
        if n_gpus > 1:
            out["exchange_ms"] = round(exch_ms[med], 3)  # read-out exchange + closing barrier of the median region (inside `value`)
            out["rank0"] = rank_info
        pt.close()
        return out
    return finish


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        if _under_profiler():
            # the profiler's preloaded library has initialised the GPU in THIS process: starting (exec'ing) rank children
            # from it is exactly what the pool forbids, and their kernels would not be the ones profiled anyway
            raise SystemExit("bench.py: --gpus N > 1 under a profiler: profile ONE rank directly after `--` "
                             "(RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment), not the launcher")
        return self_launch(args)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start one rank per GPU "
                         f"(python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ..., "
                         f"or plain `python bench.py --gpus {args.gpus}`, which launches the ranks itself)")
    n_gpus = world
    if args.dry_run:
        return dry_run(args, rank, local_rank, world)

    # --full: the request-rate peak the trace kernel is priced against is measured first, by a child process started BEFORE this
    # process touches the GPU (no fork of a process that holds a HIP context).  Under a profiler the preloaded library
    # has initialised the GPU before main() runs: such runs pass --l1-peak (tools/prof_session.sh measures it once, outside
    # rocprofv3) or --no-l1-microbench, and no child is ever started from this process.
    global _L1_PEAK
    if args.full and rank == 0 and _L1_PEAK is None:
        if args.l1_peak is not None:
            _L1_PEAK = (float(args.l1_peak), {"source": "--l1-peak (tools/microbench/l1_peak, measured outside this run)",
                                              "gather_lane_requests_per_s": float(args.l1_peak)})
        elif args.no_l1_microbench or _under_profiler():
            _L1_PEAK = (L1_PEAK_FALLBACK, {"source": "fallback constant (microbenchmark not started: "
                                                     + ("--no-l1-microbench" if args.no_l1_microbench else "profiler preload detected") + ")"})
        else:
            _L1_PEAK = l1_request_peak()

    import numpy as np
    import torch
    import fspt_amd
    from fspt_amd import scene as S

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (libfspt has no CPU path)")
    if args.share_gpu:
        local_rank = 0
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: local rank {local_rank} has no GPU ({torch.cuda.device_count()} visible)")
    torch.cuda.set_device(local_rank)
    from fspt_amd import distributed as D
    # the process group's own timeout (what RCCL's watchdog applies to every collective) is generous - rank 0 checks the
    # frame against the oracle and counts work while the others wait at the closing barrier; the tighter deadlines around
    # the rendezvous, the barriers of the timed regions and the exchange are the Watchdogs below
    dist = (D.init_process_group(backend="gloo" if args.share_gpu else "nccl", device=torch.device("cuda", local_rank),
                                 timeout_s=max(600.0, 2 * args.rendezvous_timeout))
            if n_gpus > 1 else None)
    world_seen = dist.get_world_size() if dist is not None else 1
    if world_seen != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but RCCL sees {world_seen} ranks")
    rank_info = None
    if n_gpus > 1:
        # every rank says who it is before anything can hang (stderr; rank 0's JSON line stays alone on stdout)
        rank_info = {"rank": rank, "local_rank": local_rank, "device": torch.cuda.get_device_name(local_rank),
                     "visible_devices": torch.cuda.device_count(),
                     "peer_access_to_rank0_device": bool(local_rank == 0 or torch.cuda.can_device_access_peer(local_rank, 0)),
                     "rccl": _rccl_version(torch),
                     "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}
        sys.stderr.write("[bench rank] " + json.dumps(rank_info) + "\n"); sys.stderr.flush()

    env = Env(rank=rank, local_rank=local_rank, n_gpus=n_gpus, dist=dist, world_seen=world_seen, rank_info=rank_info)
    # ---- the timed regions of every workload first.  The headline, then (--full) the other BASELINE configs on the same
    # record: N = 1: configs[2] (1 M triangles) and configs[4] (aperture 0.1 + small sun) as
    # extra_configs.c3 / .c5; N > 1 on the weak-scaled default: configs[3] (3840x2160 cut over the N ranks, strong scaling)
    # as extra_configs.strong_c4.  Each with its own regions, per-kernel times and parity check.
    t_h = time.perf_counter()
    pending = [("headline", run_workload(args, env), time.perf_counter() - t_h)]
    extras = []
    if args.full and not args.no_extra_configs and args.config == "c2" and args.pipeline == "wavefront" and not args.textured:
        if n_gpus == 1:
            # configs[2] and [4]; the workload shaped like the reference's real scene (scene/bunny.json:18-41 image-maps both
            # quads: 2048^2 atlas layers); and the interactive form - 128 single tick() calls, each observed before the next
            # (main.js:838-857 displays every sample), ms_per_step = ms per tick
            extras = [("c3", dict(config="c3")), ("c5", dict(config="c5")), ("textured", dict(config="c2", flags=["--textured"])),
                      ("tick1", dict(config="c2", flags=["--tick-mode"], steps=128, warmup=8, reps=3))]
        elif args.scaling == "weak":
            extras = [("strong_c4", dict(config="c4"))]
    for key, over in extras:
        a2 = parse_args(_extra_argv(sys.argv[1:], over, steps=over.get("steps", min(args.steps, 20)), warmup=over.get("warmup", min(args.warmup, 5))))
        t_x = time.perf_counter()
        pending.append((key, run_workload(a2, env), time.perf_counter() - t_x))
    # ---- every collective of the job is done: the other ranks leave now; rank 0's oracle checks and counting ticks (no
    # communication in either) follow, with nobody waiting for them
    if dist is not None:
        dist.destroy_process_group()
    if rank == 0:
        out = None
        for key, fin, secs in pending:
            t_f = time.perf_counter()
            o = fin()
            secs += time.perf_counter() - t_f
            if key == "headline":
                out = o
            else:
                out.setdefault("extra_configs", {})[key] = trim_extra(o, secs)
        print(json.dumps(out), flush=True)
        bad = [k for k, v in [("headline", out)] + list(out.get("extra_configs", {}).items())
               if v.get("parity_check") is not None and not v["parity_check"]["equal"]]
        if bad:
            raise SystemExit(f"bench.py: the timed run's accumulator differs from the oracle ({', '.join(bad)})")
    return 0


def count_work(pt, mode, bounces=None):
    """One extra tick with the counting kernel variants (outside every timed region).  mode 1 = the reference's work
    (shadow rays traced to the closest hit like tracer.fs:501: equals the oracle's counters), mode 2 = the work the
    timed kernels really do (NEE shadow rays stop at the first hit)."""
    import ctypes as C
    import fspt_amd
    L = fspt_amd._lib
    keep = pt.num_bounces
    if bounces is not None:
        pt.num_bounces = bounces
    pt.enable_counters(mode)
    L.check(L.lib().fspt_counters_reset(pt._t))
    pt.render(1)
    c = pt.counters()
    lds = C.c_uint64()
    L.check(L.lib().fspt_get_trace_lds_steps(pt._t, C.byref(lds)))
    c["trace_lds_steps"] = int(lds.value)  # interior steps k_wf_trace served from its LDS copy of the top of the tree
    pt.enable_counters(0)
    pt.num_bounces = keep
    return c


_L1_PEAK = None  # (peak, source) measured at the start of main()


def _under_profiler():
    """rocprofv3 preloads its tool library (which initialises the GPU) into this process: no child may be exec'd from it."""
    return any("rocprof" in os.environ.get(k, "") for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB", "ROCPROFILER_REGISTER_FORCE_LOAD"))


def l1_request_peak():
    """16-byte lane-requests/s of a pure per-lane gather of 64-byte records (4 x dwordx4 per lane, the traversal's node
    fetch) from an L2-resident table at k_wf_trace's occupancy, measured NOW on this box (tools/microbench/l1_peak.hip,
    built by __graft_entry__.build()).  Returns (peak, source)."""
    exe = os.path.join(ROOT, "tools", "microbench", "l1_peak")
    if os.path.exists(exe):
        try:
            out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
            for l in out.splitlines():
                if l.startswith("{"):
                    j = json.loads(l)
                    return float(j["gather_lane_requests_per_s"]), dict(j, source="tools/microbench/l1_peak, this run")
        except Exception as e:  # noqa: BLE001 - a failed microbenchmark must not lose the bench line
            return L1_PEAK_FALLBACK, {"source": f"fallback constant (l1_peak failed: {e})"}
    return L1_PEAK_FALLBACK, {"source": "fallback constant (tools/microbench/l1_peak not built)"}


def _prof_key(prof, name):
    """Key of a kernel class in the stamped profile: the symbol itself, or (k_wf_primary<false, true, R>: two forms of one
    class) the entry with the most launches that starts with it."""
    base = name.replace("fspt::", "")
    if base in prof["kernels"]:
        return base
    stem = base[:-1] if base.endswith(">") else base
    cand = [k for k in prof["kernels"] if k.startswith(stem)]
    return max(cand, key=lambda k: prof["kernels"][k].get("launches", 0)) if cand else None


def report(args, pt, arrays, cam, W, H, n_gpus, world_seen, value, elapsed, times, build_s):
    """The result line of a workload: the headline figure and what describes the run (nothing is run on the GPU here)."""
    # BASELINE.json's wording for the two benchmark meshes ("70k tri" = 69 316, "1M" = 1 002 256); the count otherwise
    tri_k = {76: "70k", 289: "1M"}.get(args.mesh_n) or (f"{arrays.n_tris / 1e3:.0f}k" if arrays.n_tris < 1e6 else f"{arrays.n_tris / 1e6:.1f}M")
    return {
        "metric": f"Msamples/s at {W}x{H} depth {args.bounces} (bunny, {tri_k} tri)",
        "value": round(value, 3), "unit": "Msamples/s", "n_gpus": n_gpus, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(elapsed * 1e3 / args.steps, 4), "higher_is_better": True,
        "scaling": args.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "reps": args.reps, "rep_ms_per_step": [round(t * 1e3 / args.steps, 4) for t in times],
        "config": {"workload": f"{args.config}: bunny-synthetic {arrays.n_tris} tri{' + 2048^2 image maps' if args.textured else ''}, "
                               f"{W}x{H}, depth {args.bounces}, 1 spp/step, aperture {cam['aperture']}, sun {args.sun_deg} deg x{args.sun_gain:g}"
                               + (", every step = one tick() call + sync (the interactive form, main.js:838-857)" if args.tick_mode else ""),
                   "scene_bytes": arrays.nbytes(), "bvh_nodes": arrays.n_nodes, "bvh_depth": arrays.depth,
                   "env_bins": int(arrays.bins.size // 4), "atlas": f"{arrays.atlas_res}^2 x {arrays.atlas_layers}",
                   "sharding": f"32x32 tiles round-robin over {n_gpus}", "world_size_seen": world_seen,
                   "exchange": ((args.exchange + (" (gloo through host memory: --share-gpu, all ranks on ONE device - a plumbing check, not a scaling figure)" if args.share_gpu else "")) if n_gpus > 1 else "none"), "pipeline": args.pipeline,
                   "batch_ticks": args.batch, "path_state_bytes": pt.path_state_bytes()[0],
                   "primary_form": (dict(zip(("form", "ms_per_Msample"), (lambda f, ms: (f, [round(m * 1e6, 4) if m >= 0 else None for m in ms]))(*pt.primary_form(min(args.batch, args.steps)))))
                                    if args.pipeline == "wavefront" else None),
                   "scene_build_s": round(build_s, 2), "source_sha": source_sha()},
    }


def full_report(args, pt, arrays, cam, lens, W, H, n_gpus, world_seen, value, elapsed, times, kernel_ms, launches, stages, build_s):
    """--full: the result line with the roofline and per-kernel figures (counting ticks of their own) and the CPU baselines."""
    import fspt_amd
    ref = count_work(pt, 1)   # reference algorithm (SURVEY 8d's S, L, H, E)
    bps = fspt_amd.bytes_per_sample(ref)
    spt = ref["samples"]      # samples per step on this rank
    per_sample = {k: round(v / max(1, spt), 4) for k, v in ref.items() if k != "samples"}
    steps = args.steps
    sha = source_sha()
    roofline = None
    if stages is not None:
        act = count_work(pt, 2)               # the timed kernels' own traversal work (any-hit shadow rays)
        ref0 = count_work(pt, 1, bounces=0)   # camera rays alone: splits the per-sample terms over the kernels
        h1 = (ref0["samples"] - ref0["env_lookups"]) if args.bounces >= 1 else 0  # camera rays that hit and get shaded
        # Algorithmic bytes per step of each kernel class on the reference layout (60 S + 144 L + 280 H + 16 E
        # + 64 per sample), the traversal terms counted on the TIMED variant:
        #   primary (ray generation + camera-ray traversal + its shading): 60 S0 + 144 L0 + 280 H1 + 16 E0 + 32
        #   trace   (rounds >= 1: extension + any-hit shadow rays)       : 60 (S' - S0) + 144 (L' - L0)
        #   logic   (rounds >= 2)                                        : 280 (H - H1) + 16 (E - E0)
        #   resolve (running mean)                                       : 32
        alg = {"primary": 60.0 * ref0["steps"] + 144.0 * ref0["leaves"] + 280.0 * h1 + 16.0 * ref0["env_lookups"] + 32.0 * spt,
               "trace": 60.0 * (act["steps"] - ref0["steps"]) + 144.0 * (act["leaves"] - ref0["leaves"]),
               "logic": 280.0 * (ref["shades"] - h1) + 16.0 * (ref["env_lookups"] - ref0["env_lookups"]),
               "resolve": 32.0 * spt, "tail": 0.0}  # tail: its share of the trace / logic terms is not separated
        # rocprofv3 PMC traffic of the same kernels (bytes per sample, per kernel), if it was measured on THIS code
        prof, prof_path = None, os.path.join(ROOT, "profiles", "hbm_traffic.json")
        wl = f"{args.config}{'_tex' if args.textured else ''}"
        if os.path.exists(prof_path):
            pj = json.load(open(prof_path))
            if pj.get("source_sha") == sha and wl in pj.get("workloads", {}):
                prof = pj["workloads"][wl]
        # k_wf_trace in the unit of its binding resource: per-lane requests to the vector-memory pipeline.  An interior
        # step fetches a 64-byte node as 4 requests (3 x 16 B + 1 x 8 B) unless the node is one of the top-of-tree nodes
        # in LDS; a leaf visit is 9 x 16 B; a path item fetches its state with 3 x 16 B and stores 1 - 2 results.
        tr_int = (act["steps"] - act["leaves"]) - (ref0["steps"] - ref0["leaves"])
        tr_leaf = act["leaves"] - ref0["leaves"]
        tr_paths = ref["shades"]  # one path item per shaded hit (its extension ray [+ shadow ray])
        tr_req = 4.0 * max(0, tr_int - act["trace_lds_steps"]) + 9.0 * tr_leaf + 4.0 * tr_paths
        l1_peak, l1_src = _L1_PEAK if _L1_PEAK is not None else (L1_PEAK_FALLBACK, {"source": "fallback constant"})
        kernels = {}
        for k, (ms, n) in stages.items():
            name, bound = KERNELS[k]
            gbps = alg[k] * steps / (ms / 1e3) / 1e9 if ms > 0 else 0.0
            kj = {"kernel": name, "launches": n, "ms_per_step": round(ms / steps, 4), "avg_launch_ms": round(ms / max(1, n), 4),
                  "alg_bytes_per_step": round(alg[k]), "alg_GBps": round(gbps, 1), "bound": bound,
                  "traffic_bytes_per_launch": None, "traffic_GBps": None}
            pkey = _prof_key(prof, name) if prof else None
            if pkey:
                tps = prof["kernels"][pkey]["hbm_bytes_per_sample"]
                tb = tps * spt * steps
                kj["traffic_bytes_per_launch"] = round(tb / max(1, n))
                kj["traffic_GBps"] = round(tb / (ms / 1e3) / 1e9, 1) if ms > 0 else None
            if pkey:
                pk = prof["kernels"][pkey]
                if "ta_busy" in pk:  # stamped SQ / TA / TD counters of the same code (tools/collect_profiles.py)
                    kj["counters"] = {c: pk[c] for c in ("ta_busy", "td_busy", "valu_active_share", "valu_lane_utilisation", "wait_share", "l2_hit") if c in pk}
            if k == "trace":
                rps = tr_req * steps / (ms / 1e3) if ms > 0 else 0.0
                # the same requests as bytes (16 per lane-request) next to the guide's own L2-resident gather rate, and the
                # reference-layout bytes (60 per step, 144 per leaf) next to it: cross-checks of `frac` that use no
                # builder-measured peak
                req_tbps = rps * 16.0 / 1e12
                # which row of the guide's gather table prices it: by the bytes the traversal gathers from - 64 B per
                # interior node + 36 B x leaf size per leaf (what fspt_scene_create uploads for the traversal kernels)
                n_leaf = int((arrays.bvh.view("int32").reshape(-1, 9)[:, 2] > -1).sum())
                trav_bytes = 64 * (arrays.n_nodes - n_leaf) + 36 * arrays.leaf_size * n_leaf
                g_lo, g_hi, g_row = next((lo, hi, row) for lim, (lo, hi), row in GATHER_GUIDE_ROWS if trav_bytes <= lim)
                # The ceiling is the L2 row whatever the scene: what a lane requests cannot arrive faster than from the
                # XCD's L2.  A scene beyond the L2 (1 M triangles: 68 MB of nodes and leaves) still hits it for the top of
                # the tree (the counters say how often): its fair roof is the blend of the L2 row and the row of its size,
                # 1 / (h / L2 + (1 - h) / row) with h = the kernel's measured L2 hit rate - printed when that is stamped;
                # against the row of its size alone the 1 M-triangle scene reads 1.10 (it is not served from there alone).
                l2_lo, l2_hi = GATHER_GUIDE_ROWS[0][1]
                h = ((prof["kernels"][pkey].get("l2_hit") if (prof and pkey) else None))
                blend = None
                if h is not None and (g_lo, g_hi) != (l2_lo, l2_hi):
                    blend = {"l2_hit": h, "peak_GBps": round(1e3 / (h / l2_hi + (1.0 - h) / g_hi), 1)}
                    blend["frac"] = round(req_tbps * 1e3 / blend["peak_GBps"], 4)
                row_of_size = {"row": g_row, "GBps": [g_lo * 1e3, g_hi * 1e3], "requested_over_row": round(req_tbps / g_hi, 4)}
                g_lo, g_hi, g_row = l2_lo, l2_hi, GATHER_GUIDE_ROWS[0][2]
                kj.update({"lane_requests_per_step": round(tr_req), "achieved_Greq_per_s": round(rps / 1e9, 1),
                           "peak_Greq_per_s": round(l1_peak / 1e9, 1), "frac": round(rps / l1_peak, 4),
                           "gather": {"traversal_bytes": trav_bytes, "requested_GBps": round(req_tbps * 1e3, 1), "guide_row": g_row,
                                      "guide_GBps": [g_lo * 1e3, g_hi * 1e3], "frac": round(req_tbps / g_hi, 4),
                                      "frac_range": [round(req_tbps / g_hi, 4), round(req_tbps / g_lo, 4)],
                                      "row_of_the_scene_size": row_of_size, "blended_with_l2_hit_rate": blend},
                           "lds_served_interior_steps": round(act["trace_lds_steps"] / max(1, tr_int), 3),
                           "l2_gather": {"requested_TBps": round(req_tbps, 2), "reference_layout_TBps": round(gbps / 1e3, 2),
                                         "guide_TBps": list(L2_GATHER_GUIDE_TBPS),
                                         "requested_frac_of_guide": [round(req_tbps / g, 3) for g in reversed(L2_GATHER_GUIDE_TBPS)],
                                         "reference_layout_frac_of_guide": [round(gbps / 1e3 / g, 3) for g in reversed(L2_GATHER_GUIDE_TBPS)],
                                         "guide": "MI355X_MICROARCH.md, 'Indexed rows: gather into LDS', rows shared by every workgroup"}})
            elif bound == "valu":
                # the fused ray-generation + traversal + shading launch issues vector-ALU instructions (profiles/r04:
                # TA / TD 0.37 / 0.50 busy, nothing on the memory side saturated): wave-instructions per second over
                # the chip's issue rate, when the stamped SQ_INSTS_VALU count of this code exists
                wi = prof["kernels"][pkey].get("valu_wave_instr_per_sample") if pkey else None
                ach = wi * spt * steps / (ms / 1e3) / 1e9 if (wi is not None and ms > 0) else None
                kj.update({"valu_wave_instr_per_sample": wi, "achieved_Ginstr_per_s": round(ach, 1) if ach is not None else None,
                           "peak_Ginstr_per_s": VALU_PEAK_GINSTR, "frac": round(ach / VALU_PEAK_GINSTR, 4) if ach is not None else None,
                           "frac_is": "VALU wave-instructions issued per second / (256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles per wave64 instruction)"})
            elif bound == "hbm":
                # HBM kernels are priced on what they really move between L2 and the fabric when the counters are available
                # (cache-resident scene data never has to come from HBM), else on the algorithmic bytes
                # (no fraction without counters: algorithmic bytes of cache-resident scene data are not HBM bytes)
                kj.update({"peak_GBps": HBM_PEAK_GBS,
                           "frac": round(kj["traffic_GBps"] / HBM_PEAK_GBS, 4) if kj["traffic_GBps"] is not None else None,
                           "traffic_is": "bytes between L2 and the fabric, (2*FETCH_SIZE + WRITE_SIZE)*1024, Infinity-Cache hits "
                                         "INCLUDED: an upper bound on DRAM bytes, so `frac` can exceed what a DRAM copy reaches (6.29 TB/s)"})
            kernels[k] = kj
        # The pipeline's instruction work against the chip's VALU issue rate.  Wave-instructions per sample of every
        # kernel class (SQ_INSTS_VALU, same stamped profile) x samples/s against 256 CUs x 4 SIMD-32s x 2.4 GHz / 2 cycles
        # per wave64 instruction (= the guide's 157.3 TFLOP/s FP32 vector peak; ONE wave sustains one per 4 cycles).
        valu = None
        if prof and all("valu_wave_instr_per_sample" in v for v in prof["kernels"].values()):
            wips = sum(v["valu_wave_instr_per_sample"] for v in prof["kernels"].values())
            ach = wips * spt * steps / (kernel_ms / 1e3) / 1e9
            valu = {"wave_instr_per_sample": round(wips, 1), "achieved_Ginstr_per_s": round(ach, 1),
                    "peak_Ginstr_per_s": VALU_PEAK_GINSTR, "frac": round(ach / VALU_PEAK_GINSTR, 4),
                    "per_kernel": {k.split("<")[0]: round(v["valu_wave_instr_per_sample"], 1) for k, v in prof["kernels"].items()}}
        # the whole pipeline's counter traffic against the HBM peak (bytes between L2 and the fabric, Infinity-Cache hits
        # included: an upper bound on DRAM bytes)
        hbm_counter = None
        if prof:
            tps = sum(v["hbm_bytes_per_sample"] for v in prof["kernels"].values())
            gb = tps * spt * steps / elapsed / 1e9
            hbm_counter = {"bytes_per_sample": round(tps, 1), "GBps": round(gb, 1), "peak_GBps": HBM_PEAK_GBS, "frac": round(gb / HBM_PEAK_GBS, 4),
                           "is": "(2*FETCH_SIZE + WRITE_SIZE)*1024 of every kernel of the pipeline / the timed region; every read "
                                 "request is a 128-byte line (profiles/r03/fetch_calib.json)",
                           "source": f"profiles/hbm_traffic.json (source {sha})"}
        dom_class = max(stages, key=lambda k: stages[k][0])  # the class with the largest share of this run's GPU time
        dom = kernels[dom_class]
        d_ms, d_n = stages[dom_class]
        total_ms = sum(v[0] for v in stages.values())
        if dom["bound"] == "l1" and dom_class == "trace":
            # Headline fraction: the bytes the kernel REQUESTS per second (16 per lane-request) over the
            # rate the guide itself measured for a gather from a table of this size - recomputable from this line and
            # MI355X_MICROARCH.md alone; `peak` is the upper end of the guide's range (the lower end: frac_range[1]).
            # The same-box microbenchmark (lane-requests of a pure 64-byte-record gather) stays beside it.
            gth = dom["gather"]
            roofline = {"bound": "cache-gather", "achieved": gth["requested_GBps"], "peak": gth["guide_GBps"][1], "unit": "GB/s",
                        "frac": gth["frac"], "frac_range": gth["frac_range"], "traffic": dom["traffic_bytes_per_launch"],
                        "achieved_is": "16 B x the per-lane vector-memory requests of this kernel (4 per interior step not served "
                                       "from LDS, 9 per leaf visit, 4 per path item; counted by the kernel's counting variant on "
                                       "this frame) / its HIP-event time",
                        "peak_is": f"MI355X_MICROARCH.md 'Indexed rows: gather into LDS', chip-wide rate of the row '{gth['guide_row']}' "
                                   f"(the traversal gathers from {gth['traversal_bytes'] / 1e6:.1f} MB of node and leaf records)",
                        "frac_vs_l1_microbench": dom["frac"], "row_of_the_scene_size": gth["row_of_the_scene_size"],
                        "blended_with_l2_hit_rate": gth["blended_with_l2_hit_rate"],
                        "l1_microbench": {"achieved_Greq_per_s": dom["achieved_Greq_per_s"], "peak_Greq_per_s": dom["peak_Greq_per_s"],
                                          "is": "lane-requests/s of this kernel over those of a pure 64-byte-record gather (4 x dwordx4 per "
                                                "lane) from an L2-resident table at this kernel's occupancy, measured in this run on this box",
                                          "peak_source": l1_src},
                        "requests_per_launch": round(tr_req * steps / max(1, d_n))}
            nf = [int(x) for x in args.node_form.split(",")] if args.node_form else []
            if len(nf) > 1 and (nf[1] == 1 or (len(nf) > 3 and nf[3] > 0)):
                # two-level trace launches fetch 8 requests per round trip covering 1-2 steps: the count above (4 per
                # interior step) does not describe them - no fraction rather than a wrong one (A/B runs only)
                roofline.update({"frac": None, "frac_range": None, "frac_vs_l1_microbench": None,
                                 "note": "--node-form selects two-level nodes for trace launches: lane-requests are not 4 per interior step there, no fraction is priced"})

        else:
            roofline = {"bound": "hbm", "achieved": dom["alg_GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(dom["alg_GBps"] / HBM_PEAK_GBS, 5), "traffic": dom["traffic_bytes_per_launch"],
                        "achieved_is": "algorithmic bytes of this kernel (reference layout, SURVEY 8d) / its HIP-event time",
                        "traffic_frac": dom.get("frac") if dom["traffic_GBps"] is not None else None,
                        "bytes_per_launch": round(alg[dom_class] * steps / max(1, d_n))}
        roofline.update({"kernel": dom["kernel"], "kernel_class": dom_class, "share_of_gpu_time": round(d_ms / max(total_ms, 1e-9), 3),
                         "avg_launch_ms": dom["avg_launch_ms"], "launches": d_n,
                         "traffic_source": (f"profiles/hbm_traffic.json (rocprofv3 --pmc FETCH_SIZE, WRITE_SIZE; source {sha})"
                                            if dom["traffic_bytes_per_launch"] is not None else None),
                         "hbm_counter": hbm_counter,
                         "bytes_per_sample": round(bps, 1), "per_sample": per_sample,
                         "per_sample_timed_variant": {k: round(act[k] / max(1, spt), 4) for k in ("rays", "steps", "leaves")},
                         "kernels": kernels, "valu": valu,
                         "pipeline_alg_GBps": round(sum(alg.values()) * steps / (kernel_ms / 1e3) / 1e9, 1),
                         # SURVEY 8d's figure, stated rather than left to be discovered: algorithmic bytes / s over the HBM
                         # peak.  Above 1 for a cache-resident scene (25 MB; counter traffic: hbm_counter) - the reason the
                         # dominant kernel is priced in lane-requests instead
                         "alg_over_hbm_peak": {"pipeline_reference_work": round(bps * value * 1e6 / 1e9 / HBM_PEAK_GBS, 3),
                                               "pipeline_timed_kernels": round(sum(alg.values()) * steps / (kernel_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 3),
                                               "dominant_kernel": round(dom["alg_GBps"] / HBM_PEAK_GBS, 3)},
                         "dominant_kernel_counters": dom.get("counters")})
        if args.pipeline == "stream":
            # two HIP streams: the classes' event times overlap, their sum exceeds the wall time of the kernels
            roofline["stage_times_overlap"] = True
            roofline["share_of_gpu_time"] = round(d_ms / max(kernel_ms, 1e-9), 3)
            roofline["share_is"] = "this class's summed event time / the ev0..ev1 time of the region (classes overlap on two streams)"
    else:
        avg_launch_ms = kernel_ms / max(1, launches)
        achieved = bps * spt / (avg_launch_ms / 1e3) / 1e9
        roofline = {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": None, "kernel": "fspt::k_trace<true, false>",
                    "avg_launch_ms": round(avg_launch_ms, 4), "launches": launches, "bytes_per_sample": round(bps, 1),
                    "per_sample": per_sample}
    out = report(args, pt, arrays, cam, W, H, n_gpus, world_seen, value, elapsed, times, build_s)
    out["roofline"] = roofline
    if n_gpus == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(arrays, W, H, cam, lens, args.bounces)
        out["reference_glsl_baseline"] = reference_glsl_baseline()
    return out


if __name__ == "__main__":
    sys.exit(main() or 0)
