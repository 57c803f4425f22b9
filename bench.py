#!/usr/bin/env python3
"""bench.py -- frames/s of the ORB front end (extract + match) on MI355X.

One "step" = one pass of the hot path over one batch of B synthetic 1920x1080 grey frames
that are already resident in HBM: K1 pyramid -> K2 per-cell FAST -> K3 quadtree ->
K4-6 orientation+blur+rBRIEF (2000 keypoints/frame) -> K7 best-2 Hamming match of every frame
against its predecessor in the ride.  Workload = BASELINE.json configs[1].

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run does what its headline figure needs: set-up, the sustained leg (it brings the clocks up before the
warm-up), the W warm-up and K timed steps, --dump-outputs when given, and the JSON line.  --full adds everything
else the bench measures or checks, all of it after the timed region: the oracle verification, the vocabulary
broadcast and BoW check (N > 1), the two-batches-in-flight, popcount-matcher, uploaded-frames and single-frame
legs, the rocprofv3 traffic runs and the CPU baseline.  The --no-* switches turn single legs of --full off.

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment launches its own N ranks (it
re-executes itself under torch.distributed.run on 127.0.0.1 with a free port), so both command shapes work.

Multi-GPU: frames are independent, so every rank runs its own ride on its own GPU (weak
scaling, no data-path collective); the only collectives are the barrier / max-over-ranks timing
and, with --full, one RCCL broadcast of the ORB vocabulary at start-up (outside the timed region).
Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec


def level_sizes(ext, w, h):
    inv = ext.GetInverseScaleFactors()
    import numpy as np
    return [(int(np.rint(np.float32(w) * inv[l])), int(np.rint(np.float32(h) * inv[l])))
            for l in range(ext.nlevels)]


def algorithmic_bytes(sizes, nkp, fused=False):
    """Per-frame algorithmic bytes of each kernel group.  fused: the launch that resizes
    level l -> l + 1 also detects level l (csrc/fused.hip) -- every level is read ONCE, K2 is left with the last level."""
    px = [a * b for a, b in sizes]
    return {
        "pyramid": sum(px[:-1]) + sum(px[1:]),          # reads of levels 0..L-2 + writes of 1..L-1
        "fast": px[-1] if fused else sum(px),           # one detection read of every level (fused: of the last level)
        "quadtree": 0,
        "describe": nkp * (43 * 43 + 60),               # raw window + keypoint/descriptor out
        "match": 2 * nkp * 32 + nkp * 8,
    }


_CPU_WORKER = r"""
import sys, time
sys.path.insert(0, sys.argv[1])
import numpy as np
from oracle import orb_oracle
from pilotguru_amd.synth import synth_ride, synth_ride_road
w, h, nf, warm, reps, rep_s, seed, scene, simd = (int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]),
                                                  int(sys.argv[6]), float(sys.argv[7]), int(sys.argv[8]), sys.argv[9], int(sys.argv[10]))
ride = (synth_ride_road if scene == "road" else synth_ride)(1000 + seed, w, h, 4)
ora = orb_oracle.OrbOracle(nf, 1.2, 8, 20, 7, simd=bool(simd))
if bool(simd) != ora.simd:
    sys.stdout.write("nosimd\n"); sys.stdout.flush(); sys.exit(3)
kp, prev = ora.extract(ride[0])
sys.stdout.write("ready\n"); sys.stdout.flush()
sys.stdin.readline()                                   # start gate
done = 0
def one():
    global prev, done
    kp, desc = ora.extract(ride[(done + 1) % 4])
    orb_oracle.hamming_best2(desc, prev)
    prev = desc; done += 1
for _ in range(warm):
    one()
out = []
for r in range(reps):
    t0 = time.perf_counter(); k = 0
    while time.perf_counter() - t0 < rep_s:
        one(); k += 1
    out.append("%d:%.6f" % (k, time.perf_counter() - t0))
print(" ".join(out))
"""


def _cpu_leg(nproc, w, h, nfeatures, warm, reps, rep_s, scene, lib_path, simd=False):
    """`nproc` oracle workers (one extractor each); per repetition r the rate is the frames all workers
    finished in their r-th window / the longest such window.  Returns the per-repetition rates.
    simd: the workers' extractors run the SIMD variants of what OpenCV 2.4.9 vectorises (oracle/orb_simd.c)."""
    import subprocess
    env = dict(os.environ)
    if lib_path:
        env["PGORB_ORACLE_LIB"] = lib_path
    procs = [subprocess.Popen([sys.executable, "-c", _CPU_WORKER, ROOT, str(w), str(h), str(nfeatures), str(warm), str(reps),
                               str(rep_s), str(i), scene, "1" if simd else "0"],
                              stdin=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True, env=env)
             for i in range(nproc)]
    ready = [p.stdout.readline().strip() for p in procs]   # every worker has generated its frames
    if any(r != "ready" for r in ready):
        for p in procs:
            p.kill()
        raise RuntimeError("CPU worker not ready (%s): no AVX2 on this host?" % ",".join(sorted(set(ready))))
    for p in procs:
        p.stdin.write("go\n"); p.stdin.flush()
    frames = [0] * reps
    tmax = [0.0] * reps
    for p in procs:
        toks = p.stdout.readline().split()
        p.wait()
        for r, tok in enumerate(toks):
            k, t = tok.split(":")
            frames[r] += int(k); tmax[r] = max(tmax[r], float(t))
    return [f / t for f, t in zip(frames, tmax)], sum(frames)


def usable_cores():
    """Host cores this process may actually use: the affinity mask, capped by the cgroup CPU quota (the GPU
    box shows 256 logical CPUs but grants 16 CPUs of time; 256 workers on 16 CPUs only measure the scheduler)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            tok = open(path).read().split()
            if path.endswith("cpu.max"):
                if tok[0] != "max":
                    n = min(n, max(1, int(float(tok[0]) / float(tok[1]) + 0.999)))
            else:
                q = int(tok[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, (q + per - 1) // per))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_baseline(w, h, nfeatures, scene="textured"):
    """The CPU oracle (oracle/: a scalar plain-C port of the reference path; the reference binary itself
    needs OpenCV 2.4 and cannot be built or shipped) timed on this host per BASELINE.md section 2: same
    workload (extract + best-2 match against the previous frame), built -O3 -march=native
    -ffp-contract=off on this box when it has a compiler (generic x86-64 build otherwise), (i) ONE
    thread -- how the reference runs extraction (Frame.cc:254) -- after a 20-frame warm-up, (ii) one
    extractor per host core, frames sharded; median of 5 repetitions each."""
    import statistics
    import subprocess
    cores = usable_cores()
    lib_path, flags = None, "-O3 -ffp-contract=off (generic x86-64, prebuilt)"
    try:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "native"], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        lib_path = os.path.join(ROOT, "oracle", "_native", "liborb_oracle.so")
        flags = "-O3 -march=native -ffp-contract=off (built on this host)"
    except (OSError, subprocess.CalledProcessError):
        pass
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    def both(simd):
        one, n1 = _cpu_leg(1, w, h, nfeatures, 10, 3, 1.5, scene, lib_path, simd)
        allc, na = _cpu_leg(cores, w, h, nfeatures, 3, 3, 2.0, scene, lib_path, simd)
        v1, va = statistics.median(one), statistics.median(allc)
        return {"value": va, "per_core": va / cores, "frames_timed": n1 + na,
                "one_thread": {"value": v1, "ms_per_frame": 1e3 / v1, "cores": 1, "repetitions": one}, "all_cores_repetitions": allc}
    scalar = both(False)
    try:
        simd = both(True)
    except Exception as e:                                   # noqa: BLE001 -- a host without AVX2: the scalar port is the baseline
        simd = None
        simd_err = str(e)[:200]
    best = simd if simd is not None else scalar
    out = {"value": best["value"], "unit": "frames/s", "cores": cores, "logical_cpus_visible": os.cpu_count(), "kind": "port",
           "variant": "port+simd" if simd is not None else "port (scalar)",
           "per_core": best["per_core"], "one_thread": best["one_thread"], "all_cores_repetitions": best["all_cores_repetitions"],
           "scalar_port": scalar, "flags": flags, "cpu_model": model,
           "sample": "%d synthetic %dx%d frames (%s scene), %d features, extract + best-2 match vs previous frame, per variant: 1 thread "
                     "(10-frame warm-up, median of 3 x 1.5 s) and %d worker processes, one oracle extractor per core (3-frame warm-up, "
                     "median of 3 x 2 s).  `value` = the faster variant: the C port with SIMD variants of exactly what OpenCV 2.4.9 vectorises "
                     "(FAST 16 px per vector + cornerScore, resize's vertical pass, both GaussianBlur passes; AVX2 where wider than the "
                     "reference's SSE2; oracle/orb_simd.c, bit-equal to the scalar port: tests/test_oracle.py); `scalar_port` = the plain-C port"
                     % (best["frames_timed"] + (scalar["frames_timed"] if simd is not None else 0), w, h, scene, nfeatures, cores)}
    if simd is not None:
        out["simd_over_scalar"] = {"all_cores": simd["value"] / scalar["value"], "one_thread": simd["one_thread"]["value"] / scalar["one_thread"]["value"]}
    else:
        out["simd_unavailable"] = simd_err
    return out


def verify_against_oracle(ride, kps, desc, n, mout, nfeatures):
    """After the timed region: the first and the last frame of the batch the timed steps processed and
    the last frame's best-2 match against its predecessor, byte for byte against the CPU oracle.  A
    mismatch ends the run without a JSON line."""
    import numpy as np
    from oracle import orb_oracle
    B = ride.shape[0]
    nh = n.cpu().numpy()
    odesc = {}
    for f in sorted({0, B - 2, B - 1}):
        if f < 0:
            continue
        okp, od = orb_oracle.OrbOracle(nfeatures, 1.2, 8, 20, 7).extract(ride[f])
        if f in (0, B - 1):
            if nh[f] != len(okp) or kps[f, :nh[f]].cpu().numpy().tobytes() != okp.tobytes() or \
                    not np.array_equal(desc[f, :nh[f]].cpu().numpy(), od):
                raise SystemExit("bench verification FAILED: frame %d differs from the oracle" % f)
        odesc[f] = od
    if B >= 2:
        obi, ob1, ob2 = orb_oracle.hamming_best2(odesc[B - 1], odesc[B - 2])
        m = nh[B - 1]
        if not (np.array_equal(mout[0][B - 2, :m].cpu().numpy(), obi) and
                np.array_equal(mout[1][B - 2, :m].cpu().numpy().view(np.uint16), ob1) and
                np.array_equal(mout[2][B - 2, :m].cpu().numpy().view(np.uint16), ob2)):
            raise SystemExit("bench verification FAILED: best-2 match of the last pair differs from the oracle")
    return True


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, kps, desc, n, mout, seed=0):
    """--dump-outputs: what the last timed step handed its caller, as out_dir/<name>.npy, so that two builds can be
    compared output for output.  Every buffer keeps the caller's layout (cap = max_keypoints slots per frame); only the
    first n[f] slots of frame f hold results, the rest is never written by the path and is zeroed here.
      keypoints.npy          float64 [F, cap, 7]   x, y, size, angle, response, octave, class_id (by value)
      descriptors.npy        float32 [F, cap, 32]  one descriptor byte per element
      n_keypoints.npy        float64 [F]
      match_best_idx.npy     float64 [P, cap]      best-2 match of frame f against f - 1, one row per pair
      match_best_dist.npy    float32 [P, cap]
      match_second_dist.npy  float32 [P, cap]
      frames.npy             float64 [F]           the batch's frame index of each row above
      match_query_frames.npy float64 [P]           the query frame f of each match row
    All frames when that fits DUMP_LIMIT_BYTES, else a fixed, seeded sample of them (sorted).  Returns a summary."""
    import numpy as np
    from pilotguru_amd.orb import KEYPOINT_DTYPE
    B, cap = int(kps.shape[0]), int(kps.shape[1])
    has_match = B > 1
    per_frame = cap * (7 * 8 + 32 * 4) + 8 * 2 + ((cap * (8 + 4 + 4) + 8) if has_match else 0)
    nsel = max(1, min(B, DUMP_LIMIT_BYTES // per_frame))
    frames = np.arange(B) if nsel == B else np.sort(np.random.default_rng(seed).choice(B, nsel, replace=False))
    nh = n.cpu().numpy().astype(np.int64)
    live = np.arange(cap)[None, :] < nh[frames][:, None]                      # [F, cap]: slots that hold results
    rec = kps.cpu().numpy()[frames].view(KEYPOINT_DTYPE)[..., 0]               # [F, cap] records
    kp = np.stack([rec[f].astype(np.float64) for f in KEYPOINT_DTYPE.names], axis=-1)
    kp[~live] = 0.0
    dsc = desc.cpu().numpy()[frames].astype(np.float32)
    dsc[~live] = 0.0
    out = {"keypoints": kp, "descriptors": dsc, "n_keypoints": nh[frames].astype(np.float64),
           "frames": frames.astype(np.float64)}
    if has_match:
        q = frames[frames >= 1]                                                # pair p = frame p + 1 against frame p
        mlive = np.arange(cap)[None, :] < nh[q][:, None]
        for name, t, dt in (("match_best_idx", mout[0], np.float64), ("match_best_dist", mout[1], np.float32),
                            ("match_second_dist", mout[2], np.float32)):
            a = t[:B - 1].cpu().numpy()[q - 1].astype(dt)
            a[~mlive] = 0.0
            out[name] = a
        out["match_query_frames"] = q.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))
    return {"dir": os.path.abspath(out_dir), "bytes": int(sum(a.nbytes for a in out.values())), "frames": int(nsel),
            "of_frames": B, "arrays": sorted(out)}


def upload_leg(pg, ext, ride, NF, W, H, B, seconds=2.0, depth=3, frontend=False, link=True, channels=1):
    """The same step (extract + best-2 match of every frame against its predecessor) with frames that start in
    page-locked HOST memory: pgorb_stream_* with `depth` batches in flight (upload, kernels and result download on
    three HIP streams).  Reported next to the resident number, never as `value`.  Also measures what the link
    itself gives: one large pinned hipMemcpyAsync H2D."""
    import numpy as np
    import torch
    # channels = 3: the slots hold RGB24 frames, what the reference's reader decodes (image_sequence_reader.cc:138-208);
    # Tracking's cvtColor (Tracking.cc:247-260) then runs on the device in front of the pyramid (k_ingest_rows)
    st = pg.FrameStream(ext, W, H, B, depth, channels=channels)
    if frontend:
        # + what the tracking thread does with every fresh Frame, on the device per batch: 64x48 grid,
        # SearchForInitialization(previous, current) (Tracking.cc:583-597), ORBVocabulary::transform (Frame.cc:399-406)
        from pilotguru_amd import vocab as V
        V.ORBVocabulary(blob=V.synth_vocabulary_blob(10, 5, seed=7)).upload(ext)
        st.frontend((0.0, float(W), 0.0, float(H)), 100, 0.9, True, 4)
    for sl in range(depth):
        if channels == 1:
            st.input(sl)[:] = ride                          # "the decoder" has filled every slot
        else:
            for ch in range(channels):
                st.input(sl)[..., ch] = ride
    # warm-up: fill the pipeline once
    for sl in range(depth):
        st.submit(sl)
    for sl in range(depth):
        st.wait(sl)
    t0 = time.perf_counter(); done = 0; sub = 0
    inflight = []
    while True:
        now = time.perf_counter()
        if now - t0 < seconds or not done:
            if len(inflight) == depth:
                st.wait(inflight.pop(0)); done += 1
            sl = sub % depth
            st.submit(sl); inflight.append(sl); sub += 1
        else:
            break
    for sl in inflight:
        st.wait(sl); done += 1
    t1 = time.perf_counter()
    st.close()
    fps = done * B / (t1 - t0)
    if channels != 1:
        return {"value": fps, "unit": "frames/s", "batches": done, "seconds": t1 - t0, "depth": depth, "channels": channels,
                "h2d_GBps_used": fps * W * H * channels / 1e9,
                "note": "as frames_uploaded with RGB24 frames in the page-locked slots (%d bytes per pixel over the link); grey "
                        "conversion on the device" % channels}
    if not link:
        return {"value": fps, "unit": "frames/s", "batches": done, "seconds": t1 - t0, "depth": depth,
                "note": "as frames_uploaded, plus the stream's front-end stage per batch: grid, SearchForInitialization of every "
                        "frame against its predecessor (window 100, ratio 0.9), BoW transform on a k=10 L=5 tree"}
    # the link: one pinned H2D copy of a batch, repeated
    host = torch.empty((B, H, W), dtype=torch.uint8).pin_memory()
    devt = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    devt.copy_(host, non_blocking=True); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(8):
        devt.copy_(host, non_blocking=True)
    e1.record(); torch.cuda.synchronize()
    h2d_gbs = 8 * B * H * W / (e0.elapsed_time(e1) * 1e-3) / 1e9
    link_fps = h2d_gbs * 1e9 / (W * H)
    return {"value": fps, "unit": "frames/s", "batches": done, "seconds": t1 - t0, "depth": depth,
            "h2d_GBps_used": fps * W * H / 1e9, "h2d_GBps_link": h2d_gbs, "link_bound_fps": link_fps,
            "fraction_of_link": fps / link_fps,
            "note": "frames start in page-locked host memory; upload + kernels + download of results overlapped on "
                    "three HIP streams (pgorb_stream_*); PCIe-inclusive, not the headline value"}


def live_pmc(args, kname):
    """HBM traffic (and VALU instructions) of kernel `kname`, measured by THIS run: three short child runs of this very
    command under `rocprofv3 --kernel-trace --pmc <one counter group>` (separate passes, as MI355X_MICROARCH.md's HBM
    section prescribes: FETCH_SIZE and WRITE_SIZE do not fit one pass), 1 warm-up + 3 steps each, every other leg off.
    Returns {"fetch_kb", "write_kb", "sq_insts_valu", "seconds"} per launch, or None when rocprofv3 is not usable here
    (the caller then cites the newest committed profile and says so)."""
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None
    t0 = time.perf_counter()
    base = tempfile.mkdtemp(prefix="pgorb_pmc_")
    child = [sys.executable, os.path.abspath(__file__), "--steps", "3", "--warmup", "1", "--batch", str(args.batch),
             "--width", str(args.width), "--height", str(args.height), "--features", str(args.features), "--scene", args.scene,
             "--sustain-seconds", "0"] + (["--fused-levels", str(args.fused_levels)] if args.fused_levels is not None else [])
    env = dict(os.environ, TMPDIR="/tmp", PGORB_BENCH_CHILD="1")
    out = {}
    try:
        for tag, group in (("fetch_kb", ["FETCH_SIZE"]), ("write_kb", ["WRITE_SIZE"]), ("sq_insts_valu", ["SQ_INSTS_VALU", "SQ_INSTS_SALU"])):
            d = os.path.join(base, tag)
            r = subprocess.run([exe, "--kernel-trace", "--pmc"] + group + ["-d", d, "--"] + child, env=env, cwd="/tmp",
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=90)
            dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith(".db")]
            if r.returncode != 0 or not dbs:
                return None
            con = sqlite3.connect(dbs[0])
            for counter in group:
                row = con.execute("select avg(value), count(*) from counters_collection where counter_name = ? and kernel_name like ?",
                                  (counter, "%" + kname + "%")).fetchone()
                if not row or row[0] is None:
                    return None
                out[tag if counter == group[0] else counter.lower()] = float(row[0])
            con.close()
    except (OSError, subprocess.SubprocessError, sqlite3.Error):
        return None
    finally:
        shutil.rmtree(base, ignore_errors=True)
    out["seconds"] = time.perf_counter() - t0
    return out


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-execute under torch.distributed.run, one rank per GPU
    (rank r -> device r), rendezvous on 127.0.0.1.  The children's stdout is ours, so rank 0's JSON line is the
    last line this process prints; the exit code is the launcher's."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC only on this host driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        sys.stderr.write("bench.py: self-launched %d-rank job failed with exit code %d\n" % (n, rc))
    raise SystemExit(rc)


def timed_steps(step, steps, dist, dev, sync):
    """The contract's timed region: barrier + device sync on both sides of exactly `steps` steps.  Every rank reads its
    clock after its own device sync and BEFORE the closing barrier: the figure `value` is built on is the MAXIMUM over the
    ranks of that interval -- the time of the slowest rank's K steps, which is what the job waits for -- and does not
    contain the closing barrier's own latency (an RCCL barrier is 0.3-1 ms against a 28-ms window: 1-4 % of a scaling
    efficiency that would not be kernel time).  The barrier-inclusive interval is reported beside it.
    Returns (max-over-ranks seconds, [every rank's own seconds], max-over-ranks barrier-inclusive seconds)."""
    if dist is not None:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    t_own = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
    t_incl = time.perf_counter() - t0
    if dist is None:
        return t_own, [t_own], t_incl
    import torch
    from pilotguru_amd import dist as pgd
    mine = torch.tensor([t_own], dtype=torch.float64, device=dev)
    allt = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(allt, mine)
    per_rank = [float(t.item()) for t in allt]
    return max(per_rank), per_rank, pgd.max_over_ranks(t_incl, dev)


def scaling_fields(world, frames_per_rank, elapsed, per_rank_s, n1_fps):
    """Per-rank rates and, when the caller supplies the N = 1 figure (--n1-fps), the efficiency that follows
    from them.  (The driver computes its own efficiency from the per-N `value`s; this is a convenience.)"""
    out = {"per_rank_fps": [frames_per_rank / t for t in per_rank_s], "max_rank_seconds": elapsed}
    if n1_fps:
        out["n1_fps"] = n1_fps
        out["scaling_efficiency"] = (world * frames_per_rank / elapsed) / (world * n1_fps)
    return out


def launcher_test_rank(args):
    """PGORB_BENCH_LAUNCHER_TEST=1: the rank plumbing alone on a box WITHOUT a GPU (tests/test_bench_launcher.py) --
    gloo instead of RCCL, the vocabulary broadcast on CPU tensors, the step replaced by a fixed sleep.  The line it
    prints is labelled as such and is not a measurement."""
    import torch
    import torch.distributed as dist
    from pilotguru_amd import dist as pgd
    from pilotguru_amd.vocab import synth_vocabulary_blob
    rank, _, world = pgd.env_world()
    dist.init_process_group("gloo")
    dev = torch.device("cpu")
    blob = synth_vocabulary_blob(k=4, L=3, seed=7) if rank == 0 else None
    tb0 = time.perf_counter()
    vocab = pgd.broadcast_vocabulary(blob, 0, dev)
    tb = time.perf_counter() - tb0
    sig = torch.tensor([int(vocab.to(torch.int64).sum())])
    sigs = [torch.empty_like(sig) for _ in range(world)]
    dist.all_gather(sigs, sig)
    assert all(torch.equal(sigs[0], x) for x in sigs)
    elapsed, per_rank, elapsed_incl = timed_steps(lambda: time.sleep(0.002 * (1 + rank)), args.steps, dist, dev, lambda: None)
    if rank == 0:
        out = {"metric": "LAUNCHER TEST (no GPU work)", "value": world * args.batch * args.steps / elapsed, "unit": "frames/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
               "launcher_test": True, "rides": [pgd.ride_for_rank(r, world) for r in range(world)],
               "config": {"vocab_broadcast_bytes": int(vocab.numel()), "vocab_broadcast_s": tb}}
        out.update(scaling_fields(world, args.batch * args.steps, elapsed, per_rank, args.n1_fps))
        line = json.dumps(out)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--scene", choices=("textured", "road"), default="textured",
                    help="textured = SURVEY.md 8d's scene (the headline workload); road = sky / asphalt / texture band")
    ap.add_argument("--no-overlap-leg", action="store_true", help="skip the two-batches-in-flight leg (second context)")
    ap.add_argument("--sustain-seconds", type=float, default=3.0,
                    help="BEFORE the warm-up and timed steps, step for this long and report sustained_fps (0 = skip): the GPU is in its working state when the timed region starts")
    ap.add_argument("--pipeline-pyramid", type=int, default=None,
                    help="1 / 0: run the pyramid chain beside K2 on a side stream (library default when omitted)")
    ap.add_argument("--fused-levels", type=int, default=None,
                    help="1 / 0: resize level l -> l + 1 and detect level l in one launch (csrc/fused.hip; library default when omitted)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--no-upload-leg", action="store_true")
    ap.add_argument("--no-single-frame-leg", action="store_true",
                    help="skip the one-frame-per-synchronous-call leg (the reference's call shape, tools/single_frame_bench.py)")
    ap.add_argument("--no-traffic-leg", action="store_true",
                    help="do not re-measure roofline.traffic with rocprofv3 PMC child runs after the timed region (cite the newest committed profile instead)")
    ap.add_argument("--n1-fps", type=float, default=None,
                    help="the N = 1 frames/s of the same configuration; adds scaling_efficiency to the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (rank 0's keypoints, descriptors, "
                         "counts and best-2 matches) as DIR/<name>.npy in float32 / float64, at most 64 MB (a fixed, seeded "
                         "sample of the frames when the batch is larger)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every leg beyond the headline figure: oracle verification, vocabulary "
                         "broadcast + BoW check (N > 1), two batches in flight, popcount matcher, uploaded frames, single frame, "
                         "rocprofv3 traffic runs, CPU baseline (each --no-* switch turns one of them off)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:                                           # a plain run: nothing the headline figure does not need
        args.no_cpu_baseline = args.no_verify = args.no_upload_leg = args.no_overlap_leg = True
        args.no_single_frame_leg = args.no_traffic_leg = True

    if (args.gpus > 1 or os.environ.get("PGORB_BENCH_FORCE_LAUNCH")) and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)                                  # does not return
    if os.environ.get("PGORB_BENCH_LAUNCHER_TEST"):
        if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
            raise SystemExit("--gpus %d but WORLD_SIZE=%s" % (args.gpus, os.environ.get("WORLD_SIZE")))
        return launcher_test_rank(args)

    import numpy as np
    import torch
    import pilotguru_amd as pg
    from pilotguru_amd.synth import synth_ride, synth_ride_road

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if local_rank >= torch.cuda.device_count():
        raise SystemExit("rank %d: local rank %d but only %d GPU(s) visible" % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or os.environ.get("PGORB_BENCH_FORCE_DIST"):    # the env switch exercises the N>1 code on one GPU
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)      # "nccl" is RCCL on ROCm

    W, H, B, NF = args.width, args.height, args.batch, args.features
    ext = pg.ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B, device=local_rank)

    if args.pipeline_pyramid is not None:
        ext.set_option("pipeline_pyramid", args.pipeline_pyramid)
    if args.fused_levels is not None:
        ext.set_option("fused_levels", args.fused_levels)
    # one ride per rank (ride id = rank): B consecutive frames, resident in HBM
    from pilotguru_amd import dist as pgd0
    make_ride = synth_ride_road if args.scene == "road" else synth_ride
    ride = make_ride(pgd0.ride_for_rank(rank, world)[0], W, H, B)
    frames = torch.from_numpy(ride).to(dev)
    cap = ext.max_keypoints(W, H)
    kps = torch.empty((B, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.empty((B, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.empty((B,), dtype=torch.int32, device=dev)
    pq = torch.arange(1, B, dtype=torch.int32, device=dev)      # frame f (query) vs f-1 (train)
    pt = torch.arange(0, B - 1, dtype=torch.int32, device=dev)
    mout = (torch.empty((max(B - 1, 1), cap), dtype=torch.int32, device=dev),
            torch.empty((max(B - 1, 1), cap), dtype=torch.int16, device=dev),
            torch.empty((max(B - 1, 1), cap), dtype=torch.int16, device=dev))

    # the one collective of this path: the ORB vocabulary, parsed ONCE by rank 0 from its text file, broadcast root -> peers
    # through the C ABI (pgorb_comm_create_rank + pgorb_vocab_broadcast: librccl's ncclBroadcast straight into every context's
    # vocabulary arena; torch.distributed only hands the 128-byte RCCL id round).  Reference: one ORBVocabulary shared by
    # pointer, src/optical_trajectories.cc:87-94.
    vocab_bytes, vocab_bcast_s, voc, voc_path, voc_comm = 0, None, None, None, None
    vocab_path_used, rccl_info = None, None
    if dist is not None and args.full:
        from pilotguru_amd import dist as pgd
        from pilotguru_amd import vocab as V
        if rank == 0:
            # the size of the real ORBvoc.txt (k = 10, L = 6: 1 111 111 nodes, 146 MB of text, 66.7 MB as a blob); the file
            # itself needs network access (fetch-vocabulary.sh:5)
            import tempfile
            voc_path = os.path.join(tempfile.mkdtemp(prefix="pgorb_voc_"), "orbvoc_like.txt")
            V.write_vocabulary_text_fast(voc_path, 10, 6, *V.synth_vocabulary_fast(10, 6, seed=7))
            voc = V.ORBVocabulary(text_file=voc_path)
            vocab_bytes = int(voc.blob().nbytes)
        # The C-ABI group has only ever run as ONE rank on the boxes this was written on.  If it cannot be formed on some rank
        # (librccl not loadable from the library, a unique-id mismatch ...) every rank learns it from one all_reduce and all of
        # them take the round-2..4 path instead -- torch.distributed's own RCCL broadcast of the blob + pgorb_vocab_upload_device --
        # so that a multi-GPU run still produces its line; `vocab_broadcast` in the line says which path ran.
        vocab_path_used = "pgorb_vocab_broadcast (C ABI, librccl ncclBroadcast; text parsed once on rank 0)"
        ok = 1
        try:
            voc_comm = pgd.VocabularyComm.from_torch_group(ext)
        except Exception as e:                                    # noqa: BLE001 -- any failure takes the fallback, on every rank
            sys.stderr.write("rank %d: pgorb_comm_create_rank failed (%s); falling back to torch.distributed's broadcast\n" % (rank, e))
            ok, voc_comm = 0, None
        flag = torch.tensor([ok], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        # which librccl the library resolved, and how many the process maps (one process must never run two RCCLs: the id of
        # one would be handed to the other)
        lib_path, lib_pre = pgd.VocabularyComm.library()
        with open("/proc/self/maps") as mf:
            mapped = sorted({ln.split()[-1] for ln in mf if "librccl.so" in ln.rsplit("/", 1)[-1]})
        rccl_info = {"path": lib_path, "held_by_process_before": lib_pre, "mapped": mapped}
        if int(flag.item()) == 1:
            vocab_bcast_s = voc_comm.broadcast(voc, 0)
        else:
            if voc_comm is not None:
                voc_comm.close(); voc_comm = None
            import ctypes as C
            blob_t = torch.from_numpy(np.ascontiguousarray(voc.blob()).copy()) if rank == 0 else None
            torch.cuda.synchronize(); tb0 = time.perf_counter()
            vt = pgd.broadcast_vocabulary(blob_t, 0, dev)
            torch.cuda.synchronize(); vocab_bcast_s = time.perf_counter() - tb0
            vocab_bytes = int(vt.numel())
            ext._check(ext._L.pgorb_vocab_upload_device(ext._h, C.c_void_p(vt.data_ptr()), vt.numel(),
                                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            torch.cuda.synchronize()
            vocab_path_used = "torch.distributed broadcast (RCCL) + pgorb_vocab_upload_device: the C-ABI group could not be formed"

    def step():
        ext.extract_batch_device(frames, kps, desc, n)
        if B > 1:
            ext.match_batch_device(desc, n, pq, pt, mout)

    # The sustained leg runs FIRST (round 5): the same step for >= --sustain-seconds, every rank.  It is a measurement of its own
    # (`sustained_fps`, N = 1) -- and it is what brings the GPU to the state it works in: after the seconds of host-side set-up
    # above the clocks are down, and the first ~30 steps of a cold start run 1.60 ... 1.38 ms (tools/experiments/r3_ramp.py), so the
    # driver's 5 + 20 steps used to be timed on a clock ramp (`value` sat 5-7 % under `sustained_fps`).  The contract's W warm-up
    # steps and K timed steps follow unchanged.
    sustained = None
    if args.sustain_seconds > 0:
        step(); torch.cuda.synchronize()
        t1 = time.perf_counter(); step(); torch.cuda.synchronize()
        k_chunk = max(10, int(0.25 / max(time.perf_counter() - t1, 1e-6)))
        ts = time.perf_counter(); ksteps = 0
        while time.perf_counter() - ts < args.sustain_seconds:
            for _ in range(k_chunk):
                step()
            torch.cuda.synchronize()
            ksteps += k_chunk
        te = time.perf_counter()
        ext.check_async()
        sustained = {"fps": ksteps * B / (te - ts), "seconds": te - ts, "steps": ksteps,
                     "note": "this rank's own rate; runs before the warm-up and timed steps"}

    for _ in range(args.warmup):
        step()
    ext.check_async()
    torch.cuda.synchronize()
    counts = n.cpu().numpy()

    ext.profile_begin(args.steps)
    elapsed, per_rank_s, elapsed_incl = timed_steps(step, args.steps, dist, dev, torch.cuda.synchronize)
    ncalls, stage_ms = ext.profile_read()
    ext.check_async()

    # ---- everything below is outside the timed region ------------------------------------------
    # (first: the legs below reuse kps / desc / n / mout, so the last timed step's results are saved before them)
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, kps, desc, n, mout)
    verified = None
    if not args.no_verify and rank == 0:
        verified = verify_against_oracle(ride, kps, desc, n, mout, NF)

    # config 4's criterion: every rank's BoW words -- of ITS OWN ride's first frame, through the
    # vocabulary that reached it by the broadcast -- equal the CPU oracle's on rank 0 (words, weights and nodes themselves)
    bow_verified = None
    if dist is not None and args.full:
        import ctypes as C
        n0 = int(n[0].item())
        pw = torch.empty(n0, dtype=torch.int32, device=dev)
        pwt = torch.empty(n0, dtype=torch.float64, device=dev)
        pn = torch.empty(n0, dtype=torch.int32, device=dev)
        d0 = desc[0, :n0].contiguous()
        ext._check(ext._L.pgorb_bow_transform_device(
            ext._h, C.c_void_p(d0.data_ptr()), n0, 4, C.c_void_p(pw.data_ptr()), C.c_void_p(pwt.data_ptr()),
            C.c_void_p(pn.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        torch.cuda.synchronize()
        mine = (d0.cpu().numpy(), pw.cpu().numpy(), pwt.cpu().numpy(), pn.cpu().numpy())
        parts = [None] * world
        dist.all_gather_object(parts, mine)
        if rank == 0 and not args.no_verify:
            from oracle import orb_oracle
            ora_voc = orb_oracle.VocabOracle(voc_path)
            for r, (dr, wr, wtr, nr) in enumerate(parts):
                ow, owt, on = ora_voc.transform_features(dr, 4)
                if not (np.array_equal(wr.view(np.uint32), ow) and wtr.tobytes() == owt.tobytes() and np.array_equal(nr.view(np.uint32), on)):
                    raise SystemExit("bench verification FAILED: rank %d's BoW words differ from the oracle after the vocabulary broadcast" % r)
            bow_verified = True
        if voc_comm is not None:
            voc_comm.close()

    # two batches in flight INSIDE the library (round 5: pgorb_stream_create_device, one context, two lanes): the caller submits
    # resident batches without blocking, the stream runs consecutive batches on two sibling working sets and HIP streams, so
    # that kernels with different bottlenecks (K1 HBM, K2 / K4-6 VALU issue, K3 latency, K7 matrix pipe) of neighbouring
    # batches share the chip; the match of a batch's first frame against the previous batch's last is chained in submission
    # order.  Same work per batch plus that one extra pair; reported next to `value`, not as it (the kernels' own durations
    # stretch when they share the GPU, so `roofline` and the stage times stay those of the one-batch-at-a-time loop above).
    inflight2 = None
    leg_errors = {}                                              # a LEG that fails is reported in the line; it never takes the line with it
    def _inflight_leg():
        st2 = pg.DeviceFrameStream(ext, W, H, B, depth=2, lanes=2)
        torch.cuda.synchronize()
        for k in range(4):
            if k >= 2:
                st2.wait(k & 1, on_host=False)
            st2.submit(k & 1, frames)
        r0, r1 = st2.wait(0), st2.wait(1)
        torch.cuda.synchronize()
        ts = time.perf_counter(); ksteps = 0
        st2.submit(0, frames); st2.submit(1, frames)
        while time.perf_counter() - ts < 1.5:
            for k in range(40):
                st2.wait(k & 1, on_host=False)              # (orders the slot's reuse on the caller's stream; the host does not block)
                st2.submit(k & 1, frames)
            st2.wait(0); st2.submit(0, frames)                # the host joins the queue once per 40 batches
            ksteps += 41
        r0, r1 = st2.wait(0), st2.wait(1)
        torch.cuda.synchronize()
        te = time.perf_counter()
        ksteps += 2
        ext.check_async()
        nh2 = n.cpu().tolist()
        same = all(torch.equal(r[0], n) and all(torch.equal(desc[f, :nh2[f]], r[2][f, :nh2[f]]) and
                                                 torch.equal(kps[f, :nh2[f]].view(torch.int32), r[1][f, :nh2[f]].view(torch.int32)) and
                                                 (f == 0 or torch.equal(mout[0][f - 1, :nh2[f]], r[3][f, :nh2[f]])) for f in range(B))
                   for r in (r0, r1))
        res = {"fps": ksteps * B / (te - ts), "seconds": te - ts, "steps": ksteps, "contexts": 1, "lanes": 2,
                     "every_frame_of_both_in_flight_batches_equals_the_one_batch_loop": bool(same),
                     "note": "pgorb_stream_create_device / _submit_device: resident batches submitted without blocking, two lanes (sibling "
                             "working sets on two internal HIP streams) inside ONE context; matches chained across batches"}
        st2.close()
        return res
    if not args.no_overlap_leg and dist is None and B > 1:
        try:
            inflight2 = _inflight_leg()
        except Exception as e:                                   # noqa: BLE001
            leg_errors["two_batches_in_flight"] = str(e)[:300]

    # the matcher the north star describes (ballot / popcount), timed on the same descriptors
    matcher = ext.matcher_name(cap)
    popcount_ms = None
    if args.full and dist is None and B > 1:
        try:
            ext.set_option("matcher", 1)
            for _ in range(2):
                ext.match_batch_device(desc, n, pq, pt, mout)
            torch.cuda.synchronize()
            tp = time.perf_counter()
            for _ in range(5):
                ext.match_batch_device(desc, n, pq, pt, mout)
            torch.cuda.synchronize()
            popcount_ms = (time.perf_counter() - tp) / 5 * 1e3
        except Exception as e:                                   # noqa: BLE001
            leg_errors["matcher_popcount"] = str(e)[:300]
        finally:
            ext.set_option("matcher", 0)

    # frames that start in HOST memory: the streamed path (pinned double buffers, copies overlapped with
    # the kernels of the neighbouring batches) -- PCIe-inclusive, reported next to `value`, never as it
    uploaded = None
    if not args.no_upload_leg and dist is None:
        try:
            uploaded = upload_leg(pg, ext, ride, NF, W, H, B, seconds=2.0)
            uploaded["with_front_end_stage"] = upload_leg(pg, ext, ride, NF, W, H, B, seconds=1.5, frontend=True, link=False)
            rgb = upload_leg(pg, ext, ride, NF, W, H, B, seconds=1.5, link=False, channels=3)
            rgb["link_bound_fps"] = uploaded["link_bound_fps"] / 3.0
            rgb["fraction_of_link"] = rgb["value"] / rgb["link_bound_fps"]
            uploaded["rgb24"] = rgb
        except Exception as e:                                   # noqa: BLE001
            leg_errors["frames_uploaded"] = str(e)[:300]

    if rank == 0:
        frames_total = world * B * args.steps
        fps = frames_total / elapsed
        sizes = level_sizes(ext, W, H)
        nkp = float(counts.mean())
        fused = ext.get_option("fused_levels") == 1
        abytes = algorithmic_bytes(sizes, nkp, fused)
        dom = max(("pyramid", "fast", "quadtree", "describe", "match"), key=lambda s: stage_ms[s])
        # the roofline object describes the dominant HBM-streaming kernel; the quadtree moves
        # no image bytes, so when it dominates wall time the image kernel with most time is used
        cands = [s for s in ("pyramid", "fast", "describe", "match")]
        rk = max(cands, key=lambda s: stage_ms[s])
        launches = 7 if rk == "pyramid" else 1
        ach = (abytes[rk] * B / launches) / (stage_ms[rk] / launches * 1e-3) / 1e9
        kname = {"pyramid": "k_pyr_fast" if fused else "k_pyr_resize_rows4_lds", "fast": ext.fast_kernel_name(), "describe": "k_describe",
                 "match": "k_match_mfma"}[rk]
        # HBM bytes / VALU instructions per launch of that kernel: measured by this run (three rocprofv3 PMC child runs of this
        # command, after the timed region) -- or, when rocprofv3 cannot run here, cited from the newest committed profile
        traffic, traffic_src, valu_insts, valu_src, traffic_live = None, None, None, None, False
        if not args.no_traffic_leg and world == 1 and not os.environ.get("PGORB_BENCH_CHILD"):
            live = live_pmc(args, kname)
            if live is not None:
                traffic = (2.0 * live["fetch_kb"] + live["write_kb"]) * 1024.0
                valu_insts = live.get("sq_insts_valu")
                traffic_live = True
                traffic_src = ("measured by this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE child runs of this command "
                               "(1 + 3 steps each, %.0f s), bytes = (2 x FETCH_SIZE + WRITE_SIZE) KB per launch (gfx950 FETCH_SIZE correction)"
                               % live["seconds"])
                valu_src = "SQ_INSTS_VALU of a third child run, per launch"
        if traffic is None:
            try:
                import glob
                for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json")), reverse=True):   # newest round first
                    tr = json.load(open(path))
                    if tr["workload"] == {"width": W, "height": H, "features": NF, "batch": B} and kname in tr["kernels"] \
                            and tr.get("scene", "textured") == args.scene:
                        k = tr["kernels"][kname]
                        traffic = (2.0 * k["fetch_kb"] + k["write_kb"]) * 1024.0
                        traffic_src = "CITED, not measured by this run: profiles/" + os.path.basename(path) + " (rocprofv3 PMC passes of this command on an earlier run)"
                        valu_insts = k.get("sq_insts_valu")
                        valu_src = "profiles/" + os.path.basename(path) + " (SQ_INSTS_VALU of an earlier profiled run, per launch)"
                        break
            except (OSError, KeyError, ValueError):
                pass
        out = {
            "metric": "frames/sec ORB extract+match, 1080p @ 2000 kp/frame",
            "value": fps, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8", "data": "synthetic",
            "config": {"workload": "%dx%d grayscale, %d kp/frame, 8-level pyramid, batch %d frames/GPU "
                                   "resident in HBM, extract + best-2 Hamming match vs previous frame"
                                   % (W, H, NF, B),
                       "scene": args.scene, "width": W, "height": H, "features": NF,
                       "fused_levels": fused,
                       "batch": B, "keypoints_per_frame": nkp, "parallelism": "frames-sharded x%d" % world,
                       "vocab_broadcast_bytes": vocab_bytes, "vocab_broadcast_s": vocab_bcast_s,
                       "vocab_broadcast": vocab_path_used,
                       "vocab_broadcast_librccl": rccl_info,
                       "bow_words_equal_oracle_on_every_rank": bow_verified,
                       "matcher": matcher, "matcher_popcount_ms_per_step": popcount_ms},
            "roofline": {"bound": "hbm", "kernel": kname,
                         "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": ach / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_measured_by_this_run": traffic_live, "traffic_source": traffic_src,
                         "traffic_over_algorithmic": (traffic / (abytes[rk] * B / launches)) if traffic else None,
                         "algorithmic_bytes_per_launch": abytes[rk] * B / launches,
                         "launch_ms": stage_ms[rk] / launches},
            # the resource that actually binds this path: wave-level VALU instructions of the same kernel
            # against what the chip's 1024 SIMDs can issue at the guide's 2 cycles per wave64 instruction
            "roofline_valu": None if not valu_insts else {
                "kernel": kname, "insts": valu_insts, "insts_source": valu_src,
                "cycles_per_inst_peak": 2, "simds": 1024, "clock_ghz": 2.4,
                "min_ms_at_peak": valu_insts * 2 / 1024 / 2.4e9 * 1e3, "launch_ms": stage_ms[rk] / launches,
                "frac": (valu_insts * 2 / 1024 / 2.4e9 * 1e3) / (stage_ms[rk] / launches)},
            "stage_ms_per_step": stage_ms, "dominant_stage": dom,
            "whole_path_algorithmic_GBps": sum(abytes.values()) * fps / world / 1e9,
            "verified": verified,
        }
        out.update(scaling_fields(world, B * args.steps, elapsed, per_rank_s, args.n1_fps))
        # `value` is built on the slowest rank's own K steps (clock read after its device sync); the same interval with the
        # closing barrier inside, for the record
        out["barrier_inclusive_seconds"] = elapsed_incl
        if sustained is not None:
            out["sustained_fps"] = sustained["fps"]
            out["sustained"] = sustained
        if inflight2 is not None:
            out["two_batches_in_flight"] = inflight2
        if uploaded is not None:
            out["frames_uploaded"] = uploaded
        if not args.no_single_frame_leg and world == 1:
            # the reference's call shape (Frame.cc:251-257): ONE frame per synchronous call from pageable host memory; outside
            # the timed region like frames_uploaded, never `value`
            try:
                sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
                import single_frame_bench
                out["single_frame"] = single_frame_bench.run(W, H, NF, calls=2000)
            except Exception as e:                             # (a leg, not the measurement: report and go on)
                out["single_frame"] = {"error": str(e)[:200]}
        if not args.no_cpu_baseline and world == 1:            # rank 0 at N=1 only
            try:
                out["cpu_baseline"] = cpu_baseline(W, H, NF, args.scene)
                out["speedup_vs_cpu_all_cores"] = fps / out["cpu_baseline"]["value"]
                out["speedup_vs_cpu_one_thread"] = fps / out["cpu_baseline"]["one_thread"]["value"]
            except Exception as e:                               # noqa: BLE001 -- the CPU leg must not take the GPU line with it
                leg_errors["cpu_baseline"] = str(e)[:300]
        if dumped is not None:
            out["dumped_outputs"] = dumped
        if leg_errors:
            out["leg_errors"] = leg_errors
        line = json.dumps(out)
    else:
        line = None
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if line is not None:
        # RCCL prints its version banner through C stdio, which a pipe only sees at exit: flush it
        # first so that the JSON line is the LAST line of stdout
        import ctypes
        try:
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        sys.stdout.flush()
        print(line, flush=True)


if __name__ == "__main__":
    main()
