#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X Groth16 prover hot path (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W [--full]

A plain run does what the headline figure needs and nothing else: it builds the benchmark input and its base set, runs W warm-up
and K timed steps, writes the result of the last step (--dump-outputs) and prints ONE JSON line (rank 0):

  * `value` -- G1 MSM points/sec at 2^20 (MNT4753, configs[1]).  One process per GPU; a step is ONE multi-scalar
    multiplication over 2^20 (base, scalar) pairs, bases (with their window table) and scalars resident in HBM.  N > 1 is
    the north-star split: the ONE 2^20 array is cut into N contiguous slices (multiexp.tcc:417-431), rank g runs the whole
    Pippenger on slice g, and the only exchange the path has follows -- an all_gather (RCCL over xGMI) of one 288-byte
    projective point per rank and the serial fold of the N partial sums (multiexp.tcc:433-438).  Total work is fixed
    ("strong").  Beside it, what the timed steps themselves report: `phases_ms`, `precompute_ms` (the base set's window
    table, built before timing) and `roofline` of the bucket accumulation (its HBM traffic quoted from profiles/ while the
    kernel sources are the ones it was measured on).

--full adds every other measurement and check to the same line (each --no-* option leaves one leg of it out):

  * `parity_ok` -- the timed result checked through the discrete logs of the synthetic bases (and every other result below
    against its own known answer); a failure makes the run exit non-zero.  N > 1: `weak`, 2^20 points PER GPU.
  * `prove` -- Groth16 prove time in seconds, MNT4753, full-size parameters (configs[3]): `main_hip MNT4753 compute` (the
    C++ host over the C ABI) on the seeded synthetic files of tools/synth_files.py, timed by the prover itself with the
    reference's window ("Total time from input to output", libsnark/main.cpp:203-270) and by this script around the
    process; the sha256 of the proof is compared with the one the REFERENCE wrote for the same files
    (tests/golden/oracle_hashes.json, minted in the build container by tools/mint_oracle_hashes.py).  N = 1 only.
  * `prove_mnt6753` -- the same for configs[4]'s curve and size (MNT6753, d = 2^15 - 1), and `cpu_prove`: the reference's own
    `./main` (oracle/_ref/main, compiled from /root/reference by oracle/build_ref.sh) timed on this box's host cores on the same
    files: MNT6753 2^15 and MNT4753 at the metric's own size, 2^20 (minutes of CPU time on the box's host threads;
    BENCH_CPU_PROVE_FULL=0 falls back to the 2^17 files, BENCH_CPU_PROVE=0 skips the CPU provers).
  * `exchange_us` -- the one exchange the sharded path has (multiexp.tcc:433-438: one projective point per rank, then the serial fold)
    over RCCL: mean latency of 100 all_gathers of a G1 point through parallel.PointExchange (host -> device -> all_gather -> host).
    N = 1: a world-size-1 RCCL communicator in a child process; N > 1: the communicator of the run itself.
  * `cpu_baseline` -- the reference's multi_exp on the benchmark input, its result compared with the timed one (N = 1), and
    `roofline.traffic` measured by two rocprofv3 --pmc passes of their own (child processes, N = 1).

Secondary figures on the same line (N = 1, --full): 2^20 FFT and compute_H (configs[2]) as `roofline_fft`, the G2 MSM at 2^20,
the G1 MSM without the window table, the slice sizes of an N-way split and the prove times predicted from them (`extras`).

PyTorch is plumbing here (device memory for the scalars, streams/events, torch.distributed); every kernel is in
libmnt753_hip.so, reached through the C ABI.  oracle/ is used only for the cpu_baseline leg.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

LOG_N = 20
ALGO_BYTES_PER_PAIR = 288          # 192 B affine G1 base + 96 B scalar, read once
HBM_PEAK_GBPS = 8000.0             # MI355X_MICROARCH.md: 8 TB/s HBM3E
MODMUL_PEAK_PER_S = 22.0e9         # MEASURED chip peak of the 753-bit Montgomery multiplier, VALU saturated, at the 1.96 GHz the chip sustains under it (profiles/r01/mulbench_mi355x.txt)
# first principles beside it: 1024 SIMDs x 16 lanes per cycle (v_mad_u64_u32 is a full-rate instruction: 4 cycles per wave) x 2.4 GHz
# nominal / 1458 multiply-adds per product -- a clock the chip does not hold under this load (power_and_clocks.txt: 2.07-2.10 GHz)
MODMUL_PEAK_FIRST_PRINCIPLES_PER_S = 1024 * 16 * 2.4e9 / 1458
PROFILE_ROUND = "r06"


def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        while True:
            b = f.read(1 << 24)
            if not b:
                break
            h.update(b)
    return h.hexdigest()


def kernels_fingerprint():
    """sha256 over the MSM kernel sources: the PMC traffic figure in profiles/ is only quoted while it matches."""
    h = hashlib.sha256()
    for name in ("msm_kernels.hip.h", "msm_host.hpp", "curve753.hip.h", "fp753.hip.h"):
        with open(os.path.join(ROOT, "snark-challenge-prover-reference_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def respawn_under_torchrun(args):
    """`python bench.py --gpus N` (N > 1) without a launcher: start the documented torchrun command as a CHILD before anything
    touches the GPU (never exec after HIP initialisation) and pass its exit code on."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


# ---- the exchange of the sharded path over RCCL -------------------------------------------------------------------------
def time_exchange(pkg, device, reps=100):
    """Mean / min latency in microseconds of `reps` all_gathers of one G1 projective point (36 u64) and of the block of three partial
    points of a proof (A, B2 over Fq2, C: 36 + 72 + 36 u64) through parallel.PointExchange on the initialised process group."""
    import numpy as np
    out = {}
    for name, words in (("g1_point", 36), ("proof_block", 144)):
        ex = pkg.parallel.PointExchange(words, device)
        local = np.arange(words, dtype=np.uint64) + 1
        for _ in range(5):
            got = ex.all_gather(local)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = ex.all_gather(local)
            ts.append(time.perf_counter() - t0)
        assert all(np.array_equal(g, local) for g in got), "exchange returned other words than were sent"
        out[name] = {"words": words, "mean_us": 1e6 * sum(ts) / len(ts), "min_us": 1e6 * min(ts)}
    return out


def exchange_probe_main():
    """Child process of the N = 1 run: a world-size-1 RCCL communicator on cuda:0 (backend "nccl" is RCCL on ROCm) and the
    exchange through it.  Prints one JSON line."""
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import socket
    import torch
    import torch.distributed as dist
    from __graft_entry__ import load_package
    pkg = load_package()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    t0 = time.perf_counter()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
    res = time_exchange(pkg, device)
    res["backend"] = dist.get_backend()
    res["init_and_first_exchange_s"] = None
    res["librccl_mapped"] = any("librccl" in l for l in open("/proc/self/maps"))
    try:
        res["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())   # what the box's librccl reports
    except Exception as e:   # noqa: BLE001 -- a label, never a reason to lose the measurement
        res["rccl_version"] = f"unknown ({type(e).__name__})"
    res["setup_s"] = time.perf_counter() - t0
    dist.destroy_process_group()
    print(json.dumps(res), flush=True)


def exchange_abi_probe_main():
    """Child process of the N = 1 run: the same exchange INSIDE the C ABI (mnt753_exchange_points: ncclCommInitAll over the prover's
    devices, one ncclAllGather per device in a group call; what `main_hip --fold rccl` uses).  No torch in this process."""
    import numpy as np
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg.init(0)
    res = {}
    for name, words in (("g1_point", 36), ("proof_block", 144)):
        blk = np.arange(words, dtype=np.uint64) + 1
        t0 = time.perf_counter()
        got, us = pkg.api.exchange_points([blk])          # the first call builds the communicator
        first = time.perf_counter() - t0
        ts, inner = [], []
        for _ in range(105):
            t0 = time.perf_counter()
            got, us = pkg.api.exchange_points([blk])
            ts.append(time.perf_counter() - t0); inner.append(us)
        assert np.array_equal(got[0], blk)
        res[name] = {"words": words, "mean_us": 1e6 * sum(ts[5:]) / 100, "min_us": 1e6 * min(ts[5:]), "inside_the_call_mean_us": sum(inner[5:]) / 100}
        if name == "g1_point":
            res["communicator_setup_s"] = first
    res["librccl_mapped"] = any("librccl" in l for l in open("/proc/self/maps"))
    print(json.dumps(res), flush=True)


def exchange_leg():
    """Run the probes above as children before this process touches the GPU; a failure is reported, never fatal."""
    out = _exchange_child("--exchange-probe", "world-size-1 RCCL communicator on one MI355X through torch.distributed: the software path of the exchange "
                          "(pinned host -> device -> all_gather_into_tensor -> host), no xGMI hop")
    out["inside_the_c_abi"] = _exchange_child("--exchange-probe-abi", "mnt753_exchange_points (ncclCommInitAll over the prover's devices, ncclAllGather in a group call): "
                                              "what main_hip --fold rccl puts in front of the serial fold; one device here, no xGMI hop")
    return out


def _exchange_child(flag, note):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), flag], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")))
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode == 0 and lines:
            return dict(json.loads(lines[-1]), world_size=1, note=note)
        return {"error": (r.stderr or r.stdout)[-400:]}
    except Exception as ex:
        return {"error": repr(ex)[:300]}


# ---- PMC traffic of the dominant phase, measured in this run ---------------------------------------------------------
def live_traffic():
    """FETCH_SIZE / WRITE_SIZE of the bucket-accumulation kernels of one 2^20 G1 MSM, from two rocprofv3 --pmc passes over a short
    run of this same script (child processes, started before this process touches the GPU; counters in their own runs with no trace
    domains, as the microarch guide prescribes).  Units and the gfx950 correction as in its HBM section: counters in KB, FETCH_SIZE
    doubled (128-B requests tallied at 64 B for 16-B-per-lane loads; the row gathers of the first level are an uncalibrated pattern, so
    the raw sum is reported beside it).  Returns None when rocprofv3 is not there or a pass fails."""
    import glob
    import shutil
    import sqlite3
    if shutil.which("rocprofv3") is None:
        return None
    per = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="bench_pmc_", dir="/tmp")
        try:
            cmd = ["rocprofv3", "--pmc", ctr, "-d", d, "-o", "pmc", "--", sys.executable, os.path.abspath(__file__), "--steps", "2", "--warmup", "1"]
            r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=600)
            dbs = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
            if r.returncode != 0 or not dbs:
                return None
            con = sqlite3.connect(dbs[0]); cur = con.cursor()
            t = [x[0] for x in cur.execute("select name from sqlite_master where type='table'")]
            kd = [x for x in t if "kernel_dispatch" in x][0]; ks = [x for x in t if "kernel_symbol" in x][0]
            pm = [x for x in t if "pmc_event" in x][0]; pi = [x for x in t if "info_pmc" in x][0]
            q = (f"select s.display_name, e.value from {pm} e join {pi} p on e.pmc_id = p.id join {kd} d on e.event_id = d.event_id "
                 f"join {ks} s on d.kernel_id = s.id where p.symbol = '{ctr}'")
            acc = {}
            for name, val in cur.execute(q):
                n = name.split("(")[0].replace("void mnt753::", "")
                if n.startswith("k_pair_level<mnt753::Mnt4G1") or n.startswith("k_bucket_accumulate<mnt753::Mnt4G1") or n.startswith("k_pair_fix<mnt753::Mnt4G1"):
                    acc.setdefault(n, []).append(val)
            con.close()
            msms = max((len(v) for k, v in acc.items() if k.startswith("k_bucket_accumulate")), default=0)
            if msms == 0:
                return None
            per[ctr] = {k: sum(v) / msms for k, v in acc.items()}
        except Exception:
            return None
        finally:
            shutil.rmtree(d, ignore_errors=True)
    f_kb, w_kb = sum(per["FETCH_SIZE"].values()), sum(per["WRITE_SIZE"].values())
    return {"source": "live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this run (2 timed MSMs + 1 warm-up each)",
            "FETCH_SIZE_KB_per_msm": f_kb, "WRITE_SIZE_KB_per_msm": w_kb, "raw_bytes_per_msm": (f_kb + w_kb) * 1024,
            "hbm_bytes_per_launch": (2 * f_kb + w_kb) * 1024,
            "per_kernel_FETCH_KB": per["FETCH_SIZE"], "per_kernel_WRITE_KB": per["WRITE_SIZE"],
            "correction": "MI355X_MICROARCH.md, HBM: KB units; FETCH_SIZE x 2 on gfx950 for 16-B-per-lane loads (gathers uncalibrated: raw figure beside it)"}


# ---- CPU baseline ------------------------------------------------------------------------------------------
def cpu_baseline(pkg, pts, sc, np):
    """The reference's own multi_exp (BDLO12, chunks = host threads -- what B::multiexp_G1 runs) through oracle/_ref/ref_msm_bench
    when that build is present (kind "reference"), else the oracle's restatement of it (kind "port"), on a bounded prefix of
    the benchmark input.  Returns (dict, affine result, sample size)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_msm_bench")
    cores = os.cpu_count() or 1
    if os.access(ref, os.X_OK):
        # the whole benchmark input (2^20 pairs: ~25 s on the 256 host threads of an MI355X box): the reference's result then
        # cross-checks exactly what was timed; BENCH_CPU_SAMPLE_LOG2 shrinks the sample on small hosts
        n2 = min(1 << int(os.environ.get("BENCH_CPU_SAMPLE_LOG2", "20")), len(pts))
        with tempfile.NamedTemporaryFile(dir=os.environ.get("TMPDIR", "/tmp"), suffix=".bin") as f:
            pts[:n2].tofile(f); sc[:n2].tofile(f); f.flush()
            r = subprocess.run([ref, f.name, str(n2)], capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode == 0 and lines:
            j = json.loads(lines[-1])
            got = np.array([int(j["result_affine_hex"][16 * i:16 * i + 16], 16) for i in range(24)], dtype=np.uint64)
            return dict(value=j["points_per_s"], unit="points/s", cores=j["threads"], kind="reference",
                        sample=f"{'all' if n2 == len(pts) else 'first'} 2^{n2.bit_length() - 1} (base, scalar) pairs of the benchmark input; libff multi_exp_with_mixed_addition<BDLO12> of the "
                               f"reference compiled by oracle/build_ref.sh, {j['threads']} OpenMP chunks of {n2 // j['threads']} points, {j['seconds']:.1f} s"), got, n2
    import oracle_lib as O
    threads = O.lib().oracle_max_threads()
    n = 1 << 12
    t0 = time.time(); O.msm(0, 1, pts[:n], sc[:n], chunks=threads); t_small = time.time() - t0
    n2 = n
    while n2 < (1 << 19) and t_small * (n2 * 2 / n) < 15.0:   # scale the sample towards ~12 s of CPU work
        n2 *= 2
    t0 = time.time(); got = O.msm(0, 1, pts[:n2], sc[:n2], chunks=threads); dt = time.time() - t0
    return dict(value=n2 / dt, unit="points/s", cores=threads, kind="port",
                sample=f"first 2^{n2.bit_length() - 1} (base, scalar) pairs of the benchmark input, oracle chunked BDLO12 ({threads} chunks of {n2 // threads} points; "
                       f"measured 1.5x slower than the reference's GMP build on 8 cores, BASELINE.md), {dt:.1f} s"), got, n2


# ---- full prove ----------------------------------------------------------------------------------------------
def _run_ref_main(curve_name, pp, ip, op):
    """The reference's own prover on this box's host cores (oracle/_ref/main = libsnark/main.cpp compiled where it lies; the
    oracle's restatement oracle/oracle_main when that build is absent).  Returns (dict, sha256 of its output or None)."""
    ref = os.path.join(ROOT, "oracle", "_ref", "main")
    port = os.path.join(ROOT, "oracle", "oracle_main")
    exe, kind = (ref, "reference") if os.access(ref, os.X_OK) else (port, "port")
    if not os.access(exe, os.X_OK):
        return {"error": "no CPU prover built (oracle/_ref/main, oracle/oracle_main)"}, None
    t0 = time.time()
    r = subprocess.run([exe, curve_name, "compute", pp, ip, op], capture_output=True, text=True)
    wall = time.time() - t0
    if r.returncode != 0:
        return {"error": r.stderr[-300:], "kind": kind}, None
    m = re.search(r"Total time from input to output:[ :]*([0-9.]+) ?(ms|s)", r.stdout)
    secs = (float(m.group(1)) / (1e3 if m.group(2) == "ms" else 1.0)) if m else None
    return {"kind": kind, "input_to_output_s": secs, "wall_incl_params_s": round(wall, 3), "threads": os.cpu_count(),
            "timing_window": "libsnark/main.cpp:203-270, printed at :270"}, sha256_file(op)


def _prover_times(stdout):
    m1 = re.findall(r"Total time from input to output: ([0-9.]+)s", stdout)
    m2 = re.search(r"load params: ([0-9.]+)s", stdout)
    return [float(x) for x in m1], (float(m2.group(1)) if m2 else None)


def prove_leg(log2_d=20, curve_name="MNT4753", cpu=False, repeat=3, gpus=1, share=False, cold=True):
    """main_hip on the seeded synthetic files; hash compared with the reference-minted one (or, where no hash was minted for
    the size, with the bytes the reference prover writes here, cpu=True).

    Runs in child processes BEFORE this process initialises the GPU: the metric is the reference's -- a fresh `./main` on
    an otherwise idle device.  A harness that already holds a GPU context and freed device memory measured the same prover
    4-8 % slower (0.202-0.213 s against 0.194-0.198 s stand-alone, profiles/r02) and its parameter load 25 % slower."""
    exe = os.path.join(ROOT, "snark-challenge-prover-reference_amd", "main_hip")
    key = f"{curve_name}_2p{log2_d}"
    expected = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_hashes.json"))).get(key)
    work = tempfile.mkdtemp(prefix="bench_prove_", dir=os.environ.get("TMPDIR", "/tmp"))
    pp, ip, op, oc = (os.path.join(work, k) for k in ("params", "input", "output", "output_cpu"))
    out = {"curve": curve_name, "log2_d": log2_d, "n_gpus": gpus}
    cpu_out = None
    dev_flags = ["--gpus", str(gpus)] if gpus > 1 else []
    # BENCH_SHARE_GPU=1 (development, the one-GPU test box): the logical devices of the sharded prover share the visible GPU
    child_env = dict(os.environ, MNT753_SHARE_DEVICE="1") if share and gpus > 1 else dict(os.environ)
    try:
        t0 = time.time()
        g = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "synth_files.py"), curve_name, str(log2_d), pp, ip], capture_output=True, text=True)
        if g.returncode != 0:
            out.update(error=g.stderr[-400:], parity_ok=False)
            return out, cpu_out
        d = (1 << log2_d) - 1
        out.update(d=d, m=d + 1, synth_files_s=round(time.time() - t0, 2))
        files_ok = (sha256_file(pp) == expected["params_sha256"] and sha256_file(ip) == expected["input_sha256"]) if expected else None
        # A prover that starts right behind another GPU process waits for the driver to take back the device memory that one returned
        # (measured on one box: parameter load 3.84 s first, 7.0 s right behind another prover, 3.85 s after 20 s;
        # profiles/r05/load_params_fresh_box.log) -- and this leg runs behind the bench's own profiled children: it starts after a pause
        pause = 20.0 if log2_d >= 17 else 2.0
        time.sleep(pause)
        out["pause_before_s"] = pause
        t0 = time.time()
        # `repeat` proofs of the same input in ONE process: the first is the reference's metric (fresh process, parameters loaded,
        # then input -> output); the others show what a resident prover pays per proof
        # (every prover child under a timeout: a hang on hardware this builder never saw -- several real GPUs -- must cost one leg, not the run)
        try:
            r = subprocess.run([exe, curve_name, "compute", pp, ip, op, "--repeat", str(repeat)] + dev_flags, capture_output=True, text=True,
                               env=dict(child_env, MNT753_TRACE_LOAD="1"), timeout=900)   # phases of the parameter load on stderr; nothing is printed inside a proof's window (MNT753_TRACE would)
        except subprocess.TimeoutExpired:
            out.update(error="main_hip did not finish within 900 s", parity_ok=False)
            return out, cpu_out
        wall = time.time() - t0
        if r.returncode != 0:
            out.update(error=r.stderr[-400:], parity_ok=False)
            return out, cpu_out
        m1 = re.search(r"Total time from input to output: ([0-9.]+)s", r.stdout)   # the first proof
        m2 = re.search(r"load params: ([0-9.]+)s", r.stdout)
        sha = sha256_file(op)
        out["prover_stdout_first_proof"] = [l for l in r.stdout.strip().splitlines()][:9]
        out["load_params_phases"] = [re.sub(r"\s+", " ", l.replace("mnt753: load params: ", "")) for l in r.stderr.splitlines() if l.startswith("mnt753: load params: ")]
        out.update(input_to_output_s=float(m1.group(1)) if m1 else None, load_params_s=float(m2.group(1)) if m2 else None,
                   wall_incl_params_s=round(wall, 3), sha256=sha,
                   timing_window="libsnark/main.cpp:203-270 (input load + compute + output write; parameters resident)",
                   note=f"first of --repeat {repeat} in one process; B::read_params ends with one warm-up MSM per base set (parameter-load time, outside "
                        "the window as in main.cpp:201-203); the reference's literal metric, the first proof of a process that has run nothing yet, is "
                        "`cold_process` (MNT753_NO_WARMUP=1) beside it")
        m3 = re.findall(r"Total time from input to output: ([0-9.]+)s", r.stdout)
        if len(m3) > 1:
            out["input_to_output_s_all"] = [float(x) for x in m3]
            out["resident_proof_s"] = min(float(x) for x in m3[1:])
        if expected:
            out.update(sha256_expected=expected["output_sha256"], synthetic_files_match_minted=files_ok,
                       parity_ok=bool(files_ok) and sha == expected["output_sha256"],
                       expected_from="tests/golden/oracle_hashes.json: oracle/_ref/main (the reference, bos_coster) on the same seeded files")
        if gpus > 1:
            out["sharding"] = (f"main_hip --gpus {gpus}: every parameter vector cut into {gpus} contiguous slices, one MSM per slice and device, partial points "
                               "folded in rank order (multiexp.tcc:417-440); compute_H spread over devices 0 / 1 / 2" + ("; logical devices share ONE GPU (development)" if share else ""))
        # the same files through further children: (a) a COLD process -- no warm-up MSM at parameter-load time, the reference's literal
        # metric (main.cpp:196-203: parameters loaded, nothing run yet); (b) with several devices, the fold over RCCL inside the boundary
        side = []
        if cold:
            side.append(("cold_process", ["--repeat", "2"], {"MNT753_NO_WARMUP": "1"},
                         "MNT753_NO_WARMUP=1: B::read_params builds the tables but runs nothing; the first proof pays first-touch page faults and code loading"))
        if gpus == 1:
            side.append(("one_shot", [], {"MNT753_TRACE_LOAD": "1"},
                         "`main_hip <curve> compute <params> <input> <output>` as the reference's CLI is invoked (libsnark/main.cpp:274-293): one proof per "
                         "process, so no window tables and no warm-up MSM (host/main.cpp); wall_incl_params_s is the clock around the whole process"))
        if gpus > 1:
            side.append(("fold_rccl", ["--repeat", "2", "--fold", "rccl", "--peer-bench"], {"MNT753_TRACE": "1"},
                         "partial points through mnt753_exchange_points (ncclAllGather over the prover's devices) in front of the serial fold"))
        # the side children start after the same pause (without the warm-up MSM the driver's reclaim can land INSIDE the first proof:
        # 0.18 s on a settled device, 0.9-1.0 s behind another process; both are reported as measured)
        for key, flags, env_extra, note in side:
            for q in (op,):
                if os.path.exists(q):
                    os.remove(q)
            time.sleep(pause)
            t0 = time.time()
            try:
                r2 = subprocess.run([exe, curve_name, "compute", pp, ip, op] + flags + dev_flags, capture_output=True, text=True, env=dict(child_env, **env_extra), timeout=600)
            except subprocess.TimeoutExpired:
                out[key] = {"error": "main_hip did not finish within 600 s"}
                continue
            if r2.returncode != 0:
                out[key] = {"error": r2.stderr[-300:]}
                continue
            ts, lp = _prover_times(r2.stdout)
            sha2 = sha256_file(op)
            out[key] = {"input_to_output_s": ts[0] if ts else None, "input_to_output_s_all": ts, "load_params_s": lp, "wall_incl_params_s": round(time.time() - t0, 3),
                        "same_bytes": sha2 == sha, "pause_before_s": pause, "note": note}
            if key == "one_shot":
                out["one_shot_wall_s"] = out[key]["wall_incl_params_s"]
                out[key]["one_shot_policy_applied"] = "one-shot prover" in r2.stdout
                out[key]["load_params_phases"] = [re.sub(r"\s+", " ", l.replace("mnt753: load params: ", "")) for l in r2.stderr.splitlines() if l.startswith("mnt753: load params: ")]
            if key == "fold_rccl":
                out[key]["folded"] = "over RCCL" if "over RCCL" in r2.stderr else ("on the host (no communicator: " + ("logical devices share a GPU" if share else "librccl unavailable") + ")")
                # what the box granted for the device pairs the sharded prover copies between (one MNT753_TRACE line per ordered pair)
                pairs = [l for l in r2.stderr.splitlines() if l.startswith("mnt753: device ") and " reads device " in l]
                out["peer_access"] = {"ordered_pairs": len(pairs), "direct": sum("direct" in l for l in pairs), "staged_through_host": sum("staged" in l for l in pairs),
                                      "same_gpu": sum("same GPU" in l for l in pairs)}
                # the copies DESIGN.md section 5 assumes at 2.0 ms per 100 MB, measured by the child on this box (main_hip --peer-bench)
                copies = re.findall(r"peer copy 100 MB device (\d+) -> (\d+): ([0-9.]+) ms \(([0-9.]+) GB/s\), (.*)", r2.stdout)
                if copies:
                    out["peer_copy_100MB"] = [{"src": int(a), "dst": int(b), "ms": float(ms), "GB_per_s": float(gb), "path": how.strip()} for a, b, ms, gb, how in copies]
                    to0 = [c["ms"] for c in out["peer_copy_100MB"] if c["dst"] == 0]
                    out["peer_copy_100MB_to_device0_ms"] = max(to0) if to0 else None
                    out["peer_copy_note"] = ("measured on this box; values on logical devices that share one GPU are local copies, not xGMI" if share else
                                             "measured on this box: what DESIGN.md section 5 assumed at 2.0 ms")
                lat = [float(m) for m in re.findall(r"devices in ([0-9.]+) us", r2.stderr)]
                if lat:
                    out[key]["all_gather_us"] = {"first": lat[0], "min": min(lat), "calls": len(lat)}
            if sha2 != sha:
                out["parity_ok"] = False
        if cpu:
            cpu_out, cpu_sha = _run_ref_main(curve_name, pp, ip, oc)
            cpu_out.update(curve=curve_name, log2_d=log2_d, sha256=cpu_sha, same_bytes_as_gpu=(cpu_sha == sha) if cpu_sha else None)
            if expected and cpu_sha:
                cpu_out["matches_minted_hash"] = cpu_sha == expected["output_sha256"]
            if not expected:   # no minted hash for this size: the live reference run IS the parity check
                out.update(parity_ok=bool(cpu_sha) and cpu_sha == sha, expected_from="the reference prover run by this bench on the same files (cpu_prove)")
            if cpu_out.get("input_to_output_s") and out.get("input_to_output_s"):
                cpu_out["gpu_input_to_output_s"] = out["input_to_output_s"]
    finally:
        for p in (pp, ip, op, oc):
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(work)
    return out, cpu_out


def prove_legs(gpus=1, share=False, log2_d4=20, log2_d6=15):
    """All the prove legs of the bench line, before this process touches the GPU.  gpus > 1: main_hip --gpus N (no CPU provers: the
    N = 1 line carries them)."""
    legs = {}
    if gpus > 1:
        legs["prove"], _ = prove_leg(log2_d4, "MNT4753", gpus=gpus, share=share)
        legs["prove_mnt6753"], _ = prove_leg(log2_d6, "MNT6753", gpus=gpus, share=share)
        return legs
    want_cpu = os.environ.get("BENCH_CPU_PROVE", "1") != "0"
    # BASELINE.json's metric is the prove time on the FULL MNT4753 parameters "next to the CPU ./main baseline timed on the same box's
    # host cores": the reference's own prover runs the same 2^20 files right after main_hip (libsnark/main.cpp:203-270; minutes of CPU
    # time -- 401-551 s on the 8 cores of the build container).  BENCH_CPU_PROVE_FULL=0 runs the 2^17 files instead.
    full = want_cpu and os.environ.get("BENCH_CPU_PROVE_FULL", "1") != "0"
    legs["prove"], cpu4 = prove_leg(20, "MNT4753", cpu=full)
    legs["prove_mnt6753"], cpu6 = prove_leg(15, "MNT6753", cpu=want_cpu)
    cpu = []
    if cpu6:
        cpu.append(cpu6)
    if want_cpu and not full:
        gpu4, cpu4 = prove_leg(17, "MNT4753", cpu=True, repeat=1)   # no minted hash at that size: its bytes are compared with main_hip's directly
        if cpu4:
            cpu4["gpu_parity_ok"] = gpu4.get("parity_ok")
    if cpu4:
        cpu.append(cpu4)
    legs["cpu_prove"] = cpu
    return legs


def _u64_as_f64(words, np):
    """u64 words -> float64 pairs (low 32 bits, high 32 bits): exact, since float64 holds any 32-bit integer"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return np.stack([w & np.uint64(0xFFFFFFFF), w >> np.uint64(32)], axis=-1).astype(np.float64)


def dump_outputs(path, pkg, np, out):
    """What the timed step hands its caller, from the last timed step: the G1 MSM result over the whole benchmark input (seeds 42 / 43,
    so the same arguments give the same inputs), as DIR/msm_affine.npy -- the point's affine coordinates (x, y; 12 u64 limbs each).
    The step returns projective wire words, whose scaling (X, Y, Z) may differ from run to run for the same point; the affine form is
    the value itself.  Each u64 limb is stored as its two 32-bit halves (low, high) in float64, so the array is exact: shape (2, 12, 2)."""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "msm_affine.npy"), _u64_as_f64(pkg.point_to_affine(0, 1, out), np).reshape(2, 12, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-n", type=int, default=LOG_N, help="log2 of the bases per GPU (benchmark config: 20)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, run every other leg and check of the line (parity, prove legs, CPU baselines, RCCL exchange, "
                         "live PMC traffic, extras, weak scaling; see the module docstring); a plain run only sets up, times and reports the steps")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU MSM baseline")
    ap.add_argument("--no-prove", action="store_true", help="--full without the full-prove legs")
    ap.add_argument("--no-extras", action="store_true", help="--full without the FFT / compute_H / G2 / table-less legs")
    ap.add_argument("--no-traffic", action="store_true", help="--full without the two rocprofv3 --pmc passes that measure the HBM traffic of the dominant phase")
    ap.add_argument("--no-exchange", action="store_true", help="--full without the RCCL exchange-latency leg")
    ap.add_argument("--prove-log2-d", type=int, nargs=2, default=None, metavar=("MNT4753", "MNT6753"),
                    help="sizes of the prove legs of --full (default 20 15 = the metric's; tests pass sizes with a minted hash, e.g. 14 10); runs them whatever --log-n is")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the MSM result of the last one as DIR/msm_affine.npy (see dump_outputs)")
    ap.add_argument("--exchange-probe", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--exchange-probe-abi", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.exchange_probe:
        return exchange_probe_main()
    if args.exchange_probe_abi:
        return exchange_abi_probe_main()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(respawn_under_torchrun(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s); run `python bench.py --gpus N` or torchrun with --nproc-per-node N")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    # A profiled run (rocprofv3 preloads its library, which initialises the GPU before main) must not start further GPU children: no
    # prove legs, no exchange probes, no PMC passes under the profiler.
    under_profiler = "rocprof" in os.environ.get("LD_PRELOAD", "") or any(k.startswith("ROCPROF") for k in os.environ)
    share = os.environ.get("BENCH_SHARE_GPU") == "1"
    # the full-prove leg first, in child processes, while NO rank has touched a GPU yet (see prove_leg).  N > 1: rank 0 runs
    # `main_hip ... --gpus N` (one process over the N devices); the other ranks wait on a CPU-side barrier -- a file named after the
    # launcher (same parent process and rendezvous port for all ranks of one launch).
    legs = None
    want_prove = args.full and not args.no_prove and not under_profiler and (args.log_n == LOG_N or args.prove_log2_d is not None)
    d4, d6 = args.prove_log2_d if args.prove_log2_d else (20, 15)
    if want_prove and world == 1:
        legs = prove_legs() if args.prove_log2_d is None else {"prove": prove_leg(d4, "MNT4753")[0], "prove_mnt6753": prove_leg(d6, "MNT6753")[0], "cpu_prove": []}
    elif want_prove:
        # one gate per launch: the launcher's pid, its rendezvous port and (torchrun) its run id name it, so that a stale file of an
        # earlier launch cannot let ranks through; rank 0 writes its outcome into it and the others leave at once when it failed
        gate = os.path.join(os.environ.get("TMPDIR", "/tmp"),
                            f"bench_prove_{os.getppid()}_{os.environ.get('MASTER_PORT', '0')}_{os.environ.get('TORCHELASTIC_RUN_ID', 'none')}.done")
        if rank == 0:
            status = "failed"
            try:
                if os.path.exists(gate):
                    os.remove(gate)
                legs = prove_legs(world, share, d4, d6)
                status = "ok"
            finally:
                with open(gate + ".tmp", "w") as f:
                    f.write(status + "\n")
                os.replace(gate + ".tmp", gate)
        else:
            t_wait = time.time()
            while not os.path.exists(gate):
                if time.time() - t_wait > 3600:
                    raise SystemExit("bench.py: rank 0's prove legs did not finish within an hour")
                time.sleep(0.2)
            if open(gate).read().strip() != "ok":
                raise SystemExit("bench.py: rank 0's prove legs failed; this rank leaves before it touches a GPU")
    exchange = None
    if args.full and world == 1 and not args.no_exchange and args.log_n == LOG_N and not under_profiler:
        exchange = exchange_leg()
    traffic_live = None
    if args.full and world == 1 and not args.no_traffic and args.log_n == LOG_N and not under_profiler:   # (a profiled run has the GPU initialised already)
        traffic_live = live_traffic()

    import numpy as np
    import torch
    import torch.distributed as dist
    from __graft_entry__ import load_package
    pkg = load_package()

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    # BENCH_SHARE_GPU=1 (development only): all ranks share GPU 0 and exchange over gloo, to exercise the N > 1 flow
    # on a single-GPU box; the real multi-GPU run is one rank per GPU over RCCL.
    dev_index = 0 if share else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)
    pkg.init(dev_index)

    n = 1 << args.log_n
    if world > 1 and not share:
        assert dist.get_backend() == "nccl" and dist.get_world_size() == args.gpus, "bench.py --gpus N runs N ranks over RCCL"
    stream = torch.cuda.current_stream().cuda_stream
    comm_dev = None if share else device

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            res = fn()
        phases = []
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            res = fn()
            phases.append(pkg.msm_last_timing())
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if share else device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        return res, elapsed, phases

    # The benchmark input: ONE array of 2^log_n (base, scalar) pairs (seeds 42 / 43).  N = 1: this rank owns all of it.  N > 1, the
    # headline: rank g owns the contiguous slice g of it (multiexp.tcc:417-431), resident with its window table before timing.
    lo, hi = pkg.parallel.shard_range(n, rank, world)
    pts = pkg.synth_points(0, 1, 42, n)
    sc = pkg.synth_scalars(0, 43, n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bases = pkg.BaseSet(0, 1, pts[lo:hi])                           # parameters: resident before timing (main.cpp:201-203)
    torch.cuda.synchronize()
    precompute_ms = (time.perf_counter() - t0) * 1e3
    d_sc = torch.from_numpy(sc[lo:hi].copy().view(np.int64)).to(device)   # scalars resident in HBM

    def step():
        local = bases.msm(d_sc.data_ptr(), n=hi - lo, on_device=True, stream=stream)
        return pkg.parallel.msm_sharded(pkg.api, 0, 1, local, comm_dev)

    out, elapsed, tot_ms = timed(step, args.steps, args.warmup)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, pkg, np, out)
    if args.full and world > 1:
        try:
            exchange = dict(time_exchange(pkg, comm_dev), world_size=world, backend=dist.get_backend(),
                            note="the run's own communicator: " + ("gloo on a shared GPU (development)" if share else "RCCL, one rank per GPU over xGMI"))
        except Exception as ex:
            exchange = {"error": repr(ex)[:300]}
    acc_ms = [t["accumulate_ms"] for t in tot_ms]
    plan = pkg.msm_last_plan()
    ok = True   # the checks of --full; a plain run makes none
    if args.full:
        # parity of what was just timed: the whole array through its discrete logs (one host scalar multiplication)
        exp = pkg.synth_expected_msm(0, 1, 42, sc)
        ok = bool(np.array_equal(pkg.point_to_affine(0, 1, out), pkg.point_to_affine(0, 1, exp)))

    # weak scaling beside it (N > 1): 2^log_n points PER GPU, rank g with its own array, same exchange and fold
    weak = None
    if args.full and world > 1:
        bases.close()
        pts_w = pkg.synth_points(0, 1, 42 + 1000 * rank, n) if rank else pts
        sc_w = pkg.synth_scalars(0, 43 + 1000 * rank, n) if rank else sc
        bw = pkg.BaseSet(0, 1, pts_w)
        d_w = torch.from_numpy(sc_w.view(np.int64)).to(device)

        def step_weak():
            local = bw.msm(d_w.data_ptr(), n=n, on_device=True, stream=stream)
            return pkg.parallel.msm_sharded(pkg.api, 0, 1, local, comm_dev)

        w_out, w_elapsed, _ = timed(step_weak, args.steps, args.warmup)
        w_exp = pkg.parallel.msm_sharded(pkg.api, 0, 1, pkg.synth_expected_msm(0, 1, 42 + 1000 * rank, sc_w), comm_dev)
        w_ok = bool(np.array_equal(pkg.point_to_affine(0, 1, w_out), pkg.point_to_affine(0, 1, w_exp)))
        weak = {"scaling": "weak", "workload": f"2^{args.log_n} MNT4753 G1 points per GPU, {world} GPUs, one all_gather + fold per MSM",
                "value": world * n * args.steps / w_elapsed, "unit": "points/s", "ms_per_step": w_elapsed / args.steps * 1e3, "parity_ok": w_ok}
        ok = ok and w_ok
        bw.close(); del d_w

    line = None
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = n * args.steps / elapsed
        acc = float(np.mean(acc_ms))
        n_local = hi - lo                       # pairs one launch of the dominant kernels processes on this rank
        achieved = ALGO_BYTES_PER_PAIR * n_local / (acc * 1e-3) / 1e9
        plan_c, windows = plan["window_bits"], plan["windows"]
        regular_levels, irr_levels = plan.get("pair_levels", 0), plan.get("irr_levels", 0)
        levels = regular_levels + irr_levels    # irregular levels: the same batched-affine addition on what the regular ones leave (no padding)
        # Montgomery products per sorted entry: an affine pair addition is 5 products + 1 squaring (0.76 of a product) including
        # the 3 of the simultaneous inversion, on 1/2, 1/4, ... of the entries; one divstep inversion (~94 products) per lane and
        # level over B = slots / 65536 lanes (at least 48); 11 per mixed addition on what is left
        slots = [windows * n_local / 2 ** l for l in range(1, levels + 1)]
        prod_per_entry = sum((5.76 + 94.0 / max(8.0, sl / 65536.0)) / 2 ** l for l, sl in zip(range(1, levels + 1), slots)) + 11.0 / 2 ** levels
        kernel_name = "k_bucket_accumulate<Mnt4G1>" if levels == 0 else (
            f"k_pair_level<Mnt4G1> x{regular_levels}" + (f" + x{irr_levels} irregular" if irr_levels else "") + " + k_bucket_accumulate<Mnt4G1>")
        # PMC traffic of the same phase (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, tools/collect_profiles.sh); quoted only
        # while the kernel sources are the ones it was measured on
        traffic, traffic_info = None, None
        if traffic_live:
            traffic = traffic_live["hbm_bytes_per_launch"]
            traffic_info = dict(traffic_live, achieved_GBps=traffic / (acc * 1e-3) / 1e9, frac_of_hbm_peak=traffic / (acc * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                                raw_over_algorithmic=traffic_live["raw_bytes_per_msm"] / (ALGO_BYTES_PER_PAIR * n_local))
        else:
            # no live passes (rocprofv3 absent, --no-traffic, N > 1): the figure of profiles/, quoted only while the kernel sources are
            # the ones it was measured on
            tpath = os.path.join(ROOT, "profiles", PROFILE_ROUND, "accumulate_traffic.json")
            if os.path.exists(tpath) and args.log_n == LOG_N and world == 1:
                tj = json.load(open(tpath))
                if tj.get("kernels_fingerprint") == kernels_fingerprint():
                    traffic = tj.get("hbm_bytes_per_launch")
                    traffic_info = {"source": f"profiles/{PROFILE_ROUND}/accumulate_traffic.json", "kernels_fingerprint": tj.get("kernels_fingerprint"),
                                    "achieved_GBps": traffic / (acc * 1e-3) / 1e9 if traffic else None,
                                    "frac_of_hbm_peak": traffic / (acc * 1e-3) / 1e9 / HBM_PEAK_GBPS if traffic else None}
                else:
                    traffic_info = {"stale": True, "note": "profiles traffic was measured on different kernel sources; re-run tools/collect_profiles.sh"}
        line = {
            "metric": "G1 MSM points/sec at 2^20 (MNT4753)",
            "value": value,
            "unit": "points/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            # ONE 2^20 array whatever N: the series over N = 1, 2, 4, 8 is a strong-scaling series and the N = 1 line is its first point
            # (`weak`, N > 1 only, carries 2^20 points PER GPU)
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "u32x27 limbs / u64 columns",
            "data": "synthetic",
            "config": {"workload": f"MNT4753 G1 Pippenger MSM, 2^{args.log_n} bases" + (f" split into {world} contiguous slices (one per GPU)" if world > 1 else "") +
                                   ", bit-exact vs libff::multi_exp",
                       "curve": "MNT4753", "group": "G1", "points": n, "points_per_gpu": n_local, "window_bits": plan_c, "windows": windows,
                       "window_table": plan["window_table"],
                       "limbs": "27 x 28-bit limbs in u32 registers, 64-bit multiply-add columns (v_mad_u64_u32 / v_mad_i64_i32); exact integer arithmetic",
                       "parallelism": f"slice-per-gpu x{world}, all_gather (RCCL) of one projective point per rank, serial fold (multiexp.tcc:417-440)"},
            "roofline": {"bound": "int-mad (hbm fraction reported per contract)", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                         "traffic": traffic, "traffic_info": traffic_info, "kernel": kernel_name, "kernel_ms": acc,
                         "algorithmic_bytes_per_launch": ALGO_BYTES_PER_PAIR * n_local,
                         "note": "bucket accumulation phase of one MSM (HIP events on the launch stream). `achieved` is ALGORITHMIC bytes / time as the "
                                 "contract asks; the phase is bound by the 753-bit multiplier (modmul_frac) and, in the first pairing level, by scattered "
                                 "table-row gathers (traffic_info.frac_of_hbm_peak), not by streaming",
                         "pair_levels": regular_levels, "irregular_levels": irr_levels, "products_per_entry": prod_per_entry,
                         "modmul_per_s": prod_per_entry * windows * n_local / (acc * 1e-3), "modmul_peak_per_s": MODMUL_PEAK_PER_S,
                         "modmul_frac": prod_per_entry * windows * n_local / (acc * 1e-3) / MODMUL_PEAK_PER_S,
                         "modmul_peak_first_principles_per_s": MODMUL_PEAK_FIRST_PRINCIPLES_PER_S,
                         "modmul_frac_of_first_principles": prod_per_entry * windows * n_local / (acc * 1e-3) / MODMUL_PEAK_FIRST_PRINCIPLES_PER_S,
                         "modmul_peak_note": "modmul_peak_per_s is MEASURED (multiplier microbenchmark, 1.96 GHz sustained); the first-principles figure is 1024 SIMDs x 16 "
                                             "lanes x 2.4 GHz / 1458 multiply-adds -- at a nominal clock the chip does not hold under integer multiply-add load",
                         "mixed_addition_equivalents_per_s": windows * n_local / (acc * 1e-3)},
            "phases_ms": {k: float(np.mean([t[k] for t in tot_ms])) for k in tot_ms[0]},
            "precompute_ms": precompute_ms,
        }
        if weak:
            line["weak"] = weak
        if exchange is not None:
            line["exchange"] = exchange
            if "g1_point" in exchange:
                line["exchange_us"] = exchange["g1_point"]["mean_us"]

    if world == 1:
        if args.full and not args.no_cpu_baseline:
            base, got, n2 = cpu_baseline(pkg, pts, sc, np)
            if n2 == n:      # the reference ran the whole benchmark input: compare with the result of the timed loop itself
                same = bool(np.array_equal(pkg.point_to_affine(0, 1, out), got))
            else:
                chk = pkg.BaseSet(0, 1, pts[:n2])
                same = bool(np.array_equal(pkg.point_to_affine(0, 1, chk.msm(sc[:n2])), got))
                chk.close()
            base["matches_gpu_on_sample"] = same
            line["cpu_baseline"] = base
            ok = ok and same
        if args.full and not args.no_extras and args.log_n == LOG_N:
            extras = {}
            # G1 MSM without the window table (what a caller pays who cannot keep 8.9 GB per base set resident)
            os.environ["MNT753_MSM_PRECOMP"] = "0"
            nt = pkg.BaseSet(0, 1, pts)
            del os.environ["MNT753_MSM_PRECOMP"]
            _, e2, _ = timed(lambda: nt.msm(d_sc.data_ptr(), n=n, on_device=True, stream=stream), max(3, args.steps // 2), 1)
            extras["no_table_ms_per_step"] = e2 / max(3, args.steps // 2) * 1e3
            # what `value` would be without the 9.4 GB window table per base set: beside the headline, not inside extras
            line["no_window_table"] = {"value": n / (extras["no_table_ms_per_step"] * 1e-3), "unit": "points/s", "ms_per_step": extras["no_table_ms_per_step"],
                                       "note": "same MSM with one bucket set per window (c = 16, W = 48) and no precomputed multiples: base sets below 4096 points, "
                                               "or hosts that cannot keep ~56 GB of tables per MNT4753 parameter set resident"}
            nt.close()
            bases.close()
            # 2^20 FFT and compute_H over Fr(MNT4753): BASELINE configs[2]; 192 B algorithmic per element per transform
            m = 1 << 20
            dom = pkg.Domain(0, m)
            vecs = [torch.from_numpy(pkg.synth_scalars(0, 70 + k, m).view(np.int64)).to(device) for k in range(3)]
            dh = torch.empty((m + 1) * 12, dtype=torch.int64, device=device)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def ev_time(fn, reps):
                fn(); torch.cuda.synchronize()
                ev0.record()
                for _ in range(reps):
                    fn()
                ev1.record(); torch.cuda.synchronize()
                return ev0.elapsed_time(ev1) / reps

            extras["fft_2p20_ms"] = ev_time(lambda: dom.fft(pkg.FFT, vecs[0].data_ptr(), stream=stream), 20)
            extras["fft_2p20_algorithmic_GBps"] = 192.0 * m / (extras["fft_2p20_ms"] * 1e-3) / 1e9
            extras["compute_h_2p20_ms"] = ev_time(lambda: dom.compute_h(vecs[0].data_ptr(), vecs[1].data_ptr(), vecs[2].data_ptr(), dh.data_ptr(), stream=stream), 5)
            # the pieces of compute_H a sharded prover spreads over devices: one chain x <- cosetFFT(iFFT(x)) per
            # vector, the joining step (pointwise + last transform), and the two loads device 0 still does before it can start
            extras["compute_h_chain_2p20_ms"] = ev_time(lambda: dom.compute_h_chain(vecs[0].data_ptr(), stream=stream), 5)
            extras["compute_h_finish_2p20_ms"] = ev_time(lambda: dom.compute_h_finish(vecs[0].data_ptr(), vecs[1].data_ptr(), vecs[2].data_ptr(), dh.data_ptr(), stream=stream), 5)
            try:
                with tempfile.NamedTemporaryFile(dir=os.environ.get("TMPDIR", "/tmp"), suffix=".bin") as f:
                    blob = np.zeros(96 * (m + (m >> 3)) // 8, dtype=np.uint64)     # 100 MB (one vector) + 12.5 MB (an eighth of w)
                    blob.tofile(f); f.flush()
                    tl = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        buf = pkg.DeviceBuffer.from_file(f.name, 0, blob.nbytes)
                        tl.append((time.perf_counter() - t0) * 1e3)
                        buf.close()
                    extras["input_load_112MB_ms"] = {"first": tl[0], "best": min(tl), "bytes": int(blob.nbytes),
                                                     "note": "one loader lane, file in the page cache: the range of w + one vector of compute_H that device 0 of an 8-way split streams before its chain"}
            except Exception as ex:
                extras["input_load_112MB_ms"] = {"error": repr(ex)[:200]}
            dom.close(); del vecs, dh
            # BASELINE configs[2] as a roofline object of its own (192 B per element per transform = 96 B read +
            # 96 B written once).  One transform = three launches of k_ntt_group (8 + 8 + 4 butterfly stages on LDS tiles), i.e. three
            # passes over HBM: 604 MB moved for 201 MB algorithmic; (m / 2) log2 m = 10.5 M butterflies, one product each but for the
            # first stage, whose only twiddle is 1 (skipped since round 4): 19 products per pair of elements.
            fft_s = extras["fft_2p20_ms"] * 1e-3
            line["roofline_fft"] = {"bound": "int-mad in its LDS passes (hbm fraction reported per contract)", "achieved": 192.0 * m / fft_s / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                    "frac": 192.0 * m / fft_s / 1e9 / HBM_PEAK_GBPS, "traffic": None,
                                    "kernel": "k_ntt_group x3 (one 2^20 FFT over Fr of MNT4753; HIP events on the launch stream)", "kernel_ms": extras["fft_2p20_ms"],
                                    "algorithmic_bytes_per_launch": 192 * m, "passes_over_hbm": 3, "moved_bytes_by_design": 3 * 192 * m,
                                    "moved_frac_of_hbm_peak": 3 * 192.0 * m / fft_s / 1e9 / HBM_PEAK_GBPS,
                                    "butterfly_products": (m // 2) * 19, "modmul_per_s": (m // 2) * 19 / fft_s,
                                    "modmul_frac": (m // 2) * 19 / fft_s / MODMUL_PEAK_PER_S,
                                    "compute_h_ms": extras["compute_h_2p20_ms"],
                                    "compute_h_algorithmic_GBps": 4 * 96.0 * m / (extras["compute_h_2p20_ms"] * 1e-3) / 1e9,
                                    "note": "bound by the 753-bit multiplier inside the LDS passes, not by HBM (basic_radix2_domain_aux.tcc:167-202 is the transform)"}
            # The witness-map front end at circuit scale (the first loop of r1cs_to_qap_witness_map,
            # r1cs_to_qap.tcc:223-237): 2^20 - 8 constraints, three matrices, 3 terms per row on average.  HBM-bound by design: per
            # term 96 B of the assignment gathered + 112 B coefficient + 4 B index, per row 96 B written + 16 B of row pointers.
            try:
                rng = np.random.default_rng(1)
                ncs, mv = m - 8, m - 1
                pool = pkg.synth_scalars(0, 901, 1024)
                mats = []
                for k in range(3):
                    cnt = rng.integers(1, 6, size=ncs)
                    rp = np.zeros(ncs + 1, dtype=np.uint64); rp[1:] = np.cumsum(cnt)
                    nnz = int(rp[ncs])
                    mats.append((rp, rng.integers(0, mv + 1, size=nnz).astype(np.uint32), pool[rng.integers(0, 1024, size=nnz)]))
                cs = pkg.R1cs(0, 5, mv, ncs, mats)
                terms = sum(int(t[0][ncs]) for t in mats)
                wv = torch.from_numpy(pkg.synth_scalars(0, 77, m).view(np.int64)).to(device)
                abc = [torch.empty(m * 12, dtype=torch.int64, device=device) for _ in range(3)]
                r1_ms = ev_time(lambda: cs.evaluate(wv.data_ptr(), abc[0].data_ptr(), abc[1].data_ptr(), abc[2].data_ptr(), m, stream=stream), 10)
                r1_bytes = terms * (96 + 112 + 4) + 3 * m * (96 + 16)
                extras["r1cs_evaluate_2p20"] = {"ms": r1_ms, "terms": terms, "rows": 3 * ncs, "bytes_by_design": r1_bytes,
                                                "GBps": r1_bytes / (r1_ms * 1e-3) / 1e9, "frac_of_hbm_peak": r1_bytes / (r1_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                                                "products_per_s": terms / (r1_ms * 1e-3)}
                cs.close(); del wv, abc, mats
            except Exception as ex:   # the front end is a "next" row of the scope table: its timing must not take the bench line down
                extras["r1cs_evaluate_2p20"] = {"error": repr(ex)[:200]}
            # G2 MSM at 2^20 (Fq2): 480 B algorithmic per pair
            g2 = pkg.synth_points(0, 2, 52, n)
            b2 = pkg.BaseSet(0, 2, g2)
            r2, e3, ph = timed(lambda: b2.msm(d_sc.data_ptr(), n=n, on_device=True, stream=stream), 3, 1)
            extras["g2_msm_2p20_ms"] = e3 / 3 * 1e3
            extras["g2_msm_points_per_s"] = n * 3 / e3
            extras["g2_parity_ok"] = bool(np.array_equal(pkg.point_to_affine(0, 2, r2), pkg.point_to_affine(0, 2, pkg.synth_expected_msm(0, 2, 52, sc))))
            ok = ok and extras["g2_parity_ok"]
            # The sizes an N-way split of the benchmark configurations produces (multiexp.tcc:417-431 on N devices), on ONE GPU: what
            # the first multi-GPU run should be held against.  Prefixes of the benchmark arrays (the generators are index-wise),
            # each checked through its discrete logs.
            def msm_ms(curve, group, seed_p, seed_s, pts_a, sc_a):
                k = len(pts_a)
                bs = pkg.BaseSet(curve, group, pts_a)
                d = torch.from_numpy(sc_a.copy().view(np.int64)).to(device)
                best = None
                for rep in range(3):
                    res = bs.msm(d.data_ptr(), n=k, on_device=True, stream=stream)
                    t = pkg.msm_last_timing()["total_ms"]
                    best = t if rep and (best is None or t < best) else (best if rep else None)
                good = bool(np.array_equal(pkg.point_to_affine(curve, group, res), pkg.point_to_affine(curve, group, pkg.synth_expected_msm(curve, group, seed_p, sc_a))))
                lv = pkg.msm_last_plan()["pair_levels"] + pkg.msm_last_plan().get("irr_levels", 0)
                bs.close(); del d
                return best, lv, good
            sweep, sweep_ok = {}, True
            for shift in (0, 1, 2, 3):
                k = n >> shift
                for group, arr, seed_p in ((1, pts, 42), (2, g2, 52)):
                    t, lv, good = msm_ms(0, group, seed_p, 43, arr[:k], sc[:k])
                    sweep[f"MNT4753_G{group}_2p{args.log_n - shift}"] = {"ms": round(t, 3), "pair_levels": lv}
                    sweep_ok = sweep_ok and good
            n6 = 1 << 15
            p61, p62, s6 = pkg.synth_points(1, 1, 42, n6), pkg.synth_points(1, 2, 52, n6), pkg.synth_scalars(1, 43, n6)
            for shift in (0, 1, 2, 3):
                k = n6 >> shift
                for group, arr, seed_p in ((1, p61, 42), (2, p62, 52)):
                    t, lv, good = msm_ms(1, group, seed_p, 43, arr[:k], s6[:k])
                    sweep[f"MNT6753_G{group}_2p{15 - shift}"] = {"ms": round(t, 3), "pair_levels": lv}
                    sweep_ok = sweep_ok and good
            # the one MSM for C = Ht + Lt + r Bt1 over the concatenated set H | L | B1 (B::groth16_C): 3 x the points of a slice
            for curve, name, base_n, seed_p in ((0, "MNT4753", n, 42), (1, "MNT6753", n6, 42)):
                p3 = pkg.synth_points(curve, 1, seed_p, 3 * base_n)
                s3 = pkg.synth_scalars(curve, 43, 3 * base_n)
                for shift in (0, 1, 2, 3):
                    k = (3 * base_n) >> shift
                    t, lv, good = msm_ms(curve, 1, seed_p, 43, p3[:k], s3[:k])
                    sweep[f"{name}_G1_3x2p{(args.log_n if curve == 0 else 15) - shift}"] = {"ms": round(t, 3), "pair_levels": lv}
                    sweep_ok = sweep_ok and good
                del p3, s3
            # predicted prove time on N devices (re-derived in round 4 from pieces measured in THIS run on one GPU):
            #   work bound  : device 0 runs its slices of the G2 MSM, of A's MSM and of the MSM for C back to back (the point kernels own
            #                 the whole chip: concurrency only fills launch gaps) plus its share of compute_H -- all of it
            #                 at N = 1; from N = 2 on one chain (two with two devices) and the joining step -- plus the O(1) host tail;
            #   chain bound : what must happen in sequence before device 0's slice of C can start -- its range of w and ca over ITS PCIe
            #                 link (measured: input_load_112MB_ms scaled by bytes), its chain, the arrival of the transformed cb / cc over
            #                 xGMI (ASSUMED 2.0 ms for 100 MB, ~50 GB/s on one link: no multi-GPU hardware was available), the joining
            #                 step -- then the slice of C.
            # The prediction is the larger of the two.  MNT6753 with its own compute_H share (2^15: 0.3 ms).
            pred = {}
            chain_ms, finish_ms = extras.get("compute_h_chain_2p20_ms", extras["compute_h_2p20_ms"] * 2 / 7), extras.get("compute_h_finish_2p20_ms", extras["compute_h_2p20_ms"] / 7)
            ld = extras.get("input_load_112MB_ms", {})
            load_ms_per_mb = (ld["best"] / (ld["bytes"] / 1e6)) if isinstance(ld, dict) and "best" in ld else 12.0 / 403.0
            XGMI_100MB_MS = 2.0
            for N, shift in ((1, 0), (2, 1), (4, 2), (8, 3)):
                g1 = sweep[f"MNT4753_G1_2p{args.log_n - shift}"]["ms"]; gg2 = sweep[f"MNT4753_G2_2p{args.log_n - shift}"]["ms"]
                gc = sweep[f"MNT4753_G1_3x2p{args.log_n - shift}"]["ms"]
                h_dev0 = extras["compute_h_2p20_ms"] if N == 1 else (chain_ms * (2 if N == 2 else 1) + finish_ms)
                work = gg2 + g1 + gc + h_dev0 + 2.5
                in_mb = 403.0 if N == 1 else (100.7 / N + 100.7 * (2 if N == 2 else 1))
                chain = in_mb * load_ms_per_mb + (extras["compute_h_2p20_ms"] if N == 1 else chain_ms * (2 if N == 2 else 1) + XGMI_100MB_MS + finish_ms) + gc + 2.5
                pred[f"MNT4753_2p20_{N}gpu_s"] = round(max(work, chain) * 1e-3, 4)
                pred[f"MNT4753_2p20_{N}gpu_bounds_ms"] = {"work_on_device_0": round(work, 2), "chain_to_C": round(chain, 2)}
                h1 = sweep[f"MNT6753_G1_2p{15 - shift}"]["ms"]; h2 = sweep[f"MNT6753_G2_2p{15 - shift}"]["ms"]
                hc = sweep[f"MNT6753_G1_3x2p{15 - shift}"]["ms"]
                pred[f"MNT6753_2p15_{N}gpu_s"] = round((h2 + h1 + hc + 0.3 + 2.5) * 1e-3, 4)
            extras["slice_sweep_ms"] = sweep
            extras["slice_sweep_parity_ok"] = sweep_ok
            extras["predicted_prove_s"] = dict(pred, model="max(work bound, chain bound) per N -- work: G2 MSM + G1 MSM (A) + G1 MSM over 3 x the points (C over H_g | L_g | B1_g) of "
                                                     "one slice + device 0's share of compute_H (all of it at N = 1; one chain + the joining step from N = 3, two chains at "
                                                     "N = 2) + 2.5 ms host tail; chain: device 0's input over its own PCIe link + its chain + the transformed cb / cc over "
                                                     "xGMI (ASSUMED 2.0 ms) + joining step + the slice of C.  Every piece but the xGMI copy measured on ONE GPU in this run; "
                                                     "multi-GPU hardware was not available to the builder -- the curve itself is unmeasured")
            ok = ok and sweep_ok
            b2.close(); del g2
            line["extras"] = extras
        else:
            bases.close()
        del d_sc
        torch.cuda.empty_cache()
        if legs is not None:
            line.update(legs)
            ok = ok and bool(legs["prove"].get("parity_ok")) and bool(legs["prove_mnt6753"].get("parity_ok"))
            for c in legs["cpu_prove"]:
                if c.get("same_bytes_as_gpu") is False:
                    ok = False
    elif rank == 0 and legs is not None:
        line.update(legs)
        ok = ok and bool(legs["prove"].get("parity_ok")) and bool(legs["prove_mnt6753"].get("parity_ok"))
    if rank == 0:
        if args.full:
            line["parity_ok"] = ok
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0 and want_prove and os.path.exists(gate):
            os.remove(gate)
    if not ok:
        raise SystemExit("bench.py: PARITY FAILURE")


if __name__ == "__main__":
    main()
