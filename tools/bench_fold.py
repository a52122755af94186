#!/usr/bin/env python3
"""Times the folded Groth16 verification (mnt753_groth16_verify_folded) against the per-proof verifier with the
subgroup check (mnt753_groth16_verify_ex with MNT753_VERIFY_CHECK_SUBGROUP) and prints ONE JSON line; the same object goes to
profiles/fold/bench_fold.json.

Per curve, at n = 1, at the n that gives every SIMD of the chip one wave of lane groups (CUs x 4 x 32 on MNT4753, x 21 on MNT6753) and
at four times that (section 4.12's sizes): the wall time of the call with proofs and inputs resident on the device, best of --reps,
and for the fold the split of its device time into scale, Miller-and-fold and tail (HIP events inside the call).  Every batch cycles
the 7 valid proofs of tools/bench_pairing.py and must be accepted.

The per-proof side runs in a process of its own, so that it can come from ANOTHER build of the library: --baseline-lib names the
libmnt753_hip.so of the commit before the fold (without it the current build's verify_ex is timed, and the output says so).  The two
sides alternate, one process each per repetition, in one session.  --extra adds sizes (per curve, as multiples of a wave of lane
groups, e.g. 64 256 1024) to place the smallest n at which the fold is faster.

    python tools/bench_fold.py [--reps 3] [--scale 4] [--baseline-lib PATH] [--extra K ...]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAME = {0: "MNT4753", 1: "MNT6753"}
GROUPS_PER_WAVE = {0: 32, 1: 21}


def sizes(cus, scale, extra):
    out = {}
    for curve in (0, 1):
        full = cus * 4 * GROUPS_PER_WAVE[curve]
        out[curve] = sorted({1, full, scale * full} | {k * GROUPS_PER_WAVE[curve] for k in extra})
    return out


def worker(side, scale, extra):
    """one process: every (curve, n) once; prints {"curve:n": {"s": wall seconds, ...}}"""
    import torch
    from __graft_entry__ import load_package
    import bench_pairing as BP
    import pyref
    pkg = load_package()
    if side == "per_proof":
        pkg.api.OPTIONAL_SYMBOLS.add("mnt753_groth16_verify_folded")       # MNT753_LIB may name a build from before the call existed
    pkg.init(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "cases": {}}
    for curve, ns in sizes(cus, scale, extra).items():
        vk, proofs, inp = BP.key_and_proofs(pkg, curve)
        rng = pyref.splitmix64(77 + curve)
        for n in ns:
            idx = np.arange(n) % BP.NP
            dp, di = pkg.DeviceBuffer.from_numpy(proofs[idx]), pkg.DeviceBuffer.from_numpy(np.tile(inp, (n, 1)))
            coef = np.array([rng() | 1 for _ in range(2 * n)], dtype=np.uint64).reshape(n, 2)
            if n == ns[0]:                                                   # a first call outside the timing: code objects, the reduction's workspace
                vk.verify_folded(dp.ptr.value, di.ptr.value, coef, on_device=True, n=n) if side == "fold" else \
                    vk.verify(dp.ptr.value, di.ptr.value, on_device=True, n=n, check_subgroup=True)
            pkg.lib().mnt753_sync(None)
            t0 = time.perf_counter()
            if side == "fold":
                accepted, status = vk.verify_folded(dp.ptr.value, di.ptr.value, coef, on_device=True, n=n)
            else:
                status = vk.verify(dp.ptr.value, di.ptr.value, on_device=True, n=n, check_subgroup=True)
                accepted = True
            pkg.lib().mnt753_sync(None)
            case = {"s": time.perf_counter() - t0}
            if not accepted or status.any():
                raise SystemExit(f"bench_fold: a valid batch was not accepted ({side}, curve {curve}, n {n})")
            if side == "fold":
                case["stage_ms"] = pkg.api.test_fold_last_timing()
            res["cases"][f"{curve}:{n}"] = case
        vk.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=int, default=4, help="the largest batch, in units of one wave of lane groups per SIMD")
    ap.add_argument("--baseline-lib", default=None, help="libmnt753_hip.so of the commit before the fold, for the per-proof side")
    ap.add_argument("--extra", type=int, nargs="*", default=[], help="further sizes, in waves of lane groups")
    ap.add_argument("--worker", choices=["fold", "per_proof"], default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.scale, args.extra)
    best = {"fold": {}, "per_proof": {}}
    head = {}
    for _ in range(args.reps):
        for side in ("per_proof", "fold"):
            env = dict(os.environ)
            if side == "per_proof" and args.baseline_lib:
                env["MNT753_LIB"] = os.path.abspath(args.baseline_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", side, "--scale", str(args.scale), "--extra"] + [str(k) for k in args.extra]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"bench_fold: the {side} process failed:\n{r.stdout}\n{r.stderr}")
            out = json.loads(r.stdout.strip().splitlines()[-1])
            head = {"device": out["device"], "compute_units": out["compute_units"]}
            for k, case in out["cases"].items():
                if k not in best[side] or case["s"] < best[side][k]["s"]:
                    best[side][k] = case
    res = dict(head)
    res["per_proof_library"] = "the commit before the fold (--baseline-lib)" if args.baseline_lib else "this build (no --baseline-lib given)"
    res["reps"] = args.reps
    res["cases"] = []
    for k in sorted(best["fold"], key=lambda s: (int(s.split(":")[0]), int(s.split(":")[1]))):
        curve, n = (int(v) for v in k.split(":"))
        f, p = best["fold"][k], best["per_proof"][k]
        res["cases"].append({"curve": NAME[curve], "n": n, "per_proof_check_subgroup_s": round(p["s"], 4), "folded_s": round(f["s"], 4),
                             "speedup": round(p["s"] / f["s"], 3), "folded_proofs_per_s": round(n / f["s"], 1),
                             "folded_stage_ms": {"scale": round(f["stage_ms"][0], 2), "miller_and_fold": round(f["stage_ms"][1], 2),
                                                 "tail": round(f["stage_ms"][2], 2)}})
    for curve in (0, 1):
        faster = [c["n"] for c in res["cases"] if c["curve"] == NAME[curve] and c["speedup"] > 1.0]
        res.setdefault("smallest_measured_n_where_the_fold_is_faster", {})[NAME[curve]] = min(faster) if faster else None
    line = json.dumps(res)
    out_dir = os.path.join(ROOT, "profiles", "fold")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_fold.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
