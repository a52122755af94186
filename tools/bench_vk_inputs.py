#!/usr/bin/env python3
"""Times the verifiers on keys with many public inputs, with and without the input tables (mnt753_vk_prepare_inputs, DESIGN.md
section 4.17), and prints ONE JSON line; the same object goes to profiles/vk_inputs/bench_vk_inputs.json.

Per curve, for k public inputs (--ks, default 1 4 16 64 256 1024) and n proofs (1, one wave of lane groups per SIMD, --scale times
that: section 4.12's sizes), best of --reps: the wall time of mnt753_vk_accumulate (host inputs, as the call takes them; left out
above --max-host-bytes of inputs, 1 GiB), of mnt753_groth16_verify_ex with the subgroup check and of mnt753_groth16_verify_folded, the latter two with
proofs and inputs resident on the device.  The keys are the g16 fixtures widened to k inputs (tests/vk_inputs_ref.py: ABC'_j = a_j
ABC_1, inputs that combine to the fixture's x), so every batch is accepted; a batch cycles 7 valid proofs and 64 distinct input rows.

Two sides, one process each per repetition, alternating in one session: `prepared`, this build with a prepared key -- which also
reports the build time and bytes of the tables and the walk / segment-sum split of the last chunk (HIP events) -- and `parent`, an
unprepared key on ANOTHER build of the library: --baseline-lib names the libmnt753_hip.so of the commit before the tables (without
it this build's unprepared path is timed, and the output says so).  --widths adds a sweep of the table width at k = 64.

    python tools/bench_vk_inputs.py [--reps 3] [--scale 4] [--ks K ...] [--baseline-lib PATH] [--widths W ...] [--max-parent-k K]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAME = {0: "MNT4753", 1: "MNT6753"}
GROUPS_PER_WAVE = {0: 32, 1: 21}
ROWS = 64
NEW_SYMBOLS = ("mnt753_vk_prepare_inputs", "mnt753_vk_input_plan", "mnt753_vk_release_inputs")


def timed(pkg, fn):
    pkg.lib().mnt753_sync(None)
    t0 = time.perf_counter()
    out = fn()
    pkg.lib().mnt753_sync(None)
    return time.perf_counter() - t0, out


def widened_key(pkg, curve, k, parts):
    """-> (key object, [ROWS, 12 k] input words, every row combining to the fixture's x)"""
    import pyref
    import vk_inputs_ref as VR
    C = pyref.Curve(curve)
    keys, abc, inp = parts
    w2 = pkg.affine_words(curve, 2)
    a = VR.ratios(C.r, k, 1000 * curve + k)
    fb = pkg.FixedBase(curve, 1, abc[24:])
    pts = fb.batch_exp(np.array([C.fr_to_words(v) for v in a], dtype=np.uint64))
    fb.close()
    vk = pkg.VerificationKey(curve, keys[:24], keys[48:48 + w2], keys[72 + w2:72 + 2 * w2], np.concatenate([abc[:24], pts.reshape(-1)]))
    x = C.fr_from_words([int(v) for v in inp])
    rng = pyref.splitmix64(5 + curve + k)
    rows = []
    for _ in range(ROWS):
        head = [pyref.rand_below(rng, C.r) for _ in range(k - 1)]
        rows.append(np.array([w for v in head + [VR.solve_last(C.r, a, head, x)] for w in C.fr_to_words(v)], dtype=np.uint64))
    return vk, np.stack(rows)


def worker(side, args):
    import torch
    from __graft_entry__ import load_package
    import bench_pairing as BP
    import pyref
    pkg = load_package()
    if side == "parent":
        pkg.api.OPTIONAL_SYMBOLS.update(NEW_SYMBOLS)                          # MNT753_LIB may name a build from before the calls existed
    pkg.init(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "cases": {}, "tables": {}, "widths": {}}
    for curve in (0, 1):
        full = cus * 4 * GROUPS_PER_WAVE[curve]
        ns = sorted({1, full, args.scale * full})
        base_vk, proofs, inp = BP.key_and_proofs(pkg, curve)
        base_vk.close()
        w2 = pkg.affine_words(curve, 2)
        keys = np.fromfile(BP.g16(curve, "keys.bin"), dtype="<u8").astype(np.uint64)
        raw = open(BP.g16(curve, "vk.txt"), "rb").read()
        pos = 8 * w2 + 1 + 8 * w2
        abc = np.concatenate([np.frombuffer(raw[pos + 1:pos + 193], dtype="<u8"), np.frombuffer(raw[pos + 202:pos + 394], dtype="<u8")]).astype(np.uint64)
        rng = pyref.splitmix64(77 + curve)
        dproofs = {n: torch.from_numpy(proofs.view(np.int64)).cuda().repeat((n + BP.NP - 1) // BP.NP, 1)[:n].contiguous() for n in ns}
        for k in args.ks:
            if side == "parent" and k > args.max_parent_k:
                continue
            vk, rows = widened_key(pkg, curve, k, (keys, abc, inp))
            if side == "prepared":
                t, plan = timed(pkg, lambda: vk.prepare_inputs())
                res["tables"][f"{curve}:{k}"] = {"prepare_s": t, "build_ms": vk.test_inputs_last_timing()[2], "window_bits": plan["window_bits"],
                                                 "windows": plan["windows"], "table_bytes": plan["table_bytes"]}
            drows = torch.from_numpy(rows.view(np.int64)).cuda()
            for n in ns:
                di = drows.repeat((n + ROWS - 1) // ROWS, 1)[:n].contiguous()
                dp = dproofs[n]
                coef = np.array([rng() | 1 for _ in range(2 * n)], dtype=np.uint64).reshape(n, 2)
                case = {}
                if side == "prepared":
                    case["inputs_per_lane"] = vk.input_plan(min(n, 1 << 16))["inputs_per_lane"]
                if 96 * k * n <= args.max_host_bytes:
                    host = np.tile(rows, ((n + ROWS - 1) // ROWS, 1))[:n].reshape(n, k, 12)
                    if n == 1:
                        vk.accumulate(host)                                  # a first call outside the timing: code objects
                    case["accumulate_s"], _ = timed(pkg, lambda: vk.accumulate(host))
                    if side == "prepared":
                        case["accumulate_walk_ms"], case["accumulate_sum_ms"] = vk.test_inputs_last_timing()[:2]
                    del host
                if n == 1:
                    vk.verify(dp.data_ptr(), di.data_ptr(), on_device=True, n=n, check_subgroup=True)
                    vk.verify_folded(dp.data_ptr(), di.data_ptr(), coef, on_device=True, n=n)
                case["verify_ex_s"], verdicts = timed(pkg, lambda: vk.verify(dp.data_ptr(), di.data_ptr(), on_device=True, n=n, check_subgroup=True))
                if side == "prepared":
                    case["verify_walk_ms"], case["verify_sum_ms"] = vk.test_inputs_last_timing()[:2]
                case["verify_folded_s"], (accepted, status) = timed(pkg, lambda: vk.verify_folded(dp.data_ptr(), di.data_ptr(), coef, on_device=True, n=n))
                if verdicts.any() or not accepted or status.any():
                    raise SystemExit(f"bench_vk_inputs: a valid batch was not accepted ({side}, curve {curve}, k {k}, n {n})")
                res["cases"][f"{curve}:{k}:{n}"] = case
                print(f"[{side}] {NAME[curve]} k={k} n={n}: {case}", file=sys.stderr, flush=True)
                del di
            if side == "prepared" and k == 64 and args.widths:
                n = ns[1]
                host = np.tile(rows, ((n + ROWS - 1) // ROWS, 1))[:n].reshape(n, k, 12)
                for w in args.widths:
                    t, plan = timed(pkg, lambda: vk.prepare_inputs(window_bits=w, max_table_bytes=8 << 30))   # (wider than the default cap allows: the sweep asks)
                    vk.accumulate(host)
                    walk, ssum, build = vk.test_inputs_last_timing()
                    res["widths"][f"{curve}:{w}"] = {"n": n, "build_ms": build, "table_bytes": plan["table_bytes"], "walk_ms": walk, "sum_ms": ssum}
            vk.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=int, default=4, help="the largest batch, in units of one wave of lane groups per SIMD")
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 4, 16, 64, 256, 1024])
    ap.add_argument("--widths", type=int, nargs="*", default=[4, 6, 8, 10, 12])
    ap.add_argument("--max-parent-k", type=int, default=1 << 20, help="the parent side skips keys with more inputs (measured: 22-43 ms per input and chunk)")
    ap.add_argument("--max-host-bytes", type=int, default=1 << 30, help="mnt753_vk_accumulate (host inputs) is left out above this many bytes of inputs")
    ap.add_argument("--baseline-lib", default=None, help="libmnt753_hip.so of the commit before the input tables, for the parent side")
    ap.add_argument("--worker", choices=["prepared", "parent"], default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args)
    runs = {"prepared": [], "parent": []}
    for _ in range(args.reps):
        for side in ("parent", "prepared"):
            env = dict(os.environ)
            if side == "parent" and args.baseline_lib:
                env["MNT753_LIB"] = os.path.abspath(args.baseline_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", side, "--scale", str(args.scale), "--max-parent-k", str(args.max_parent_k),
                   "--max-host-bytes", str(args.max_host_bytes), "--ks"] + [str(k) for k in args.ks] + ["--widths"] + [str(w) for w in args.widths]
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=1100)      # (stderr passes through: the progress lines)
            if r.returncode != 0:
                raise SystemExit(f"bench_vk_inputs: the {side} process failed:\n{r.stdout[-3000:]}")
            runs[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
    head = runs["prepared"][0]
    res = {"device": head["device"], "compute_units": head["compute_units"], "reps": args.reps,
           "command": "python tools/bench_vk_inputs.py " + " ".join(sys.argv[1:]),
           "parent_library": "the commit before the input tables (--baseline-lib)" if args.baseline_lib else "this build, key not prepared (no --baseline-lib given)",
           "cases": [], "tables": [], "width_sweep_k64": []}
    calls = ("accumulate_s", "verify_ex_s", "verify_folded_s")
    order = lambda s: tuple(int(v) for v in s.split(":"))
    for key in sorted(head["cases"], key=order):
        curve, k, n = order(key)
        case = {"curve": NAME[curve], "k": k, "n": n, "inputs_per_lane": head["cases"][key].get("inputs_per_lane")}
        for call in calls:
            for side in ("prepared", "parent"):
                vals = [r["cases"][key][call] for r in runs[side] if key in r["cases"] and call in r["cases"][key]]
                if vals:
                    case[f"{side}_{call}"] = round(min(vals), 5)
                    case[f"{side}_{call}_spread"] = round(max(vals) - min(vals), 5)
            if f"prepared_{call}" in case and f"parent_{call}" in case:
                case[f"speedup_{call[:-2]}"] = round(case[f"parent_{call}"] / case[f"prepared_{call}"], 3)
        for ms in ("accumulate_walk_ms", "accumulate_sum_ms", "verify_walk_ms", "verify_sum_ms"):
            vals = [r["cases"][key][ms] for r in runs["prepared"] if ms in r["cases"][key]]
            if vals:
                case[ms] = round(min(vals), 3)
        res["cases"].append(case)
    for key in sorted(head["tables"], key=order):
        curve, k = order(key)
        t = dict(head["tables"][key])
        t["prepare_s"] = round(min(r["tables"][key]["prepare_s"] for r in runs["prepared"]), 5)
        t["build_ms"] = round(min(r["tables"][key]["build_ms"] for r in runs["prepared"]), 3)
        res["tables"].append({"curve": NAME[curve], "k": k, **t})
    for key in sorted(head["widths"], key=order):
        curve, w = order(key)
        t = {f: round(min(r["widths"][key][f] for r in runs["prepared"]), 3) for f in ("build_ms", "walk_ms", "sum_ms")}
        res["width_sweep_k64"].append({"curve": NAME[curve], "window_bits": w, "n": head["widths"][key]["n"], "table_bytes": head["widths"][key]["table_bytes"], **t})
    line = json.dumps(res)
    out_dir = os.path.join(ROOT, "profiles", "vk_inputs")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_vk_inputs.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
