#!/usr/bin/env python3
"""Times the folded Groth16 verification with one tail per segment (mnt753_groth16_verify_folded_locate)
against what a caller had before it, and prints ONE JSON line; the same object goes to profiles/fold_locate/bench_fold_locate.json.

Per curve, at bench_fold's sizes -- n = 1, the n that gives every SIMD of the chip one wave of lane groups (CUs x 4 x 32 on MNT4753,
x 21 on MNT6753) and four times that -- with proofs and inputs resident on the device, wall time of the call(s), best of --reps and
the spread (worst / best - 1) of each side:
  accepted      a valid batch: the new call against mnt753_groth16_verify_folded
  rejected_one  one C := A proof in the middle: the new call against what verify(.., fold=True) does, mnt753_groth16_verify_folded
                followed by mnt753_groth16_verify_ex with the subgroup check
  every_16th    (largest n only) one C := A proof in every 16th segment: the same comparison, and proofs_rechecked
The new call reports its four stage times (scale, Miller, tails, recheck).

The baseline side runs in a process of its own, so that it can come from ANOTHER build of the library: --baseline-lib names the
libmnt753_hip.so of the commit before this call (without it the current build's fold and verify_ex are timed, and the output says
so).  The two sides alternate, one process each per repetition, in one session.

    python tools/bench_fold_locate.py [--reps 3] [--scale 4] [--baseline-lib PATH]"""
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
SEGMENT = {0: 128, 1: 84}
NEW = ("mnt753_fold_segment_proofs", "mnt753_groth16_verify_folded_locate")


def sizes(cus, scale):
    return {curve: sorted({1, cus * 4 * GROUPS_PER_WAVE[curve], scale * cus * 4 * GROUPS_PER_WAVE[curve]}) for curve in (0, 1)}


def batches(curve, n, largest):
    """-> [(name, indices of the C := A proofs)]"""
    out = [("accepted", []), ("rejected_one", [n // 2])]
    if largest:
        g = SEGMENT[curve]
        out.append(("every_16th", [s * g + g // 2 for s in range(0, n // g, 16)]))
    return out


def worker(side, scale):
    """one process: every (curve, n, batch) once; prints {"curve:n:batch": {"s": wall seconds, ...}}"""
    import torch
    from __graft_entry__ import load_package
    import bench_pairing as BP
    import pyref
    pkg = load_package()
    if side == "baseline":
        pkg.api.OPTIONAL_SYMBOLS.update(NEW)                                 # MNT753_LIB may name a build from before the call existed
    pkg.init(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "cases": {}}
    sync = lambda: pkg.lib().mnt753_sync(None)
    for curve, ns in sizes(cus, scale).items():
        vk, pool, inp = BP.key_and_proofs(pkg, curve)
        w2 = pkg.affine_words(curve, 2)
        rng = pyref.splitmix64(77 + curve)
        for n in ns:
            good = pool[np.arange(n) % BP.NP]
            di = pkg.DeviceBuffer.from_numpy(np.tile(inp, (n, 1)))
            coef = np.array([rng() | 1 for _ in range(2 * n)], dtype=np.uint64).reshape(n, 2)
            for name, bad in batches(curve, n, n == ns[-1] and n > 1):
                proofs = good.copy()
                for i in bad:
                    proofs[i, 24 + w2:] = proofs[i, :24]
                dp = pkg.DeviceBuffer.from_numpy(proofs)
                args = (dp.ptr.value, di.ptr.value)
                if n == ns[0] and name == "accepted":                        # a first call outside the timing: code objects, workspaces
                    if side == "locate":
                        vk.verify_folded_locate(*args, coef, on_device=True, n=n)
                    else:
                        vk.verify_folded(*args, coef, on_device=True, n=n)
                        vk.verify(*args, on_device=True, n=n, check_subgroup=True)
                sync()
                t0 = time.perf_counter()
                if side == "locate":
                    verdicts, rep = vk.verify_folded_locate(*args, coef, on_device=True, n=n)
                    sync()
                    case = {"s": time.perf_counter() - t0, "report": rep}
                else:
                    accepted, verdicts = vk.verify_folded(*args, coef, on_device=True, n=n)
                    sync()
                    case = {"fold_s": time.perf_counter() - t0}
                    if not accepted:                                         # what verify(.., fold=True) does next
                        verdicts = vk.verify(*args, on_device=True, n=n, check_subgroup=True)
                        sync()
                    case["s"] = time.perf_counter() - t0
                if sorted(np.flatnonzero(verdicts)) != sorted(bad) or any(verdicts[i] != 2 for i in bad):
                    raise SystemExit(f"bench_fold_locate: wrong verdicts ({side}, curve {curve}, n {n}, {name})")
                res["cases"][f"{curve}:{n}:{name}"] = case
        vk.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=int, default=4, help="the largest batch, in units of one wave of lane groups per SIMD")
    ap.add_argument("--baseline-lib", default=None, help="libmnt753_hip.so of the commit before this call, for the baseline side")
    ap.add_argument("--worker", choices=["locate", "baseline"], default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.scale)
    runs = {"locate": {}, "baseline": {}}
    head = {}
    for _ in range(args.reps):
        for side in ("baseline", "locate"):
            env = dict(os.environ)
            if side == "baseline" and args.baseline_lib:
                env["MNT753_LIB"] = os.path.abspath(args.baseline_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", side, "--scale", str(args.scale)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"bench_fold_locate: the {side} process failed:\n{r.stdout}\n{r.stderr}")
            out = json.loads(r.stdout.strip().splitlines()[-1])
            head = {"device": out["device"], "compute_units": out["compute_units"]}
            for k, case in out["cases"].items():
                runs[side].setdefault(k, []).append(case)
    res = dict(head)
    res["baseline_library"] = "the commit before this call (--baseline-lib)" if args.baseline_lib else "this build (no --baseline-lib given)"
    res["baseline"] = "accepted: mnt753_groth16_verify_folded; rejected: mnt753_groth16_verify_folded + mnt753_groth16_verify_ex(check_subgroup)"
    res["reps"] = args.reps
    res["cases"] = []
    order = lambda s: (int(s.split(":")[0]), int(s.split(":")[1]), s.split(":")[2])
    for k in sorted(runs["locate"], key=order):
        curve, n, name = k.split(":")
        loc, base = runs["locate"][k], runs["baseline"][k]
        lb, bb = min(loc, key=lambda c: c["s"]), min(base, key=lambda c: c["s"])
        spread = lambda cs: round(max(c["s"] for c in cs) / min(c["s"] for c in cs) - 1.0, 4)
        rep = lb["report"]
        res["cases"].append({"curve": NAME[int(curve)], "n": int(n), "batch": name, "locate_s": round(lb["s"], 4), "baseline_s": round(bb["s"], 4),
                             "baseline_fold_s": round(bb["fold_s"], 4), "baseline_over_locate": round(bb["s"] / lb["s"], 3),
                             "locate_spread": spread(loc), "baseline_spread": spread(base),
                             "segments": rep["segments"], "segments_rejected": rep["segments_rejected"], "proofs_rechecked": rep["proofs_rechecked"],
                             "locate_stage_ms": {f: round(rep["ms_" + f], 2) for f in ("scale", "miller", "tails", "recheck")}})
    line = json.dumps(res)
    out_dir = os.path.join(ROOT, "profiles", "fold_locate")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_fold_locate.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
