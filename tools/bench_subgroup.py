#!/usr/bin/env python3
"""Times the subgroup test of G2 and prints ONE JSON line; the same object goes to
profiles/subgroup/bench_subgroup.json.

Per curve, inputs resident on the device, wall time of the call, best of --reps:
  * verify: mnt753_groth16_verify against mnt753_groth16_verify_ex with MNT753_VERIFY_CHECK_SUBGROUP at the batch sizes of
    tools/bench_pairing.py (1, one wave of lane groups per SIMD, --scale times that), the two back to back in one process.  The
    unflagged call runs the kernel instantiation whose resource report equals the one of the commit before the flag existed;
  * check: mnt753_check_subgroup on G2 at n = 1, one full chip of lane groups and 2^20 (MNT4753) / 2^15 (MNT6753), beside
    mnt753_pairing at the same n.
Every batch is checked: all proofs accepted, no point reported.  Run each invocation under a time limit of its own
(`timeout -k 10 600 python tools/bench_subgroup.py`); it starts no threads of its own.

    python tools/bench_subgroup.py [--reps 3] [--scale 4]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from bench_pairing import GROUPS_PER_WAVE, NAME, NP, best_of, key_and_proofs  # noqa: E402

LARGE = {0: 1 << 20, 1: 1 << 15}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=int, default=4)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    pkg.init(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "verify": [], "check": []}
    for curve in (0, 1):
        full = cus * 4 * GROUPS_PER_WAVE[curve]
        vk, proofs, inp = key_and_proofs(pkg, curve)
        for n in (1, full, args.scale * full):
            idx = np.arange(n) % NP
            dp, di = pkg.DeviceBuffer.from_numpy(proofs[idx]), pkg.DeviceBuffer.from_numpy(np.tile(inp, (n, 1)))
            verdicts = []
            t_off = best_of(pkg, args.reps, lambda: verdicts.append(vk.verify(dp.ptr.value, di.ptr.value, on_device=True, n=n)))
            t_on = best_of(pkg, args.reps, lambda: verdicts.append(vk.verify(dp.ptr.value, di.ptr.value, on_device=True, n=n, check_subgroup=True)))
            if any(v.any() for v in verdicts):
                raise SystemExit(f"bench_subgroup: a valid proof was not accepted (curve {curve}, n {n})")
            res["verify"].append({"curve": NAME[curve], "n": n, "verify_s": round(t_off, 4), "proofs_per_s": round(n / t_off, 1),
                                  "verify_subgroup_s": round(t_on, 4), "proofs_per_s_subgroup": round(n / t_on, 1),
                                  "ratio": round(t_on / t_off, 4)})
        vk.close()
        g1, g2 = pkg.synth_points(curve, 1, 71, NP), pkg.synth_points(curve, 2, 72, NP)
        wt = pkg.gt_words(curve)
        for n in (1, full, LARGE[curve]):
            idx = np.arange(n) % NP
            d1, d2 = pkg.DeviceBuffer.from_numpy(g1[idx]), pkg.DeviceBuffer.from_numpy(g2[idx])
            dout = pkg.DeviceBuffer(8 * wt * n)
            reports = []
            t_chk = best_of(pkg, args.reps, lambda: reports.append(pkg.check_subgroup(curve, 2, d2.ptr.value, on_device=True, n=n)))
            if any(r != (0, 0, 0) for r in reports):
                raise SystemExit(f"bench_subgroup: a point of G2 was reported (curve {curve}, n {n}): {reports}")
            t_pair = best_of(pkg, args.reps, lambda: pkg.pairing(curve, d1.ptr.value, d2.ptr.value, on_device=True, n=n, out=dout.ptr.value))
            res["check"].append({"curve": NAME[curve], "n": n, "check_subgroup_s": round(t_chk, 4), "points_per_s": round(n / t_chk, 1),
                                 "pairing_s": round(t_pair, 4), "pairings_per_s": round(n / t_pair, 1), "pairings_per_point": round(t_chk / t_pair, 4)})
    line = json.dumps(res)
    out_dir = os.path.join(ROOT, "profiles", "subgroup")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_subgroup.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
