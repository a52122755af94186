#!/usr/bin/env python3
"""Times the batch pairing (mnt753_pairing) and batch Groth16 verification (mnt753_groth16_verify) and prints ONE JSON line; the same
object goes to profiles/pairing/bench_pairing.json.

Per curve, at n = 1, at the n that gives every SIMD of the chip one wave of lane groups (CUs x 4 x 32 on MNT4753, x 21 on MNT6753) and at
four times that: the wall time of the call with inputs resident on the device (best of --reps), pairings / proofs per second, and the
bytes of device workspace the call allocates beside its inputs and outputs.  Every batch cycles 7 distinct pairs (the proofs: the
fixture's proof re-randomised as A' = rho A, B' = B / rho) and is checked: equal inputs give equal outputs, every proof is accepted,
and output 0 equals the single call's.

For context only: the wall time of the reference's verifier for ONE proof (oracle/_ref/ref_groth16 verify, where that build exists).
It is a whole process: start, init_public_params and reading the key are in it -- the only reference figure there is without a new
reference binary; it is not a like-for-like kernel time.

    python tools/bench_pairing.py [--reps 3] [--scale 4]"""
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
from __graft_entry__ import load_package  # noqa: E402
import pyref  # noqa: E402

NAME = {0: "MNT4753", 1: "MNT6753"}
GROUPS_PER_WAVE = {0: 32, 1: 21}
NP = 7


def g16(curve, name):
    return os.path.join(ROOT, "tests", "golden", f"g16_mnt{4 if curve == 0 else 6}", name)


def key_and_proofs(pkg, curve):
    """the fixture's key (keys.bin, vk.txt) and NP valid proofs of its statement"""
    C = pyref.Curve(curve)
    w2 = pkg.affine_words(curve, 2)
    keys = np.fromfile(g16(curve, "keys.bin"), dtype="<u8").astype(np.uint64)
    raw = open(g16(curve, "vk.txt"), "rb").read()
    pos = 8 * w2 + 1 + 8 * w2
    abc = np.concatenate([np.frombuffer(raw[pos + 1:pos + 193], dtype="<u8"), np.frombuffer(raw[pos + 202:pos + 394], dtype="<u8")]).astype(np.uint64)
    vk = pkg.VerificationKey(curve, keys[:24], keys[48:48 + w2], keys[72 + w2:72 + 2 * w2], abc)
    proof = np.fromfile(g16(curve, "full.bin"), dtype="<u8").astype(np.uint64)
    inp = np.fromfile(g16(curve, "input.bin"), dtype="<u8", count=24).astype(np.uint64)[12:]
    rng = pyref.splitmix64(33 + curve)
    sw = lambda x: np.array(C.fr_to_words(x), dtype=np.uint64)
    scale = lambda g, x, p: pkg.point_to_affine(curve, g, pkg.point_scale(curve, g, sw(x), pkg.point_from_affine(curve, g, p)))
    proofs = [proof]
    for _ in range(NP - 1):
        rho = pyref.rand_below(rng, C.r - 1) + 1
        proofs.append(np.concatenate([scale(1, rho, proof[:24]), scale(2, pow(rho, -1, C.r), proof[24:24 + w2]), proof[24 + w2:]]))
    return vk, np.stack(proofs), inp


def best_of(pkg, reps, fn):
    best = 1e30
    for _ in range(reps):
        pkg.lib().mnt753_sync(None)
        t0 = time.perf_counter()
        fn()
        pkg.lib().mnt753_sync(None)
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=int, default=4, help="the largest batch, in units of one wave of lane groups per SIMD")
    args = ap.parse_args()
    import torch
    pkg = load_package()
    pkg.init(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "cases": []}
    for curve in (0, 1):
        full = cus * 4 * GROUPS_PER_WAVE[curve]
        g1, g2 = pkg.synth_points(curve, 1, 71, NP), pkg.synth_points(curve, 2, 72, NP)
        vk, proofs, inp = key_and_proofs(pkg, curve)
        wt = pkg.gt_words(curve)
        one_gt = pkg.pairing(curve, g1[0], g2[0])[0]
        for n in (1, full, args.scale * full):
            idx = np.arange(n) % NP
            d1, d2 = pkg.DeviceBuffer.from_numpy(g1[idx]), pkg.DeviceBuffer.from_numpy(g2[idx])
            dout = pkg.DeviceBuffer(8 * wt * n)
            t_pair = best_of(pkg, args.reps, lambda: pkg.pairing(curve, d1.ptr.value, d2.ptr.value, on_device=True, n=n, out=dout.ptr.value))
            out = dout.to_numpy().reshape(n, wt)
            if not np.array_equal(out[0], one_gt) or any(not np.array_equal(out[k], out[k % NP]) for k in (1 % n, n // 2, n - 1)):
                raise SystemExit(f"bench_pairing: outputs of equal inputs differ (curve {curve}, n {n})")
            dp, di = pkg.DeviceBuffer.from_numpy(proofs[idx]), pkg.DeviceBuffer.from_numpy(np.tile(inp, (n, 1)))
            verdicts = []
            t_ver = best_of(pkg, args.reps, lambda: verdicts.append(vk.verify(dp.ptr.value, di.ptr.value, on_device=True, n=n)))
            if any(v.any() for v in verdicts):
                raise SystemExit(f"bench_pairing: a valid proof was not accepted (curve {curve}, n {n})")
            chunk = min(n, 1 << 16)
            res["cases"].append({"curve": NAME[curve], "n": n, "pairing_s": round(t_pair, 4), "pairings_per_s": round(n / t_pair, 1),
                                 "verify_s": round(t_ver, 4), "proofs_per_s": round(n / t_ver, 1),
                                 "pairing_workspace_bytes": 8 * (24 + pkg.affine_words(curve, 2)) + 32,      # the stand-in pair, the check's record
                                 "verify_workspace_bytes": chunk * (192 + 96 * vk.num_inputs + 2)})             # points, integers, flags and verdicts
        vk.close()
        ref = os.path.join(ROOT, "oracle", "_ref", "ref_groth16")
        if os.access(ref, os.X_OK):
            t0 = time.perf_counter()
            r = subprocess.run([ref, "verify", NAME[curve], os.path.dirname(g16(curve, "vk.txt")), g16(curve, "full.bin")], capture_output=True, text=True)
            res.setdefault("reference_verifier_process_wall_s", {})[NAME[curve]] = {
                "seconds": round(time.perf_counter() - t0, 3), "verdict": r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "",
                "note": "one proof, one CPU process: start, init_public_params and key parsing included; context only"}
    line = json.dumps(res)
    out_dir = os.path.join(ROOT, "profiles", "pairing")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_pairing.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
