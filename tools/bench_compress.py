#!/usr/bin/env python3
"""Times the compressed points and prints ONE JSON line; the same object goes to
profiles/compress/bench_compress.json.

Inputs resident on the device; every figure is HIP-event time (torch.cuda.Event around the call on the null stream, which the library's
launches use; the square-root hook brackets its kernel itself), after --warmup untimed calls, --reps repetitions, min and median:
  * sqrt: the square-root kernel alone per coordinate field and window W = 1, 2, 4 of the fixed exponent (the test hook
    mnt753_test_field_sqrt_window) on squares, one chip's worth of lanes / lane groups (4 waves per SIMD), with the operation count
    beside it: field products per root from the exponent's bits and (s - 1)(s - 2) / 2, the same in base-field products (a lane-split
    Fq2 product is 4 of them, an Fq3 product 9), and the achieved base-field products per second as a fraction of bench.py's
    MODMUL_PEAK_PER_S, the denominator of its modmul_frac;
  * points: mnt753_decompress_points and mnt753_compress_points per (curve, group) at n = 2^16;
  * verify: mnt753_groth16_verify_compressed next to mnt753_groth16_verify on the same proofs in the same run, one chip's worth of
    lane groups; `decompress_share` is the ratio (compressed - plain) / compressed of those two.
Every result is checked: all roots are roots, all points come back, all proofs are accepted.  Run under a time limit of its own
(`timeout -k 10 600 python tools/bench_compress.py`); it starts no threads of its own.

    python tools/bench_compress.py [--reps 5] [--warmup 1]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from bench_pairing import GROUPS_PER_WAVE, NAME, NP, key_and_proofs  # noqa: E402
import gen_constants as GC  # noqa: E402
import mnt753_params as P  # noqa: E402
import pyref  # noqa: E402

MODMUL_PEAK_PER_S = 22.0e9      # bench.py: the measured chip peak of the 753-bit Montgomery multiplier
N_POINTS = 1 << 16
WINDOWS = (1, 2, 4)
FIELDS = [(0, 1, P.MOD_B, 0, 1), (1, 1, P.MOD_A, 0, 1), (0, 2, P.MOD_B, 13, 4), (1, 3, P.MOD_A, 11, 9)]   # curve, deg, q, nr, base products per product


def operation_count(q, deg, nr, window):
    """(squarings, products) of one square root of csrc/fp_sqrt.hip.h: the windowed power a^((t - 1) / 2), x = a w, b = x w, the
    fixed loop ((s - 1)(s - 2) / 2 squarings of the tests, s - 1 of c, 2 (s - 1) products) and the closing x^2"""
    c = GC.sqrt_constants(q, deg, nr)
    s, e = c["s"], c["e"]
    bits = e.bit_length()
    if window == 1:
        sq, mul = bits - 1, bin(e).count("1") - 1
    else:
        nwin = (bits + window - 1) // window
        digits = [(e >> (window * k)) & ((1 << window) - 1) for k in range(nwin)]
        sq, mul = window * (nwin - 1), (1 << window) - 2 + sum(1 for d in digits[:-1] if d)
    return sq + (s - 1) * (s - 2) // 2 + (s - 1) + 1, mul + 2 + 2 * (s - 1)


def timed(torch, reps, warmup, fn):
    """[milliseconds] of `reps` calls of fn, HIP events on the null stream"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms, n):
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "per_s": round(n / (min(ms) * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    pkg.init(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "reps": args.reps, "warmup": args.warmup,
           "modmul_peak_per_s": MODMUL_PEAK_PER_S, "sqrt": [], "points": [], "verify": []}
    # ---- the square-root kernel per field and window ----
    for curve, deg, q, nr, base in FIELDS:
        C = pyref.Curve(curve)
        lanes = 64 if deg == 1 else GROUPS_PER_WAVE[curve]
        n = cus * 4 * 4 * lanes
        rng = pyref.splitmix64(41 + curve + deg)
        pool = []
        for _ in range(16):                                                # squares u^2 of random u
            u = [pyref.rand_below(rng, q) for _ in range(deg)]
            u = u[0] if deg == 1 else tuple(u)
            pool.append(C.coord_to_words(C.f_mul(u, u)))
        words = np.array(pool, dtype=np.uint64)[np.arange(n) % 16]
        for w in WINDOWS:
            ms = []
            for k in range(args.warmup + args.reps):
                roots, sq, t = pkg.api.test_field_sqrt(curve, deg, words, window=w)
                if not sq.all():
                    raise SystemExit(f"bench_compress: a square was not recognised (curve {curve}, degree {deg}, window {w})")
                if k >= args.warmup:
                    ms.append(t)
            squarings, products = operation_count(q, deg, nr, w)
            rate = n * (squarings + products) * base / (min(ms) * 1e-3)
            res["sqrt"].append({"field": f"Fq{deg if deg > 1 else ''} of {NAME[curve]}", "window": w, "n": n, **stats(ms, n), "squarings": squarings,
                                "products": products, "base_field_products": (squarings + products) * base, "base_field_products_per_s": round(rate, 1),
                                "frac_of_modmul_peak": round(rate / MODMUL_PEAK_PER_S, 4)})
    # ---- decompress / compress per group ----
    for curve in (0, 1):
        for group in (1, 2):
            n = N_POINTS
            wx = pkg.compressed_words(curve, group)
            pts = pkg.synth_points(curve, group, 71 + group, NP)[np.arange(n) % NP]
            d_in = pkg.DeviceBuffer.from_numpy(pts)
            d_x, d_f, d_out = pkg.DeviceBuffer(8 * wx * n), pkg.DeviceBuffer(n), pkg.DeviceBuffer(16 * wx * n)
            t_c = timed(torch, args.reps, args.warmup, lambda: pkg.compress_points(curve, group, d_in.ptr.value, on_device=True, n=n, x_out=d_x.ptr.value,
                                                                                  flags_out=d_f.ptr.value))
            reports = []
            t_d = timed(torch, args.reps, args.warmup, lambda: reports.append(pkg.decompress_points(curve, group, d_x.ptr.value, d_f.ptr.value, on_device=True,
                                                                                                  n=n, out=d_out.ptr.value)[1]))
            if any(r != (0, 0, 0) for r in reports) or not np.array_equal(d_out.to_numpy().reshape(n, -1), pts):
                raise SystemExit(f"bench_compress: the points did not come back (curve {curve}, group {group})")
            res["points"].append({"curve": NAME[curve], "group": group, "n": n, "compress": stats(t_c, n), "decompress": stats(t_d, n)})
    # ---- verify_compressed next to verify ----
    for curve in (0, 1):
        vk, proofs, inp = key_and_proofs(pkg, curve)
        w2 = pkg.affine_words(curve, 2)
        n = cus * 4 * GROUPS_PER_WAVE[curve]
        idx = np.arange(n) % NP
        xs, fl = [], []
        for group, at, words in ((1, 0, 24), (2, 24, w2), (1, 24 + w2, 24)):
            x, f = pkg.compress_points(curve, group, np.ascontiguousarray(proofs[:, at:at + words]))
            xs.append(x)
            fl.append(f)
        x, flags = np.concatenate(xs, axis=1)[idx], np.stack(fl, axis=1)[idx]
        dp, di = pkg.DeviceBuffer.from_numpy(proofs[idx]), pkg.DeviceBuffer.from_numpy(np.tile(inp, (n, 1)))
        dx, df = pkg.DeviceBuffer.from_numpy(x), pkg.DeviceBuffer.from_numpy(flags)
        verdicts = []
        t_plain = timed(torch, args.reps, args.warmup, lambda: verdicts.append(vk.verify(dp.ptr.value, di.ptr.value, on_device=True, n=n)))
        t_comp = timed(torch, args.reps, args.warmup, lambda: verdicts.append(vk.verify_compressed(dx.ptr.value, df.ptr.value, di.ptr.value, on_device=True, n=n)))
        if any(v.any() for v in verdicts):
            raise SystemExit(f"bench_compress: a valid proof was not accepted (curve {curve})")
        vk.close()
        res["verify"].append({"curve": NAME[curve], "n": n, "verify": stats(t_plain, n), "verify_compressed": stats(t_comp, n),
                              "decompress_share": round((min(t_comp) - min(t_plain)) / min(t_comp), 4)})
    line = json.dumps(res)
    out_dir = os.path.join(ROOT, "profiles", "compress")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_compress.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
