#!/usr/bin/env python3
"""Times the fixed-base batch scalar multiplication (FixedBase / mnt753_batch_exp) and prints ONE JSON line.

Per case -- 2^20 G1 scalars on both curves, 2^18 G2 scalars on both -- at the library's default width: the table build and the walk
and the normalisation of one pass over all scalars, from HIP events (mnt753_fixed_base_last_timing; tile = n so that the pass is the
call), scalars and output resident on the device; the wall time of the same call at the default tile; the product count per scalar
(W mixed additions of 11 products, 6 per result for the normalisation and the wire form) and what fraction of the measured multiplier peak
(profiles/r01/mulbench_mi355x.txt, the figure bench.py uses) the walk reaches; and the time of the only other route to these points,
mnt753_point_scale per scalar on one host thread (256 scalars, extrapolated).  --sweep adds the walk time per width for the G1 cases
(and the G2 cases at a quarter of their size).  Every result is spot-checked against point_scale on four outputs.

    python tools/bench_batch_exp.py [--sweep] [--log-n1 20] [--log-n2 18] [--widths 8,10,...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

PEAK_GMULS = 22.0   # 1e9 753-bit Montgomery products per second, whole chip, measured: profiles/r01/mulbench_mi355x.txt (MODMUL_PEAK_PER_S of bench.py)
DEG = {(0, 1): 1, (1, 1): 1, (0, 2): 2, (1, 2): 3}
# base-field products per extension-field product on the lane-split fields: every lane runs one fused product of DEG terms
BASE_PER_PRODUCT = {1: 1, 2: 3, 3: 6}   # 2 lanes x fp_mul2 (2187 multiply-adds) = 3 x 1458; 3 lanes x fp_mul3 (2916) = 6 x 1458


def timed_call(pkg, fb, d_s, d_o, n, reps):
    best = None
    for _ in range(reps):
        fb.batch_exp(d_s.ptr.value, on_device=True, n=n, out_ptr=d_o.ptr.value)
        t = fb.last_timing()
        if best is None or t["walk_ms"] + t["normalise_ms"] < best["walk_ms"] + best["normalise_ms"]:
            best = t
    return best


def wall_call(pkg, fb, d_s, d_o, n, reps):
    best = 1e30
    for _ in range(reps):
        pkg.lib().mnt753_sync(None)
        t0 = time.perf_counter()
        fb.batch_exp(d_s.ptr.value, on_device=True, n=n, out_ptr=d_o.ptr.value)
        pkg.lib().mnt753_sync(None)
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def spot_check(pkg, curve, group, point, scalars, d_o, n):
    aw = pkg.affine_words(curve, group)
    out = d_o.to_numpy().reshape(-1, aw)[:n]
    proj = pkg.point_from_affine(curve, group, point)
    for k in (0, 1, n // 2, n - 1):
        exp = pkg.point_to_affine(curve, group, pkg.point_scale(curve, group, scalars[k], proj))
        if not np.array_equal(out[k], exp):
            raise SystemExit(f"bench_batch_exp: output {k} of curve {curve} group {group} differs from point_scale")


def host_route_ms(pkg, curve, group, point, scalars, n):
    proj = pkg.point_from_affine(curve, group, point)
    t0 = time.perf_counter()
    for k in range(256):
        pkg.point_to_affine(curve, group, pkg.point_scale(curve, group, scalars[k], proj))
    return (time.perf_counter() - t0) * 1e3 / 256 * n


def case(pkg, curve, group, log_n, reps, sweep_widths, sweep_log_n):
    n = 1 << log_n
    aw = pkg.affine_words(curve, group)
    point = pkg.api.test_generator(curve, group)
    scalars = pkg.synth_scalars(curve, 4242, n)
    d_s = pkg.DeviceBuffer.from_numpy(scalars)
    d_o = pkg.DeviceBuffer(8 * aw * n)
    res = {"curve": curve, "group": group, "log_n": log_n}
    try:
        fb = pkg.FixedBase(curve, group, point, tile=n)
        plan = fb.plan()
        fb.batch_exp(d_s.ptr.value, on_device=True, n=n, out_ptr=d_o.ptr.value)   # warm-up
        t = timed_call(pkg, fb, d_s, d_o, n, reps)
        spot_check(pkg, curve, group, point, scalars, d_o, n)
        products = (plan["windows"] * 11 + 6) * BASE_PER_PRODUCT[DEG[(curve, group)]]
        res.update(window_bits=plan["window_bits"], windows=plan["windows"], table_mb=round(fb.table_bytes / 2**20, 1),
                   table_build_ms=round(t["table_build_ms"], 3), walk_ms=round(t["walk_ms"], 3), normalise_ms=round(t["normalise_ms"], 3),
                   base_field_products_per_scalar=products,
                   fraction_of_multiplier_peak=round(products * n / ((t["walk_ms"] + t["normalise_ms"]) * 1e-3) / (PEAK_GMULS * 1e9), 3))
        fb.close()
        fb = pkg.FixedBase(curve, group, point)
        fb.batch_exp(d_s.ptr.value, on_device=True, n=n, out_ptr=d_o.ptr.value)
        res.update(default_tile=fb.plan()["tile"], wall_ms_default_tile=round(wall_call(pkg, fb, d_s, d_o, n, reps), 3))
        fb.close()
        res["host_point_scale_ms_extrapolated"] = round(host_route_ms(pkg, curve, group, point, scalars, n), 1)
        if sweep_widths:
            m = 1 << sweep_log_n
            sweep = {}
            for w in sweep_widths:
                try:
                    fb = pkg.FixedBase(curve, group, point, window_bits=w, tile=m)
                except pkg.Mnt753Error as e:
                    sweep[str(w)] = {"error": str(e)[:80]}
                    continue
                fb.batch_exp(d_s.ptr.value, on_device=True, n=m, out_ptr=d_o.ptr.value)
                t = timed_call(pkg, fb, d_s, d_o, m, max(1, reps - 1))
                sweep[str(w)] = {"table_mb": round(fb.table_bytes / 2**20, 1), "table_build_ms": round(t["table_build_ms"], 2),
                                 "walk_ms": round(t["walk_ms"], 3), "normalise_ms": round(t["normalise_ms"], 3)}
                fb.close()
            res["sweep_log_n"] = sweep_log_n
            res["width_sweep"] = sweep
    finally:
        d_s.close(); d_o.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n1", type=int, default=20)
    ap.add_argument("--log-n2", type=int, default=18)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--widths", default="8,10,12,13,14,15,16,17,18")
    a = ap.parse_args()
    pkg = load_package()
    pkg.init(0)
    widths = [int(w) for w in a.widths.split(",")] if a.sweep else []
    cases = []
    for curve, group in ((0, 1), (1, 1), (0, 2), (1, 2)):
        log_n = a.log_n1 if group == 1 else a.log_n2
        cases.append(case(pkg, curve, group, log_n, a.reps, widths, log_n if group == 1 else log_n - 2))
    print(json.dumps({"bench": "batch_exp", "peak_gmuls": PEAK_GMULS, "cases": cases}))


if __name__ == "__main__":
    main()
