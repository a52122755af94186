#!/usr/bin/env python3
"""Times the QAP at a point (Domain.lagrange_at, R1cs.qap_at) and prints ONE JSON line.

* lagrange_at: HIP events around the call on a 2^20 basic domain (MNT4753) and on the 2^15 basic and the 25 * 2^15 mixed domain
  of MNT6753, output resident on the device; the first call (it allocates the workspace) and the median of ten later calls.
* qap_at: HIP events around the call on the 2^20-row synthetic system of tests/test_groth16_gpu.py (the generator is copied here: a
  tool does not import a test) on the 2^20 basic domain of MNT4753: the build of the column-major view alone (R1cs.qap_plan, wall
  time) with its bytes, the first call after it, and the median of ten later calls -- and the Lagrange part of that median, so that
  the column sums stand alone.  Beside the times: the counted traffic per term (112 B coefficient + 96 B of u gathered + 8 B of
  permutation: row and term index) and the fraction of the HBM roof the column sums reach, computed as DESIGN.md section 4.4 does
  (algorithmic bytes / time / 8 TB/s).  Two choices that fraction inherits: the count leaves out the partial sums (112 B written and
  read per chunk) and the chunk lists, and it is 216 B where a kernel that also read the 4-byte column index would count 220; and the
  time of the column sums is not measured directly -- it is the median of qap_at less the medians of lagrange_at and vec_powers timed
  on their own.

    python tools/bench_qap.py [--log-rows 20] [--out profiles/qap/bench_qap.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

HBM_ROOF_GBS = 8000.0            # the roof DESIGN.md section 4.4 divides by
BYTES_PER_TERM = 112 + 96 + 8    # coefficient in the device radix, u[row] in wire form, row and term index of the permutation


def synthetic_system(pkg, curve, nc, m, seed, pool=4096):
    """tests/test_groth16_gpu.py synthetic_system: most rows have 1-4 terms, one in 64 has 40-200; every fifth term on column 0"""
    rng = np.random.default_rng(seed)
    coeffs = pkg.synth_scalars(curve, 900 + seed, pool)
    mats = []
    for k in range(3):
        counts = rng.integers(1, 5, size=nc)
        heavy = rng.random(nc) < 1.0 / 64
        counts[heavy] = rng.integers(40, 200, size=int(heavy.sum()))
        counts[rng.random(nc) < 0.01] = 0
        rp = np.zeros(nc + 1, dtype=np.uint64); rp[1:] = np.cumsum(counts)
        nnz = int(rp[nc])
        col = rng.integers(0, m + 1, size=nnz).astype(np.uint32)
        col[::5] = 0
        cf = coeffs[rng.integers(0, pool, size=nnz)]
        mats.append((rp, col, cf))
    return mats


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def first_and_median(fn, reps=10):
    first = event_ms(fn)
    later = [event_ms(fn) for _ in range(reps)]
    return round(first, 3), round(statistics.median(later), 3), round(min(later), 3)


def lagrange_case(pkg, curve, dom, t):
    out = pkg.DeviceBuffer(96 * dom.m)
    first, med, best = first_and_median(lambda: dom.lagrange_at(t, out_ptr=out.ptr.value))
    out.close()
    return {"curve": curve, "kind": dom.kind, "m": dom.m, "first_ms": first, "median_ms": med, "min_ms": best,
            "ns_per_element": round(med * 1e6 / dom.m, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = load_package()
    pkg.init(0)
    torch.cuda.init()
    res = {"bench": "qap", "hbm_roof_gbs": HBM_ROOF_GBS, "bytes_per_term": BYTES_PER_TERM, "lagrange_at": []}
    for curve, make in ((0, lambda: pkg.Domain(0, 1 << a.log_rows)), (1, lambda: pkg.Domain(1, 1 << 15)), (1, lambda: pkg.Domain.mixed(1, 25 << 15))):
        dom = make()
        res["lagrange_at"].append(lagrange_case(pkg, curve, dom, pkg.synth_scalars(curve, 0x51, 1)[0]))
        dom.close()
    curve, rows = 0, 1 << a.log_rows
    nc, m, num_inputs = rows - 8, rows - 1, 5
    mats = synthetic_system(pkg, curve, nc, m, seed=11)
    cs = pkg.R1cs(curve, num_inputs, m, nc, mats)
    dom = pkg.Domain(curve, rows)
    t = pkg.synth_scalars(curve, 0x51, 1)[0]
    t0 = time.perf_counter()
    plan = cs.qap_plan()
    build_ms = (time.perf_counter() - t0) * 1e3
    bufs = [pkg.DeviceBuffer(96 * (m + 1)) for _ in range(3)] + [pkg.DeviceBuffer(96 * (dom.m + 1))]
    outs = tuple(b.ptr.value for b in bufs)
    first, med, best = first_and_median(lambda: cs.qap_at(dom, t, out=outs))
    u = pkg.DeviceBuffer(96 * dom.m)
    lag = [event_ms(lambda: dom.lagrange_at(t, out_ptr=u.ptr.value)) for _ in range(10)]
    pw = [event_ms(lambda: pkg.vec_powers(curve, t, dom.m + 1, out_ptr=bufs[3].ptr.value)) for _ in range(10)]
    lag_ms, pow_ms = statistics.median(lag), statistics.median(pw)
    sums_ms = med - lag_ms - pow_ms
    gb = plan["terms"] * BYTES_PER_TERM / 1e9
    res["qap_at"] = {"curve": curve, "rows": nc, "variables": m, "domain": dom.m, "plan": plan, "transpose_build_ms": round(build_ms, 1),
                     "first_call_ms": first, "median_ms": med, "min_ms": best, "lagrange_part_ms": round(lag_ms, 3), "powers_part_ms": round(pow_ms, 3),
                     "column_sums_ms": round(sums_ms, 3), "counted_gb": round(gb, 3),
                     "column_sums_gbs": round(gb / (sums_ms * 1e-3), 1), "fraction_of_hbm_roof": round(gb / (sums_ms * 1e-3) / HBM_ROOF_GBS, 4)}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
