#!/usr/bin/env python3
"""Times Groth16 key generation on the device (generate = mnt753_groth16_generate) and its parts, and prints ONE JSON line.

Two systems, the synthetic_system of tests/test_groth16_gpu.py (the generator is copied here: a tool does not import a test): 2^20
rows on MNT4753 (what tools/bench_qap.py uses) and 2^15 rows on MNT6753.  One run, HIP events around every call whose ends are on the
device; calls that block on a count (the swap, the compactions) are wall time and say so in their key (`_wall_ms`).

* whole: generate() on a fresh system (it builds the column-major view of qap_at and both window tables) and a second call on the
  same object (the view is kept; the tables are built again: they belong to the call).
* parts, each on its own: the swap count, qap_plan (the view), qap_at, the combination kernel, the count of At, the two table builds,
  batch_exp for At, Bt, ABC | Lt and Ht on the G1 table and for Bt on the G2 table.
* compaction on against off: batch_exp and batch_exp_sparse on the same object and the same vector, for G1 and G2, with Bt as qap_at
  gives it (its own density) and with entries zeroed on the host down to 50 % and 10 % non-zero.

    python tools/bench_keygen.py [--log-rows-mnt4 20] [--log-rows-mnt6 15] [--out profiles/keygen/bench_keygen.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

G1, G2 = 1, 2


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
    return round(a.elapsed_time(b), 3)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 3), out


def case(pkg, curve, rows):
    nc, m, ni = rows - 8, rows - 1, 5
    mats = synthetic_system(pkg, curve, nc, m, seed=11)
    t, alpha, beta, delta = pkg.synth_scalars(curve, 0x6b, 4)
    g1, g2 = pkg.group_generator(curve, G1), pkg.group_generator(curve, G2)
    res = {"curve": curve, "rows": nc, "variables": m, "num_inputs": ni, "domain": rows}
    # ---- the whole call, first on a fresh system, then again on the same object
    cs, dom = pkg.R1cs(curve, ni, m, nc, mats), pkg.Domain(curve, rows)
    whole = {}
    for name in ("first_call", "second_call"):
        ms, key = wall_ms(lambda: pkg.generate(cs, dom, t, alpha, beta, delta, g1))
        whole[name + "_wall_ms"] = ms
        res.update(non_zero_at=key.non_zero_at, non_zero_bt=key.non_zero_bt)
        whole[name + "_swapped"] = key.swapped
        key.close()
    res["generate"] = whole
    cs.close()
    # ---- the parts, on a fresh system
    cs = pkg.R1cs(curve, ni, m, nc, mats)
    parts = {}
    parts["swap_count_wall_ms"], swapped = wall_ms(cs.swap_ab_if_beneficial)
    parts["swapped"] = swapped
    parts["qap_view_build_wall_ms"], plan = wall_ms(cs.qap_plan)
    bufs = [pkg.DeviceBuffer(96 * (m + 1)) for _ in range(3)] + [pkg.DeviceBuffer(96 * (dom.m + 1))]
    at, bt, ct, ht = (b.ptr.value for b in bufs)
    parts["qap_at_ms"] = event_ms(lambda: cs.qap_at(dom, t, out=(at, bt, ct, ht)))
    zt = dom.vanishing_at(t)
    one = pkg.api.mont_one(curve)
    comb = pkg.DeviceBuffer(96 * (m + 1))
    parts["combine_ms"] = event_ms(lambda: pkg.keygen_combine(curve, at, bt, ct, m + 1, ni, beta, alpha, delta, comb.ptr.value))   # any factor times the same
    parts["count_at_wall_ms"], nz_a = wall_ms(lambda: pkg.compact_nonzero(at, m + 1))
    fb1, fb2 = pkg.FixedBase(curve, G1, g1), pkg.FixedBase(curve, G2, g2)
    parts["g1_plan"], parts["g2_plan"] = fb1.plan(), fb2.plan()
    parts["g1_table_build_ms"] = round(fb1.last_timing()["table_build_ms"], 3)
    parts["g2_table_build_ms"] = round(fb2.last_timing()["table_build_ms"], 3)
    w1, w2 = pkg.affine_words(curve, G1), pkg.affine_words(curve, G2)
    o1, o2 = pkg.DeviceBuffer(8 * w1 * (dom.m + 1)), pkg.DeviceBuffer(8 * w2 * (m + 1))
    parts["batch_exp_g1_at_ms"] = event_ms(lambda: fb1.batch_exp(at, on_device=True, n=m + 1, out_ptr=o1.ptr.value))
    parts["batch_exp_g1_bt_ms"] = event_ms(lambda: fb1.batch_exp(bt, on_device=True, n=m + 1, out_ptr=o1.ptr.value))
    parts["batch_exp_g1_abc_lt_ms"] = event_ms(lambda: fb1.batch_exp(comb.ptr.value, on_device=True, n=m + 1, out_ptr=o1.ptr.value))
    parts["batch_exp_g1_ht_ms"] = event_ms(lambda: fb1.batch_exp(ht, coeff=zt, on_device=True, n=dom.m - 1, out_ptr=o1.ptr.value))
    parts["batch_exp_g2_bt_ms"] = event_ms(lambda: fb2.batch_exp(bt, on_device=True, n=m + 1, out_ptr=o2.ptr.value))
    res["parts"] = parts
    device_parts = ("qap_at_ms", "combine_ms", "g1_table_build_ms", "g2_table_build_ms", "batch_exp_g1_at_ms", "batch_exp_g1_bt_ms",
                    "batch_exp_g1_abc_lt_ms", "batch_exp_g1_ht_ms", "batch_exp_g2_bt_ms")
    res["sum_of_device_parts_ms"] = round(sum(parts[k] for k in device_parts), 3)
    res["sum_of_parts_with_swap_and_count_ms"] = round(res["sum_of_device_parts_ms"] + parts["swap_count_wall_ms"] + parts["count_at_wall_ms"], 3)
    # ---- compaction on against off
    bt_host = bufs[1].to_numpy().reshape(m + 1, 12)
    rng = np.random.default_rng(5)
    nz = np.flatnonzero(bt_host.any(axis=1))
    sweep = []
    for target in (None, 0.5, 0.1):
        v = bt_host.copy()
        if target is not None:
            keep = int(target * (m + 1))
            v[rng.permutation(nz)[keep:]] = 0
        dv = pkg.DeviceBuffer.from_numpy(v)
        row = {"non_zero": int(v.any(axis=1).sum()), "n": m + 1, "density": round(float(v.any(axis=1).mean()), 4)}
        for name, fb, out in (("g1", fb1, o1), ("g2", fb2, o2)):
            row[name + "_dense_ms"] = event_ms(lambda: fb.batch_exp(dv.ptr.value, on_device=True, n=m + 1, out_ptr=out.ptr.value))
            row[name + "_sparse_ms"] = event_ms(lambda: fb.batch_exp_sparse(dv.ptr.value, m + 1, out.ptr.value))
        row["compact_alone_wall_ms"], _ = wall_ms(lambda: pkg.compact_nonzero(dv.ptr.value, m + 1, o2.ptr.value, o1.ptr.value))   # scratch outputs
        sweep.append(row)
        dv.close()
    res["compaction"] = sweep
    for x in bufs + [comb, o1, o2, fb1, fb2, cs, dom]:
        x.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows-mnt4", type=int, default=20)
    ap.add_argument("--log-rows-mnt6", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = load_package()
    pkg.init(0)
    torch.cuda.init()
    res = {"bench": "keygen", "cases": [case(pkg, 0, 1 << a.log_rows_mnt4), case(pkg, 1, 1 << a.log_rows_mnt6)]}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
