#!/usr/bin/env python3
"""Times the spot check of compute_H and prints ONE JSON line.

On a 2^20 basic domain of MNT4753 and the 2^15 basic domain of MNT6753, satisfied rows (cc = ca cb by vec_muleq), best of 3 each:

* compute_h against compute_h_checked: wall time around the call and a stream synchronisation (the checked call returns a verdict
  to the host, so both are timed to the same point); the vectors are restored from copies outside the timed region;
* the parts of the check alone: interp_at (lagrange_at + three inner products against one u), vec_dot with one vector, poly_eval
  over m + 1 coefficients, lagrange_at, each with the bytes it reads (96 B per element per stream: 2 streams for vec_dot, 4 for
  the three inner products of interp_at, 1 for poly_eval) and that count per second beside the 8 TB/s HBM roof DESIGN.md section 4.4
  divides by.  The counts leave out the partial sums (at most 1024 blocks x 112 B per result).

Nothing is gated on these numbers.

    python tools/bench_h_check.py [--out profiles/h_check/bench_h_check.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

HBM_ROOF_GBS = 8000.0            # the roof DESIGN.md section 4.4 divides by
REPS = 3


def best_ms(pkg, fn, before=None):
    best = None
    for _ in range(REPS):
        if before:
            before()
        pkg.lib().mnt753_sync(None)
        t0 = time.perf_counter()
        fn()
        pkg.lib().mnt753_sync(None)
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def case(pkg, curve, m):
    dom = pkg.Domain(curve, m)
    a, b = pkg.synth_scalars(curve, 0x61, m), pkg.synth_scalars(curve, 0x62, m)
    src = [pkg.DeviceBuffer.from_numpy(x) for x in (a, b, a)]
    pkg.vec_muleq(curve, src[2].ptr.value, src[1].ptr.value, m)        # cc = ca cb
    work = [pkg.DeviceBuffer(96 * m) for _ in range(3)]
    dh = pkg.DeviceBuffer(96 * (m + 1))
    u = pkg.DeviceBuffer(96 * m)
    t = pkg.synth_scalars(curve, 0x51, 1)[0]
    p = [w.ptr.value for w in work]

    def restore():
        for s, w in zip(src, work):
            pkg.copy_d2d(w.ptr.value, s.ptr.value, 96 * m)

    verdicts = []
    restore(); dom.compute_h(p[0], p[1], p[2], dh.ptr.value)           # warm-up: first launches, the Lagrange workspace
    restore(); verdicts.append(dom.compute_h_checked(p[0], p[1], p[2], dh.ptr.value, t=t)[0])
    plain = best_ms(pkg, lambda: dom.compute_h(p[0], p[1], p[2], dh.ptr.value), restore)
    checked = best_ms(pkg, lambda: verdicts.append(dom.compute_h_checked(p[0], p[1], p[2], dh.ptr.value, t=t)[0]), restore)
    restore()
    parts = {}

    def part(name, fn, streams, n):
        ms = best_ms(pkg, fn)
        gb = 96.0 * streams * n / 1e9
        parts[name] = {"ms": round(ms, 4), "counted_gb": round(gb, 4), "gbs": round(gb / (ms * 1e-3), 1),
                       "fraction_of_hbm_roof": round(gb / (ms * 1e-3) / HBM_ROOF_GBS, 4)}

    part("lagrange_at", lambda: dom.lagrange_at(t, out_ptr=u.ptr.value), 1, m)
    part("interp_at_k3", lambda: dom.interp_at(t, p, u_ptr=u.ptr.value), 4, m)
    part("vec_dot", lambda: pkg.vec_dot(curve, p[0], p[1], m), 2, m)
    part("poly_eval", lambda: pkg.poly_eval(curve, dh.ptr.value, m + 1, t), 1, m + 1)
    out = {"curve": curve, "m": m, "compute_h_ms": round(plain, 4), "compute_h_checked_ms": round(checked, 4),
           "check_ms": round(checked - plain, 4), "check_fraction_of_compute_h": round((checked - plain) / plain, 4),
           "all_verdicts_ok": all(verdicts), "parts": parts}
    for buf in src + work + [dh, u]:
        buf.close()
    dom.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = load_package()
    pkg.init(0)
    res = {"bench": "h_check", "reps": REPS, "timer": "wall clock around the call and a stream synchronisation", "hbm_roof_gbs": HBM_ROOF_GBS,
           "cases": [case(pkg, 0, 1 << 20), case(pkg, 1, 1 << 15)]}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
