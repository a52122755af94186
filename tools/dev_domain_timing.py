#!/usr/bin/env python3
"""Development timing (GPU box): compute_H per evaluation domain, HIP events on the default stream, 5 warm-up + 20 timed calls.

    python tools/dev_domain_timing.py [--lib PATH/libmnt753_hip.so] CASE [CASE ...]       CASE = MNT4753:1048576, MNT6753:65536, MNT6753:163840, ...

Plain ctypes on the library named by --lib (default: the one in the package directory), so that an OLDER build -- one without
mnt753_domain_create_for -- can be timed on its power-of-two sizes for an A/B comparison on one box: run the two builds alternately,
three times each, and compare the differences with each build's own run-to-run spread.  Prints one JSON line per case:
median / min / max milliseconds per compute_H, the domain's creation time and the device memory it occupies."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, TIMED = 5, 20


def main():
    args = sys.argv[1:]
    lib_path = os.path.join(ROOT, "snark-challenge-prover-reference_amd", "libmnt753_hip.so")
    if args[:1] == ["--lib"]:
        lib_path, args = args[1], args[2:]
    L = C.CDLL(lib_path)
    hip = C.CDLL("libamdhip64.so")
    vp, sz = C.c_void_p, C.c_size_t
    L.mnt753_last_error.restype = C.c_char_p
    L.mnt753_dev_alloc.argtypes = [C.POINTER(vp), sz]
    L.mnt753_dev_free.argtypes = [vp]
    L.mnt753_copy_h2d.argtypes = [vp, vp, sz]
    L.mnt753_sync.argtypes = [vp]
    L.mnt753_dev_mem_info.argtypes = [C.POINTER(sz), C.POINTER(sz)]
    L.mnt753_synth_scalars.argtypes = [C.c_int, C.c_uint64, sz, vp]
    L.mnt753_domain_free.argtypes = [vp]
    L.mnt753_domain_size.argtypes = [vp]
    L.mnt753_domain_size.restype = sz
    L.mnt753_compute_h.argtypes = [vp] * 6
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"{what} failed (rc={rc}): {L.mnt753_last_error().decode()}")

    create = getattr(L, "mnt753_domain_create_for", None) or L.mnt753_domain_create     # an older build: power-of-two sizes only
    create.argtypes = [C.c_int, sz, C.POINTER(vp)]
    if hasattr(L, "mnt753_domain_create_for_ex"):      # mixed-radix sizes of MNT6753 (5 * 2^15, 25 * 2^15) allowed; the others select as before
        L.mnt753_domain_create_for_ex.argtypes = [C.c_int, sz, C.c_uint, C.POINTER(vp)]
        create = lambda curve, m, out: L.mnt753_domain_create_for_ex(curve, m, 1, out)
    ok(L.mnt753_init(0), "mnt753_init")
    ev = [vp(), vp()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    for case in args:
        name, m = case.split(":")
        curve, m = {"MNT4753": 0, "MNT6753": 1}[name], int(m)
        free0, free1, total = sz(), sz(), sz()
        L.mnt753_sync(None)
        L.mnt753_dev_mem_info(C.byref(free0), C.byref(total))
        dom = vp()
        t0 = time.time()
        ok(create(curve, m, C.byref(dom)), "domain creation")
        L.mnt753_sync(None)
        create_ms = (time.time() - t0) * 1e3
        L.mnt753_dev_mem_info(C.byref(free1), C.byref(total))
        assert L.mnt753_domain_size(dom) == m
        host = (C.c_uint64 * (12 * m))()
        bufs = []
        for k in range(4):
            p = vp()
            ok(L.mnt753_dev_alloc(C.byref(p), 96 * (m + 1)), "mnt753_dev_alloc")
            if k < 3:
                ok(L.mnt753_synth_scalars(curve, 11 + k, m, host), "mnt753_synth_scalars")
                ok(L.mnt753_copy_h2d(p, host, 96 * m), "mnt753_copy_h2d")
            bufs.append(p)
        times = []
        for it in range(WARMUP + TIMED):       # the vectors are transformed in place: every call works on what the last one left, same cost
            hip.hipEventRecord(ev[0], None)
            ok(L.mnt753_compute_h(dom, bufs[0], bufs[1], bufs[2], bufs[3], None), "mnt753_compute_h")
            hip.hipEventRecord(ev[1], None)
            hip.hipEventSynchronize(ev[1])
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
            if it >= WARMUP:
                times.append(ms.value)
        for p in bufs:
            L.mnt753_dev_free(p)
        L.mnt753_domain_free(dom)
        print(json.dumps({"lib": os.path.relpath(lib_path, ROOT), "case": case, "compute_h_ms_median": round(statistics.median(times), 4),
                          "min": round(min(times), 4), "max": round(max(times), 4), "create_ms": round(create_ms, 1),
                          "domain_device_bytes": free0.value - free1.value}), flush=True)


if __name__ == "__main__":
    main()
