#!/bin/sh
# Mints tests/golden/qap/: the REFERENCE's values of the QAP at a point -- evaluate_all_lagrange_polynomials, compute_vanishing_polynomial
# and r1cs_to_qap_instance_map_with_evaluation -- for tests/test_qap_cpu.py and tests/test_qap_gpu.py.
#
# Build container only: compiles tools/mint_qap.cpp (OUR program) against the reference's sources where they lie, with the flags and
# the objects of oracle/build_ref.sh (oracle/_ref/obj/*.o; run `make -C oracle ref` first).  The binary goes into oracle/_ref/ and is
# never committed; what is committed is data: .bin files of Fr elements in the wire format and one index.json.
#
#     sh tools/mint_qap.sh [reference_dir]
set -e
R=${1:-/root/reference}
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(dirname "$HERE")
O=$ROOT/oracle/_ref
OUT=$ROOT/tests/golden/qap
GMP_SO=/usr/lib/x86_64-linux-gnu/libgmp.so.10
[ -d "$R/libsnark" ] || { echo "mint_qap: $R not found"; exit 1; }
ls $O/obj/*.o >/dev/null 2>&1 || { echo "mint_qap: $O/obj is empty: run make -C oracle ref"; exit 1; }
F="-std=c++14 -O2 -fopenmp -DMULTICORE=1 -DBINARY_OUTPUT -DMONTGOMERY_OUTPUT -DNO_PT_COMPRESSION=1 -DUSE_ASM -DNO_PROCPS -DCURVE_MNT4 -I$O/inc -I$R -I$R/depends/libff -I$R/depends/libfqfft -w"
g++ $F -I$R/libsnark/prover_reference_include $HERE/mint_qap.cpp $O/obj/*.o -o $O/mint_qap $GMP_SO
WORK=$(mktemp -d)
trap 'rm -rf "$WORK"' EXIT
mkdir -p $OUT $WORK/mnt4 $WORK/mnt6
# the generic t of both curves: synth_scalars(curve, 0x51, 1) of the library (host code, no device)
python3 - "$ROOT" "$OUT" <<'EOF'
import sys
sys.path.insert(0, sys.argv[1])
from __graft_entry__ import load_package
pkg = load_package()
for curve, name in ((0, "mnt4"), (1, "mnt6")):
    pkg.synth_scalars(curve, 0x51, 1).tofile(f"{sys.argv[2]}/t_{name}.bin")
EOF
$O/mint_qap MNT4753 $WORK/mnt4 $OUT/t_mnt4.bin $ROOT/tests/golden/g16_mnt4/r1cs.bin > $WORK/mnt4/log
$O/mint_qap MNT6753 $WORK/mnt6 $OUT/t_mnt6.bin $ROOT/tests/golden/g16_mnt6/r1cs.bin > $WORK/mnt6/log
cat $WORK/mnt4/log $WORK/mnt6/log
# the index; vectors above 1152 elements are kept as their sha256 and a sample (a 6 MB vector is over what the repository commits)
python3 - "$WORK" "$OUT" <<'EOF'
import hashlib, json, os, re, sys
work, out = sys.argv[1], sys.argv[2]
FULL_LIMIT = 1152
CLASS_KIND = {"basic_radix2_domain": "basic", "extended_radix2_domain": "extended", "step_radix2_domain": "step"}
def sample_indices(m):
    return sorted(set(list(range(16)) + list(range(m // 2 - 8, m // 2 + 8)) + list(range(m - 16, m)) + list(range(0, m, 1021))))
index = {"_about": "the reference's QAP at a point: minted by tools/mint_qap.sh (tools/mint_qap.cpp on the reference's libfqfft / libsnark) in the "
                   "build container; every element is 12 little-endian uint64, Montgomery form",
         "t": "synth_scalars(curve, 0x51, 1)", "lagrange": [], "qap": []}
for name, curve in (("mnt4", 0), ("mnt6", 1)):
    for line in open(os.path.join(work, name, "log")):
        f = dict(kv.split("=", 1) for kv in line.split()[2:])
        if line.startswith("qap "):
            data = open(os.path.join(work, name, "qap.bin"), "rb").read()
            open(os.path.join(out, f"qap_{name}.bin"), "wb").write(data)
            index["qap"].append({"curve": curve, "file": f"qap_{name}.bin", "t_file": f"t_{name}.bin", "r1cs": f"g16_{name}/r1cs.bin",
                                 "num_inputs": int(f["num_inputs"]), "num_variables": int(f["num_variables"]),
                                 "num_constraints": int(f["num_constraints"]), "m": int(f["m"]), "reference_class": f["class"],
                                 "layout": "At | Bt | Ct (num_variables + 1 each) | Ht (m + 1) | Zt", "sha256": hashlib.sha256(data).hexdigest()})
        elif line.startswith("lag "):
            m, min_size = int(f["m"]), int(f["min_size"])
            kind = CLASS_KIND.get(f["class"], f["class"])
            if kind == "basic" and m & (m - 1):
                kind = "mixed"           # a basic_radix2_domain of 2^a 5^b elements
            data = open(os.path.join(work, name, f"lag_{min_size}.bin"), "rb").read()
            rec_bytes = 96 * (m + 2)
            labels = f["t"].split(",")
            assert len(data) == rec_bytes * len(labels)
            entry = {"curve": curve, "min_size": min_size, "m": m, "reference_class": f["class"], "kind": kind, "t": labels,
                     "file": f"lag_{name}_{min_size}.bin", "u_sha256": []}
            keep = b""
            idx = None if m <= FULL_LIMIT else sample_indices(m)
            for k in range(len(labels)):
                rec = data[k * rec_bytes:(k + 1) * rec_bytes]
                u = rec[192:]
                entry["u_sha256"].append(hashlib.sha256(u).hexdigest())
                keep += rec if idx is None else rec[:192] + b"".join(u[96 * i:96 * i + 96] for i in idx)
            entry["layout"] = "per t: t | Z(t) | u[0 .. m)" if idx is None else "per t: t | Z(t) | u[i] for i in sample_indices"
            if idx is not None:
                entry["sample_indices"] = idx
            open(os.path.join(out, entry["file"]), "wb").write(keep)
            index["lagrange"].append(entry)
json.dump(index, open(os.path.join(out, "index.json"), "w"), indent=1)
print("mint_qap: wrote", len(index["lagrange"]), "Lagrange files and", len(index["qap"]), "instance maps into", out)
EOF
