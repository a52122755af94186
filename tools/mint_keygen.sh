#!/bin/sh
# Mints tests/golden/keygen_mnt{4,6}_{full,cut21}/: Groth16 keys made by the REFERENCE's own functions from given randomness, for
# tests/test_keygen_cpu.py and tests/test_keygen_gpu.py.
#
# Build container only: compiles tools/mint_keygen.cpp (OUR program) against the reference's sources where they lie, with the flags and
# the objects of oracle/build_ref.sh (oracle/_ref/obj/*.o; run `make -C oracle ref` first).  The binary goes into oracle/_ref/ and is
# never committed; what is committed is data.
#
# Two systems per curve, both derived from tests/golden/g16_mnt{4,6}/r1cs.bin and witness.bin (1 input, 32 variables, 30 constraints; the
# witness satisfies any subset of the constraints):
#   full    the system as it is: a touches 32 variables, b 31 -- no swap; 30 + 1 + 1 = 32: a basic domain of 32 elements
#   cut21   its first 21 constraints: a touches 11, b 22 -- the swap fires; 21 + 1 + 1 = 23: the step domain of 16 + 8 = 24 elements;
#           9 variables are touched by no matrix, so at least 9 rows of A, B (G1 and G2) and L are the identity
# The minting program checks each of these properties and fails if one does not hold.
# Randomness: t, alpha, beta, delta = synth_scalars(curve, 0x6b, 4) of the library (host code, no device); the G1 generator is
# 0x6b65 * G1::one(), computed by libff inside the minting program.
#
#     sh tools/mint_keygen.sh [reference_dir]
set -e
R=${1:-/root/reference}
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(dirname "$HERE")
O=$ROOT/oracle/_ref
G=$ROOT/tests/golden
GMP_SO=/usr/lib/x86_64-linux-gnu/libgmp.so.10
G1_MULTIPLE=0x6b65
[ -d "$R/libsnark" ] || { echo "mint_keygen: $R not found"; exit 1; }
ls $O/obj/*.o >/dev/null 2>&1 || { echo "mint_keygen: $O/obj is empty: run make -C oracle ref"; exit 1; }
F="-std=c++14 -O2 -fopenmp -DMULTICORE=1 -DBINARY_OUTPUT -DMONTGOMERY_OUTPUT -DNO_PT_COMPRESSION=1 -DUSE_ASM -DNO_PROCPS -DCURVE_MNT4 -I$O/inc -I$R -I$R/depends/libff -I$R/depends/libfqfft -w"
g++ $F -I$R/libsnark/prover_reference_include $HERE/mint_keygen.cpp $O/obj/*.o -o $O/mint_keygen $GMP_SO
WORK=$(mktemp -d)
trap 'rm -rf "$WORK"' EXIT
# the inputs: the scalars of both curves, and r1cs_in.bin of the four fixtures
python3 - "$ROOT" "$WORK" <<'EOF'
import os, sys
import numpy as np
root, work = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
from __graft_entry__ import load_package
pkg = load_package()
for curve, name in ((0, "mnt4"), (1, "mnt6")):
    pkg.synth_scalars(curve, 0x6b, 4).tofile(f"{work}/scalars_{name}.bin")
    src = f"{root}/tests/golden/g16_{name}/r1cs.bin"
    ni, m, nc, mats = pkg.api.read_r1cs_file(src)
    for tag, keep in (("full", nc), ("cut21", 21)):
        d = f"{root}/tests/golden/keygen_{name}_{tag}"
        os.makedirs(d, exist_ok=True)
        with open(f"{d}/r1cs_in.bin", "wb") as f:
            f.write(np.array([ni, m, keep], dtype="<u8").tobytes())
            for rp, col, cf in mats:
                nnz = int(rp[keep])
                f.write(rp[:keep + 1].astype("<u8").tobytes())
                f.write(col[:nnz].astype("<u4").tobytes())
                f.write(cf[:nnz].astype("<u8").tobytes())
    assert open(f"{root}/tests/golden/keygen_{name}_full/r1cs_in.bin", "rb").read() == open(src, "rb").read()
EOF
for name in mnt4 mnt6; do
  [ $name = mnt4 ] && CURVE=MNT4753 || CURVE=MNT6753
  for tag in full cut21; do
    D=$G/keygen_${name}_$tag
    cp $G/g16_$name/witness.bin $D/witness.bin
    if [ $tag = full ]; then EXPECT="32 31 basic_radix2_domain 32 0"; else EXPECT="11 22 step_radix2_domain 24 9"; fi
    $O/mint_keygen $CURVE $D/r1cs_in.bin $WORK/scalars_$name.bin $D/witness.bin $D $G1_MULTIPLE $EXPECT > $D/log
    cat $D/log
    python3 - "$D" "$name" "$tag" <<'EOF'
import json, os, sys
d, name, tag = sys.argv[1:4]
line = [l for l in open(os.path.join(d, "log")) if l.startswith("keygen ")][-1]      # libsnark prints its own lines around it
f = dict(kv.split("=", 1) for kv in line.split()[1:])
index = {"_about": "a Groth16 key made by the reference's own functions from given randomness: minted by tools/mint_keygen.sh "
                   "(tools/mint_keygen.cpp on the reference's libff / libfqfft / libsnark) in the build container",
         "curve": 0 if name == "mnt4" else 1, "system": tag,
         "randomness": "t | alpha | beta | delta = synth_scalars(curve, 0x6b, 4); G1 generator = g1_multiple * G1::one()",
         "g1_multiple": int(f["g1_multiple"]), "num_inputs": int(f["num_inputs"]), "num_variables": int(f["num_variables"]),
         "num_constraints": int(f["num_constraints"]), "domain_size": int(f["m"]), "reference_class": f["class"], "swapped": bool(int(f["swapped"])),
         "touched_a": int(f["touched_a"]), "touched_b": int(f["touched_b"]), "untouched_variables": int(f["untouched"]),
         "non_zero_At": int(f["non_zero_At"]), "non_zero_Bt": int(f["non_zero_Bt"]),
         "reference_g1_window": int(f["g1_window"]), "reference_g2_window": int(f["g2_window"])}
with open(os.path.join(d, "index.json"), "w") as out:
    json.dump(index, out, indent=1)
    out.write("\n")
EOF
    rm $D/log
  done
done
# the checksums of these fixtures, in a manifest of their own (tests/test_keygen_cpu.py checks it; SHA256SUMS keeps the other fixtures)
( cd $G && sha256sum keygen_mnt*/* > keygen_SHA256SUMS )
echo "mint_keygen: wrote $(ls -d $G/keygen_mnt* | wc -l) fixtures"
