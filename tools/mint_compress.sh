#!/bin/sh
# Mints tests/golden/compress/: points and proofs in libff's COMPRESSED stream format, written by the REFERENCE's own operator<< with
# point compression ON (libff's default; the challenge reference and oracle/build_ref.sh build with NO_PT_COMPRESSION), for
# tests/test_compress_cpu.py and tests/test_compress_gpu.py.
#
# Build container only: compiles tools/mint_compress.cpp (OUR program) against the reference's sources where they lie.
# oracle/_ref/obj/*.o were compiled with NO_PT_COMPRESSION, so the four group files whose operator<< / operator>> depend on that
# define are compiled a second time WITHOUT it, into a temporary directory, with otherwise the flags of oracle/build_ref.sh; every
# other object is taken from oracle/_ref/obj (run `make -C oracle ref` first).  oracle/ itself is not touched.  The binary goes into
# oracle/_ref/ and is never committed; what is committed is data:
#   compress/mnt{4,6}_g{1,2}/points.bin   16 points, uncompressed wire words: k G for k = 1 .. 15, the identity in the sixth place
#   compress/mnt{4,6}_g{1,2}/stream.bin   libff's compressed stream of the same points (read back by libff and compared)
#   compress/mnt{4,6}/proof_stream.bin    the compressed stream of the proof in tests/golden/g16_mnt{4,6}/full.bin
#   compress/SHA256SUMS
#
#     sh tools/mint_compress.sh [reference_dir]
set -e
R=${1:-/root/reference}
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(dirname "$HERE")
O=$ROOT/oracle/_ref
G=$ROOT/tests/golden
GMP_SO=/usr/lib/x86_64-linux-gnu/libgmp.so.10
[ -d "$R/libsnark" ] || { echo "mint_compress: $R not found"; exit 1; }
ls $O/obj/*.o >/dev/null 2>&1 || { echo "mint_compress: $O/obj is empty: run make -C oracle ref"; exit 1; }
# the flags of oracle/build_ref.sh without -DNO_PT_COMPRESSION=1
F="-std=c++14 -O2 -fopenmp -DMULTICORE=1 -DBINARY_OUTPUT -DMONTGOMERY_OUTPUT -DUSE_ASM -DNO_PROCPS -DCURVE_MNT4 -I$O/inc -I$R -I$R/depends/libff -I$R/depends/libfqfft -w"
L=$R/depends/libff/libff
WORK=$(mktemp -d)
trap 'rm -rf "$WORK"' EXIT
GROUP_SRCS="algebra/curves/mnt753/mnt4753/mnt4753_g1.cpp algebra/curves/mnt753/mnt4753/mnt4753_g2.cpp algebra/curves/mnt753/mnt6753/mnt6753_g1.cpp algebra/curves/mnt753/mnt6753/mnt6753_g2.cpp"
PIDS=""
for s in $GROUP_SRCS; do
  g++ $F -c $L/$s -o $WORK/$(echo $s | tr / _).o & PIDS="$PIDS $!"
done
for p in $PIDS; do wait $p || { echo "mint_compress: a compile job failed"; exit 1; }; done
# every other object as oracle/build_ref.sh made it
OTHERS=""
for o in $O/obj/*.o; do
  [ -f $WORK/$(basename $o) ] || OTHERS="$OTHERS $o"
done
g++ $F -I$R/libsnark/prover_reference_include $HERE/mint_compress.cpp $WORK/*.o $OTHERS -o $O/mint_compress $GMP_SO
D=$G/compress
mkdir -p $D/mnt4_g1 $D/mnt4_g2 $D/mnt6_g1 $D/mnt6_g2 $D/mnt4 $D/mnt6
$O/mint_compress $D $G/g16_mnt4/full.bin $G/g16_mnt6/full.bin
( cd $D && sha256sum mnt*/* > SHA256SUMS )
echo "mint_compress: wrote $(ls $D/mnt*/* | wc -l) files, $(du -cb $D/mnt*/* | tail -1 | cut -f1) bytes"
