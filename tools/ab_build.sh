#!/bin/bash
# Build timing-only variants of libgpsjam_hip.so into build_ab/ (ablation / A-B experiments):
#   tools/ab_build.sh <name> "<extra hipcc flags>" [source, default k_welch.hip]
# and run them with GPSJAM_LIB=$PWD/build_ab/libgpsjam_<name>.so python tools/run_kernel.py welch
# The object list and the compile command of <source> are the Makefile's own (asked of make, not copied here), so the
# variant exports everything gpsjam/_ffi.py binds.  To compare with another commit, build the library in a checkout of
# that commit and copy it to build_ab/libgpsjam_<name>.so.
set -euo pipefail
NAME=$1
EXTRA=${2:-}
SRC=${3:-k_welch.hip}
cd "$(dirname "$0")/../gps-jamming_amd/csrc"
mkdir -p ../../build_ab
make -s -j8
OBJ=${SRC%.hip}.o
VARIANT=../../build_ab/ab_$NAME.o
ALL_OBJS=$(printf 'ab-print-objs:\n\t@echo $(OBJS)\n' | make -s -f Makefile -f - ab-print-objs)
HIPCC_BIN=$(printf 'ab-print-hipcc:\n\t@echo $(HIPCC)\n' | make -s -f Makefile -f - ab-print-hipcc)
ARCH=$(printf 'ab-print-arch:\n\t@echo $(ARCH)\n' | make -s -f Makefile -f - ab-print-arch)
case " $ALL_OBJS " in *" $OBJ "*) ;; *) echo "$SRC is not one of the library's sources: $ALL_OBJS" >&2; exit 1;; esac
# the Makefile's command for this object (per-file flags included), with the variant's flags and output
COMPILE=$(make -n -W "$SRC" "$OBJ" | grep -- "-c $SRC")
COMPILE=${COMPILE/-o $OBJ/-o $VARIANT}
$COMPILE $EXTRA
OBJS=""
for o in $ALL_OBJS; do
  if [ "$o" = "$OBJ" ]; then OBJS="$OBJS $VARIANT"; else OBJS="$OBJS $o"; fi
done
"$HIPCC_BIN" -shared -fPIC --offload-arch="$ARCH" -o ../../build_ab/libgpsjam_$NAME.so $OBJS -ldl
echo built build_ab/libgpsjam_$NAME.so
