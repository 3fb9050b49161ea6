#!/bin/bash
# usage: [FILES="conv_f32 conv_halo"] tools/build_variant.sh <name> <extra hipcc -D flags...>   -> variants/lib_<name>.so
# (the listed sources -- default conv_f32.hip and conv_halo.hip -- rebuilt with the flags; every other object of the regular build linked unchanged)
set -e
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}; C=$R/casapose_amd/csrc; name=$1; shift
FILES=${FILES:-"conv_f32 conv_halo"}
mkdir -p $R/variants
make -C $C -s
# the source list, the compiler and the flags are the Makefile's own
srcs=$(make -C $C -s print-SRCS); hipcc=$(make -C $C -s print-HIPCC); flags=$(make -C $C -s print-FLAGS)
objs=""
for n in ${srcs//.hip/}; do
  if echo " $FILES " | grep -q " $n "; then
    $hipcc $flags "$@" -c $C/$n.hip -o /tmp/${n}_$name.o
    objs="$objs /tmp/${n}_$name.o"
  else
    objs="$objs $C/build/$n.o"
  fi
done
$hipcc --offload-arch=gfx950 -shared -fPIC $objs -o $R/variants/lib_$name.so
echo built variants/lib_$name.so
