#!/bin/bash
# Build an experimental variant of the library next to the product one:
#   tools/build_variant.sh NAME file.hip "-DMACRO=1 ..." [replaces.hip]   -> build_variants/libcra5_NAME.so
# file.hip is a source of cra5_amd/csrc, or a path to a copy kept elsewhere (an earlier commit's version, say:
#   git show HEAD~1:cra5_amd/csrc/attention_split_f16.hip > build_variants/parent_attention_split_f16.hip
#   tools/build_variant.sh parent build_variants/parent_attention_split_f16.hip "" attention_split_f16.hip);
# replaces.hip names the source of the product whose object it stands in for (default: file.hip's own name).
# Select it at run time with CRA5_LIB=build_variants/libcra5_NAME.so, or beside the product in one process with
# tools/attn_ab.py.
set -e
cd "$(dirname "$0")/.."
name=$1; src=$2; defs=$3; repl=${4:-$(basename "$src")}
[ -f "$src" ] || src=cra5_amd/csrc/$src
python -m cra5_amd.build >/dev/null
mkdir -p build_variants
obj=build_variants/${name}_${repl%.hip}.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -pragma-unroll-threshold=262144 -Wno-inline-asm -I cra5_amd/csrc $defs -c "$src" -o "$obj"
objs=""
for f in $(python -c "import os; from cra5_amd import build; print(' '.join(os.path.splitext(s)[0] for s in build.SOURCES))"); do
  if [ "$f.hip" == "$repl" ]; then objs="$objs $obj"; else objs="$objs cra5_amd/csrc/$f.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build_variants/libcra5_${name}.so $objs -lpthread
echo build_variants/libcra5_${name}.so
