#!/bin/bash
# mkvar.sh NAME [extra hipcc flags]: compile the working tree into build/variants/lib_NAME.so (build/ is git-ignored)
name=$1; shift
mkdir -p build/variants
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-unused-function -shared "$@" -o build/variants/lib_$name.so -x hip ccfindr_amd/csrc/*.cpp ccfindr_amd/csrc/*.hip -pthread 2>&1 | grep -E "error|spill"
ls -la build/variants/lib_$name.so
