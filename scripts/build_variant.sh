#!/bin/bash
# Build libswbank with extra compile flags into lib/libswbank_NAME.so (A/B of kernel variants on
# one box with SWBANK_LIB=...):   scripts/build_variant.sh NAME "-DSWK_PRIO_ROT=0 ..."
# Objects go to build/var_NAME; the CLI is not built.  Every in-tree .so travels with the tree
# to the GPU box: delete the variant when its A/B is done.
set -eu
NAME=$1; FLAGS=${2:-}
cd "$(dirname "$0")/../smith-waterman-fpga-module_amd"
make -j8 BUILD_DIR="build/var_$NAME" LIB_FILE="lib/libswbank_$NAME.so" EXTRA_HIPFLAGS="$FLAGS" \
  "lib/libswbank_$NAME.so"
echo "lib/libswbank_$NAME.so"
