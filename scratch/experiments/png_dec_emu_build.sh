#!/bin/bash
# Builds the CPU emulation of the two PNG decoder kernels kept here as text: ./png_dec_emu_build.sh OUTDIR  ->  OUTDIR/png_dec_emu
# (256 host threads per workgroup, real barriers; no GPU, no HIP runtime).  Then:  OUTDIR/png_dec_emu a.png a.rgb b.png - ...
# decodes the files as ONE batch; NAME.rgb holds the expected h*w*3 bytes, "-" none.  Exit status 1 if a pixel or a padding byte is wrong.
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
root="$(cd "$here/../.." && pwd)"
out="${1:?output directory}"
mkdir -p "$out"
cp "$here/png_dec_emu.h.txt" "$out/emu.h"
sed 's/#include "wu_common.h"/#include "emu.h"/' "$here/png_dec_internal.h.txt" > "$out/png_internal.h"
cp "$here/png_dec_device.hip.txt" "$out/png_dec.hip"
sed 's/#include "wu_common.h"/#include "emu.h"/' "$root/weather-unet_amd/csrc/png_dec.hip" > "$out/png_dec_parse.cpp"
cp "$here/png_dec_emu_harness.cpp.txt" "$out/harness.cpp"
cxx="${CXX:-clang++}"
"$cxx" -x c++ -std=c++20 -O1 -g -pthread -I "$root/include" -I "$out" "$out/harness.cpp" "$out/png_dec_parse.cpp" -o "$out/png_dec_emu"
echo "$out/png_dec_emu"
