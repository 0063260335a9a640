#!/bin/bash
# Builds the CPU emulation of the PNG decoder's two kernels (scratch/png_dec_emu.cpp, its shim scratch/png_dec_emu.h) twice:
#   ./png_dec_emu_build.sh OUTDIR   ->   OUTDIR/png_dec_emu_asan (-fsanitize=address,undefined), OUTDIR/png_dec_emu_tsan (-fsanitize=thread)
# CPU only: no GPU, no HIP runtime, nothing loaded into an interpreter.  csrc/png_dec.hip and png_internal.h are compiled as they are; the
# shim stands in for wu_common.h.  Then:
#   python scratch/png_dec_emu_fixtures.py OUTDIR/fixtures && OUTDIR/png_dec_emu_asan --fuzz 10 OUTDIR/fixtures && OUTDIR/png_dec_emu_tsan OUTDIR/fixtures
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
root="$(cd "$here/.." && pwd)"
out="${1:?output directory}"
mkdir -p "$out/src"
cp "$here/png_dec_emu.h" "$out/src/wu_common.h"
cp "$root/weather-unet_amd/csrc/png_internal.h" "$root/weather-unet_amd/csrc/png_dec.hip" "$here/png_dec_emu.cpp" "$out/src/"
cxx="${CXX:-clang++}"
common=(-x c++ -std=c++17 -O1 -g -fno-omit-frame-pointer -pthread -I "$root/include" -I "$out/src" "$out/src/png_dec_emu.cpp")
"$cxx" "${common[@]}" -fsanitize=address,undefined -fno-sanitize-recover=undefined -o "$out/png_dec_emu_asan"
"$cxx" "${common[@]}" -fsanitize=thread -o "$out/png_dec_emu_tsan"
echo "$out/png_dec_emu_asan $out/png_dec_emu_tsan"
