#!/bin/bash
# Builds the CPU emulation of the device Huffman decoder (scratch/jpeg_huff_emu.cpp, its shim scratch/jpeg_huff_emu.h) twice:
#   ./jpeg_huff_emu_build.sh OUTDIR   ->   OUTDIR/jpeg_huff_emu_asan (-fsanitize=address,undefined), OUTDIR/jpeg_huff_emu_tsan (-fsanitize=thread)
# CPU only: no GPU, no HIP runtime, nothing loaded into an interpreter.  csrc/jpeg_huff.hip and csrc/jpeg.hip are compiled as they are; the
# shim stands in for wu_common.h.  Then:
#   python scratch/jpeg_huff_emu_fixtures.py OUTDIR/fixtures && OUTDIR/jpeg_huff_emu_asan --fuzz 6 OUTDIR/fixtures && OUTDIR/jpeg_huff_emu_tsan OUTDIR/fixtures
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
root="$(cd "$here/.." && pwd)"
out="${1:?output directory}"
mkdir -p "$out/src"
cp "$here/jpeg_huff_emu.h" "$out/src/wu_common.h"
cp "$root/weather-unet_amd/csrc/jpeg.hip" "$root/weather-unet_amd/csrc/jpeg_huff.hip" "$here/jpeg_huff_emu.cpp" "$out/src/"
cxx="${CXX:-clang++}"
common=(-x c++ -std=c++17 -O1 -g -fno-omit-frame-pointer -pthread -I "$root/include" -I "$out/src" "$out/src/jpeg_huff_emu.cpp")
"$cxx" "${common[@]}" -fsanitize=address,undefined -fno-sanitize-recover=undefined -o "$out/jpeg_huff_emu_asan"
"$cxx" "${common[@]}" -fsanitize=thread -o "$out/jpeg_huff_emu_tsan"
echo "$out/jpeg_huff_emu_asan $out/jpeg_huff_emu_tsan"
