#!/usr/bin/env bash
# TEST INFRASTRUCTURE ONLY: builds tests/_emu_albedo/librrtmg_emu_albedo.so (host emulation of the shortwave with the surface
# albedo by band, emu_sw_albedo.hip).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="$ROOT/tests/_emu_albedo"
mkdir -p "$OUT"
CC="hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -ffp-contract=off"
pids=()
for src in "$HERE/emu_sw_albedo.hip" "$ROOT/climt_amd/csrc/rrtmg_tables.cpp"; do
  $CC -c "$src" -o "$OUT/$(basename "$src").o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
$CC -shared -o "$OUT/librrtmg_emu_albedo.so" "$OUT/emu_sw_albedo.hip.o" "$OUT/rrtmg_tables.cpp.o"
echo "built tests/_emu_albedo/librrtmg_emu_albedo.so"
