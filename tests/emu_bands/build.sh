#!/usr/bin/env bash
# TEST INFRASTRUCTURE ONLY: builds tests/_emu_bands/librrtmg_emu_bands.so (host emulation of the band fluxes of both
# spectra, emu_bands.hip).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="$ROOT/tests/_emu_bands"
mkdir -p "$OUT"
CC="hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -ffp-contract=off"
pids=()
for src in "$HERE/emu_bands.hip" "$ROOT/climt_amd/csrc/rrtmg_tables.cpp" "$ROOT/tests/emu/mt_host_stream.cpp"; do
  $CC -c "$src" -o "$OUT/$(basename "$src").o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
$CC -shared -o "$OUT/librrtmg_emu_bands.so" "$OUT/emu_bands.hip.o" "$OUT/rrtmg_tables.cpp.o" "$OUT/mt_host_stream.cpp.o"
echo "built tests/_emu_bands/librrtmg_emu_bands.so"
