#!/usr/bin/env bash
# TEST INFRASTRUCTURE ONLY: builds tests/_emu_lw_allsky/librrtmg_emu_lw_allsky.so (host emulation of the longwave device
# functions with the clear-sky outputs off).  Floating-point contraction off, as tests/emu/build.sh.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="$ROOT/tests/_emu_lw_allsky"
mkdir -p "$OUT"
rm -f "$OUT"/*.o
CC="hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -ffp-contract=off"
pids=()
for src in "$HERE/emu_lw_allsky.hip" "$ROOT/climt_amd/csrc/rrtmg_tables.cpp" "$ROOT/tests/emu/mt_host_stream.cpp"; do
  $CC -c "$src" -o "$OUT/$(basename "$src").o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
$CC -shared -o "$OUT/librrtmg_emu_lw_allsky.so" "$OUT"/*.o
echo "built tests/_emu_lw_allsky/librrtmg_emu_lw_allsky.so"
