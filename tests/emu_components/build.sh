#!/usr/bin/env bash
# TEST INFRASTRUCTURE ONLY: builds tests/_emu_components/librrtmg_emu_components.so (host emulation of the shortwave flux
# components, emu_sw_components.hip).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="$ROOT/tests/_emu_components"
mkdir -p "$OUT"
CC="hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -ffp-contract=off"
$CC -c "$HERE/emu_sw_components.hip" -o "$OUT/emu_sw_components.o" &
p1=$!
$CC -c "$ROOT/climt_amd/csrc/rrtmg_tables.cpp" -o "$OUT/rrtmg_tables.o" &
p2=$!
wait $p1; wait $p2
$CC -shared -o "$OUT/librrtmg_emu_components.so" "$OUT/emu_sw_components.o" "$OUT/rrtmg_tables.o"
echo "built tests/_emu_components/librrtmg_emu_components.so"
