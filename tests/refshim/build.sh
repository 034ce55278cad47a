#!/usr/bin/env bash
# TEST INFRASTRUCTURE ONLY: builds tests/_refshim/libsw_shim.so and liblw_bands_shim.so, our drivers of the reference's
# shortwave / longwave procedures (sw_shim.f90, lw_bands_shim.f90), against the module files and the shared libraries that
# oracle/build_ref.sh made in oracle/_ref/.  Nothing is built (exit 0) where those are absent or no Fortran compiler is found.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
REF="$ROOT/oracle/_ref"
FC="${FC:-/opt/rocm/lib/llvm/bin/flang}"
OUT="$ROOT/tests/_refshim"
for shim in sw_shim lw_bands_shim; do
  w="${shim%%_*}"
  if [ ! -f "$REF/librrtmg_${w}_ref.so" ] || [ ! -f "$REF/$w/parkind.mod" ] || ! command -v "$FC" > /dev/null; then
    echo "refshim ($shim): oracle/_ref or $FC not present -- not built" >&2
    continue
  fi
  SRC="$HERE/$shim.f90" LIB="$OUT/lib$shim.so" DIR="$OUT/$shim"
  if [ -f "$LIB" ] && [ "$LIB" -nt "$SRC" ] && [ "$LIB" -nt "$REF/librrtmg_${w}_ref.so" ]; then continue; fi
  mkdir -p "$DIR"
  (cd "$DIR" && "$FC" -fPIC -O2 -c "$SRC" -o "$DIR/$shim.o" -module-dir "$DIR" -I"$REF/$w")
  # linked AGAINST the reference library (not its objects): one copy of the reference's module state in the process
  "$FC" -shared -fPIC -o "$LIB" "$DIR/$shim.o" -L"$REF" -lrrtmg_${w}_ref -Wl,-rpath,"$REF"
  echo "built $LIB"
done
