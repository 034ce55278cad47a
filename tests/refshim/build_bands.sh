#!/usr/bin/env bash
# TEST INFRASTRUCTURE ONLY: builds tests/_refshim/libsw_bands_shim.so and liblw_bands_shim.so, our drivers of the reference's
# shortwave / longwave procedures band by band (sw_bands_shim.f90, lw_bands_shim.f90), against the module files and the
# shared libraries that oracle/build_ref.sh made in oracle/_ref/.  Nothing is built (exit 0) where those are absent or no
# Fortran compiler is found.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
REF="$ROOT/oracle/_ref"
FC="${FC:-/opt/rocm/lib/llvm/bin/flang}"
OUT="$ROOT/tests/_refshim"
if [ ! -f "$REF/librrtmg_sw_ref.so" ] || [ ! -f "$REF/librrtmg_lw_ref.so" ] || [ ! -f "$REF/sw/rrtmg_sw_spcvrt.mod" ] ||
   [ ! -f "$REF/lw/rrtmg_lw_rtrnmc.mod" ] || ! command -v "$FC" > /dev/null; then
  echo "refshim (bands): oracle/_ref or $FC not present -- not built" >&2
  exit 0
fi
mkdir -p "$OUT/sw_bands" "$OUT/lw_bands"
for w in sw lw; do
  SRC="$HERE/${w}_bands_shim.f90" LIB="$OUT/lib${w}_bands_shim.so" DIR="$OUT/${w}_bands"
  if [ -f "$LIB" ] && [ "$LIB" -nt "$SRC" ] && [ "$LIB" -nt "$REF/librrtmg_${w}_ref.so" ]; then continue; fi
  (cd "$DIR" && "$FC" -fPIC -O2 -c "$SRC" -o "$DIR/${w}_bands_shim.o" -module-dir "$DIR" -I"$REF/$w")
  # linked AGAINST the reference library (not its objects): one copy of the reference's module state in the process
  "$FC" -shared -fPIC -o "$LIB" "$DIR/${w}_bands_shim.o" -L"$REF" -lrrtmg_${w}_ref -Wl,-rpath,"$REF"
  echo "built $LIB"
done
