#!/usr/bin/env bash
# TEST INFRASTRUCTURE ONLY: builds tests/_refshim/libsw_albedo_shim.so, our driver of the reference's shortwave procedures
# with the surface albedo given by band (sw_albedo_shim.f90), against the module files and the shared library that
# oracle/build_ref.sh made in oracle/_ref/.  Nothing is built (exit 0) where those are absent or no Fortran compiler is found.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
REF="$ROOT/oracle/_ref"
FC="${FC:-/opt/rocm/lib/llvm/bin/flang}"
OUT="$ROOT/tests/_refshim"
if [ ! -f "$REF/librrtmg_sw_ref.so" ] || [ ! -f "$REF/sw/rrtmg_sw_spcvrt.mod" ] || [ ! -f "$REF/sw/rrtmg_sw_spcvmc.mod" ] ||
   ! command -v "$FC" > /dev/null; then
  echo "refshim (albedo): oracle/_ref or $FC not present -- not built" >&2
  exit 0
fi
SRC="$HERE/sw_albedo_shim.f90" LIB="$OUT/libsw_albedo_shim.so" DIR="$OUT/sw_albedo"
mkdir -p "$DIR"
if [ -f "$LIB" ] && [ "$LIB" -nt "$SRC" ] && [ "$LIB" -nt "$REF/librrtmg_sw_ref.so" ]; then exit 0; fi
(cd "$DIR" && "$FC" -fPIC -O2 -c "$SRC" -o "$DIR/sw_albedo_shim.o" -module-dir "$DIR" -I"$REF/sw")
# linked AGAINST the reference library (not its objects): one copy of the reference's module state in the process
"$FC" -shared -fPIC -o "$LIB" "$DIR/sw_albedo_shim.o" -L"$REF" -lrrtmg_sw_ref -Wl,-rpath,"$REF"
echo "built $LIB"
