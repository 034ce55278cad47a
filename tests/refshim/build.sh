#!/usr/bin/env bash
# TEST INFRASTRUCTURE ONLY: builds tests/_refshim/libsw_components_shim.so, our driver of the reference's shortwave
# procedures (sw_components_shim.f90), against the module files and the shared library that oracle/build_ref.sh made in
# oracle/_ref/.  Nothing is built (exit 0) where those are absent or no Fortran compiler is found.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
REF="$ROOT/oracle/_ref"
FC="${FC:-/opt/rocm/lib/llvm/bin/flang}"
OUT="$ROOT/tests/_refshim"
if [ ! -f "$REF/librrtmg_sw_ref.so" ] || [ ! -f "$REF/sw/rrtmg_sw_spcvrt.mod" ] || ! command -v "$FC" > /dev/null; then
  echo "refshim: oracle/_ref or $FC not present -- not built" >&2
  exit 0
fi
mkdir -p "$OUT"
SRC="$HERE/sw_components_shim.f90" LIB="$OUT/libsw_components_shim.so"
if [ -f "$LIB" ] && [ "$LIB" -nt "$SRC" ] && [ "$LIB" -nt "$REF/librrtmg_sw_ref.so" ]; then exit 0; fi
(cd "$OUT" && "$FC" -fPIC -O2 -c "$SRC" -o "$OUT/sw_components_shim.o" -module-dir "$OUT" -I"$REF/sw")
# linked AGAINST the reference library (not its objects): one copy of the reference's module state in the process
"$FC" -shared -fPIC -o "$LIB" "$OUT/sw_components_shim.o" -L"$REF" -lrrtmg_sw_ref -Wl,-rpath,"$REF"
echo "built $LIB"
