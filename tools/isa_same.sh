#!/bin/bash
# Is the device code of mve_amd/csrc/dmrecon_device.hip the same in two trees?  CPU only: needs hipcc, no GPU.
#   tools/isa_same.sh <tree-A> <tree-B> [widths]        (default widths: 3 5 7 9 11)
# Per filter width both trees' file is compiled to device assembly with the compiler and the DEVFLAGS of the tree's own Makefile
# (asked from make, not copied here) and -DMI_FW=<w>; the assembly is compared line by line, the __hip_cuid_<hash> lines left out
# (the hash is one of the source TEXT).  Prints the number of differing lines per width; exit status 1 if any width differs.
# The proof a refactor of that file owes: 0 for every width.
set -u
[ $# -ge 2 ] || { echo "usage: $0 <tree-A> <tree-B> [widths]" >&2; exit 2; }
A=$(cd "$1" && pwd) || exit 2
B=$(cd "$2" && pwd) || exit 2
shift 2
WIDTHS=${*:-3 5 7 9 11}
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT

compile() {     # <tree> <tag> <width>
  local dir=$1/mve_amd/csrc
  local ask='isa-same-print: ; @echo $(HIPCC) $(DEVFLAGS)'
  local cmd
  cmd=$(make -s -C "$dir" --no-print-directory --eval "$ask" isa-same-print) || return 1
  (cd "$dir" && $cmd -DMI_FW=$3 --cuda-device-only -S dmrecon_device.hip -o "$OUT/$2_fw$3.s") 2> "$OUT/$2_fw$3.err" \
    || { echo "$1, width $3: does not compile" >&2; tail -20 "$OUT/$2_fw$3.err" >&2; return 1; }
}
export -f compile
export OUT

for w in $WIDTHS; do printf '%s A %s\n%s B %s\n' "$A" "$w" "$B" "$w"; done \
  | xargs -P "$(nproc)" -L 1 bash -c 'compile "$0" "$1" "$2"' || exit 2

status=0
for w in $WIDTHS; do
  n=$(diff <(grep -v __hip_cuid_ "$OUT/A_fw$w.s") <(grep -v __hip_cuid_ "$OUT/B_fw$w.s") | grep -c '^[<>]')
  echo "width $w: $n differing lines"
  [ "$n" -eq 0 ] || status=1
done
exit $status
