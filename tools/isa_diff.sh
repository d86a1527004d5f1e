#!/bin/bash
# Dev tool: prove that a kernel clean-up changes no machine instruction.  Needs hipcc, no GPU.
#   tools/isa_diff.sh <parent-ref> [file.hip ...]      (default: every geoformer_amd/csrc/*.hip)
# Compiles each source device-only to gfx950 assembly with the library's own flags (geoformer_amd/_build.py), once from
# <parent-ref> (git archive into a temporary directory) and once from the working tree, drops the lines that hold the
# per-compilation __hip_cuid_ symbol and compares.  The .amdhsa_* directives (registers, LDS, scratch) are part of the
# text, so occupancy is covered.  Prints a verdict per file; exit status 1 if any file differs or fails to compile.
#   ISA_DIFF_KEEP=<dir>: keep the assembly there (<dir>/parent, <dir>/head) instead of a temporary directory
#   ISA_DIFF_JOBS=<n>:   parallel compilations (default 6)
set -u
[ $# -ge 1 ] || { echo "usage: $0 <parent-ref> [file.hip ...]" >&2; exit 2; }
ref=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
hipcc=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
jobs=${ISA_DIFF_JOBS:-6}
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
out=${ISA_DIFF_KEEP:-$tmp}
mkdir -p "$tmp/src" "$out/parent" "$out/head"
git -C "$root" archive "$ref" geoformer_amd/csrc include | tar -x -C "$tmp/src" || exit 2

if [ $# -gt 0 ]; then names=$(for f in "$@"; do basename "$f"; done)
else names=$( (ls "$root/geoformer_amd/csrc" "$tmp/src/geoformer_amd/csrc") | grep '\.hip$' | sort -u); fi

asm() {  # <tree> <name.hip> <out.s>
    [ -f "$1/geoformer_amd/csrc/$2" ] || return 1
    "$hipcc" --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-gpu-rdc -Wno-unused-result \
        "-I$1/include" "-I$1/geoformer_amd/csrc" --cuda-device-only -S "$1/geoformer_amd/csrc/$2" -o "$3.raw" 2> "$3.err" || return 1
    grep -v __hip_cuid_ "$3.raw" > "$3"; rm -f "$3.raw"
}
export -f asm; export hipcc
for n in $names; do
    printf '%s\0%s\0%s\0' "$tmp/src" "$n" "$out/parent/${n%.hip}.s"
    printf '%s\0%s\0%s\0' "$root" "$n" "$out/head/${n%.hip}.s"
done | xargs -0 -n 3 -P "$jobs" bash -c 'asm "$0" "$1" "$2" || touch "$2.failed"'

bad=0
for n in $names; do
    p=$out/parent/${n%.hip}.s; h=$out/head/${n%.hip}.s
    if [ -e "$p.failed" ] || [ -e "$h.failed" ]; then
        echo "FAILED     $n (missing or does not compile: $([ -e "$p.failed" ] && echo parent) $([ -e "$h.failed" ] && echo head))"; bad=1
    elif cmp -s "$p" "$h"; then
        echo "identical  $n ($(wc -l < "$h") lines)"
    else
        echo "DIFFERENT  $n ($(diff "$p" "$h" | grep -c '^[<>]') differing lines of $(wc -l < "$h"))"; bad=1
    fi
done
[ $bad -eq 0 ] && echo "same ISA in every file against $ref" || echo "ISA differs against $ref"
exit $bad
