#!/bin/bash
# Dev tool: prove that a kernel clean-up changes no machine instruction.  Needs hipcc, no GPU.
#   tools/isa_diff.sh <parent-ref> [file.hip ...]      (default: every geoformer_amd/csrc/*.hip)
# Compiles each source device-only to gfx950 assembly with the library's own flags (geoformer_amd/_build.py), once from
# <parent-ref> (git archive into a temporary directory) and once from the working tree, drops the lines that hold the
# per-compilation __hip_cuid_ symbol and the assembler comment lines (first non-blank character `;`) and compares.  The
# compiler moves its `; implicit-def:` notes when a loop becomes an inlined call although no instruction moves; every
# instruction, label and directive is still compared.  The .amdhsa_* directives (registers, LDS, scratch) are part of the
# text, so occupancy is covered.  Prints a verdict per file, under a file that differs the kernels whose bodies differ
# (needs c++filt); exit status 1 if any kernel differs or a file fails to compile.
#   ISA_DIFF_RENAME=<file>: `old new` name pairs, one per line, replaced in both sides' assembly before the comparison (for
#                        kernels and types that a clean-up renames).  When the whole files then differ, the per-kernel
#                        comparison below is the verdict: `same kernels` if no kernel's body differs, and only then is
#                        the size of a kernel's arguments left out of it.  A pair becomes an unanchored sed expression
#                        over the whole assembly: give names long enough to hit nothing else, or a whole mangled symbol
#                        where a signature changes
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
    grep -v -e __hip_cuid_ -e '^[[:space:]]*;' "$3.raw" | sed -f "$renames" > "$3"; rm -f "$3.raw"
}
renames=$tmp/renames.sed  # `old new` per line -> s/old/new/g (names of equal length keep a mangled name valid)
awk 'NF == 2 { printf "s/%s/%s/g\n", $1, $2 }' ${ISA_DIFF_RENAME:+"$ISA_DIFF_RENAME"} < /dev/null > "$renames" || exit 2
export -f asm; export hipcc renames
for n in $names; do
    printf '%s\0%s\0%s\0' "$tmp/src" "$n" "$out/parent/${n%.hip}.s"
    printf '%s\0%s\0%s\0' "$root" "$n" "$out/head/${n%.hip}.s"
done | xargs -0 -n 3 -P "$jobs" bash -c 'asm "$0" "$1" "$2" || touch "$2.failed"'

# The kernels of a file that differs, one line each: demangled name, lines before -> after, then the register / LDS /
# scratch directives before -> after.  A kernel is its symbol's text from the `_Z...:` label to its .Lfunc_end (the
# .amdhsa_* block lies in between), with the function numbers of the local labels (.LBB, .Ltmp, .Lfunc_end, and the BB of a
# trailing `; in Loop: Header=BB...` or `; Parent Loop BB...` comment) dropped: a template that moves into a header is
# emitted in another place, which renumbers the labels of every kernel after it without moving an instruction.  With a
# rename list the .amdhsa_kernarg_size line is left out too: an argument struct that loses a field changes that and no more.
kernels_diff() {  # <parent.s> <head.s>
    awk -v renamed="${ISA_DIFF_RENAME:+1}" '
        FNR == 1 { side++ }
        /^_Z[A-Za-z0-9_.$]*:/ { sym = $1; sub(/:$/, "", sym); seen[sym]; next }
        sym == "" { next }
        /^\.Lfunc_end/ { sym = ""; next }
        renamed && $1 == ".amdhsa_kernarg_size" { next }
        { l = $0; gsub(/\.L(BB|tmp|func_end)[0-9]+/, ".L", l); gsub(/BB[0-9]+_/, "BB_", l); body[side, sym] = body[side, sym] l "\n"; n[side, sym]++ }
        $1 ~ /^\.amdhsa_(next_free_[vs]gpr|accum_offset|(group|private)_segment_fixed_size)$/ { val[side, sym, $1] = $2 }
        END {
            split("next_free_vgpr accum_offset next_free_sgpr group_segment_fixed_size private_segment_fixed_size", key, " ")
            for (s in seen) if (body[1, s] != body[2, s]) {
                line = sprintf("    %s: %d -> %d lines;", s, n[1, s], n[2, s])
                for (i = 1; i <= 5; i++) line = line sprintf(" %s %s -> %s%s", key[i], val[1, s, ".amdhsa_" key[i]], val[2, s, ".amdhsa_" key[i]], i < 5 ? "," : "")
                print line
            }
        }' "$1" "$2" | c++filt -p | sort
}

bad=0
for n in $names; do
    p=$out/parent/${n%.hip}.s; h=$out/head/${n%.hip}.s
    if [ -e "$p.failed" ] || [ -e "$h.failed" ]; then
        echo "FAILED     $n (missing or does not compile: $([ -e "$p.failed" ] && echo parent) $([ -e "$h.failed" ] && echo head))"; bad=1
    elif cmp -s "$p" "$h"; then
        echo "identical  $n ($(wc -l < "$h") lines)"
    else
        k=$(kernels_diff "$p" "$h")
        if [ -z "$k" ]; then
            echo "same kernels  $n ($(diff "$p" "$h" | grep -c '^[<>]') lines differ in label numbers, argument sizes or outside the kernels, of $(wc -l < "$h"))"
        else
            echo "DIFFERENT  $n ($(diff "$p" "$h" | grep -c '^[<>]') differing lines of $(wc -l < "$h"))"; bad=1
            echo "$k"
        fi
    fi
done
[ $bad -eq 0 ] && echo "same ISA in every file against $ref" || echo "ISA differs against $ref"
exit $bad
