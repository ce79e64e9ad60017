#!/bin/bash
# VGPRs / SGPRs / scratch / occupancy / LDS / instruction count of every kernel in one .hip file (compiler remarks and
# the device assembly; no GPU needed)
#   bash tools/kernel_resources.sh libpll_amd/csrc/hip/partials_fused.hip [name filter]
#   (KR_FLAGS: extra compiler flags, e.g. KR_FLAGS='-mllvm -amdgpu-mfma-vgpr-form' for partials_aa_fused.hip)
f=$1; filt=${2:-.}

flags="--offload-arch=gfx950 -O3 -fPIC -ffp-contract=off -fvisibility=hidden -Iinclude -Ilibpll_amd/csrc/hip $KR_FLAGS"
asm=$(mktemp --suffix=.s)
trap 'rm -f "$asm"' EXIT
/opt/rocm/bin/hipcc $flags --cuda-device-only -S "$f" -o "$asm" 2>/dev/null
# instructions between a kernel's label and the end of its function (labels, directives and comments are not counted)
declare -A ninstr
while read -r name n; do ninstr[$name]=$n; done < <(awk '
  /^[A-Za-z_][A-Za-z0-9_$.]*:/ { if (!in_fn) { name = $1; sub(/:.*/, "", name); in_fn = 1; n = 0 } next }
  /^\.Lfunc_end/ { if (in_fn) print name, n; in_fn = 0; next }
  in_fn && /^[ \t]+[a-z]/ && !/^[ \t]+\./ { ++n }' "$asm")
/opt/rocm/bin/hipcc $flags -c "$f" -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 | \
  grep -E "Function Name|SGPRs:|VGPRs:|ScratchSize|Occupancy|LDS Size" | sed 's/.*remark: [^ ]* *//; s/ \[-Rpass.*//' | \
  paste - - - - - - | grep -E "$filt" | while IFS=$'\t' read -r n s v sc o l; do
    mangled=$(echo "$n" | sed -E 's/^(Function )?Name: //')
    echo "$(echo "$mangled" | c++filt | cut -c1-90) | $s | $v | $sc | $o | $l | instructions: ${ninstr[$mangled]:-?}"
  done
