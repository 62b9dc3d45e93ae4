#!/bin/bash
# device_asm.sh FILE.hip OUT.s -- gfx950 device assembly of one translation unit, compiled with build.sh's flags, for comparing a
# kernel file before and after a refactor (cmp).  The __hip_cuid_ symbol is a fresh hash on every compile: its lines are dropped.
set -euo pipefail
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S -o "$2.raw" "$1"
grep -v __hip_cuid_ "$2.raw" > "$2"
rm "$2.raw"
