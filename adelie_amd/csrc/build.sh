#!/bin/bash
# Builds adelie_amd/libadelie_hip.so for gfx950 (cross-compiles without a GPU).  build.mk has the list of translation units and the
# rules; a failed compile stops the build before the link.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
# AHIP_VARIANT=name builds libadelie_hip_name.so from objects under build_name/ (compile-time A/B variants, with AHIP_EXTRA_FLAGS)
V="${AHIP_VARIANT:-}"
OUT="$HERE/../libadelie_hip${V:+_$V}.so"
OBJ="build${V:+_$V}"
mkdir -p "$HERE/$OBJ"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function ${AHIP_EXTRA_FLAGS:-}"
make -s -C "$HERE" -f build.mk -j "${MAX_JOBS:-$(nproc)}" OBJ="$OBJ" OUT="$OUT" HIPCC="$HIPCC" FLAGS="$FLAGS"
echo "built $OUT"
