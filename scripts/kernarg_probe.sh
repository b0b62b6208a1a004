#!/bin/sh
# Builds and runs scripts/kernarg_probe.hip: the same source without and with kernel-argument preload.
#   scripts/kernarg_probe.sh build     compile both programs (no GPU needed)
#   scripts/kernarg_probe.sh run       run them, plain first; one JSON line per block offset and program
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
case "$1" in
build)
    $HIPCC -O3 -std=c++17 --offload-arch=gfx950 kernarg_probe.hip -o kernarg_probe_plain
    $HIPCC -O3 -std=c++17 --offload-arch=gfx950 -mllvm -amdgpu-kernarg-preload-count=6 kernarg_probe.hip -o kernarg_probe_preload
    ;;
run)
    echo "# plain" && timeout -k 10 60 ./kernarg_probe_plain && echo "# preload" && timeout -k 10 60 ./kernarg_probe_preload
    ;;
*)
    echo "usage: $0 build|run" >&2
    exit 2
    ;;
esac
