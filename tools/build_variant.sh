#!/bin/bash
# Build an alternative kernel library for A/B runs: tools/build_variant.sh NAME [hipcc flags...]
# -> textblaster_amd/libtbhip_NAME.so ; select it with TB_HIP_LIB=<path>. Every kernel translation
# unit of csrc/hip/ takes the flags (the TB_*_WPE budgets live in several of them), compiled in
# parallel; the runtime layer and the HTML kernels are linked from the default build (build/hip/).
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p build/variants
python3 -c "from textblaster_amd import native; native.build_hip()" > /dev/null
default_units="runtime html"
objs=""
jobs=0
pids=""
for src in csrc/hip/*.hip; do
  unit=$(basename "$src" .hip)
  case " $default_units " in *" $unit "*) objs="$objs build/hip/$unit.hip.o"; continue ;; esac
  obj=build/variants/${unit}_$name.o
  objs="$objs $obj"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -fconstexpr-steps=200000000 "$@" \
    -c "$src" -o "$obj" &
  pids="$pids $!"
  jobs=$((jobs + 1))
  if [ "$jobs" -ge 16 ]; then  # at most 16 compiles at a time
    for p in $pids; do wait "$p"; done
    pids=""; jobs=0
  fi
done
for p in $pids; do wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o textblaster_amd/libtbhip_$name.so $objs
echo textblaster_amd/libtbhip_$name.so
