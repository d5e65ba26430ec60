#!/bin/bash
# Build A/B variants of librt_hip.so HERE (hipcc cross-compiles; the .so files travel with the gpurun snapshot):
#   tools/ab_build.sh name1:"-DFLAG1 -DFLAG2" name2:"-DFLAG3" ...     -> cpuraytracer_amd/lib/exp/librt_hip_<name>.so
# then on the GPU box: tools/ab_run.sh name1 name2 ...  (interleaved timing of the same scene through tools/bench_scene.py)
set -e
cd "$(dirname "$0")/../cpuraytracer_amd/csrc"
mkdir -p ../lib/exp
FLAGS=$(make -pn | sed -n 's/^HIPFLAGS = //p' | head -1 | sed 's/\$(ARCH)/gfx950/')
# the units every variant links beside its own rt_capi object (no variant flags): the denoiser's HIP unit and the host-only ones
REST="rt_denoise rt_scene_prep rt_launch_plan rt_sequence rt_tile_tables rt_denoise_host rt_temporal_host"
for o in $REST; do make ../../build/obj/$o.o; done
RESTOBJS=$(for o in $REST; do echo ../../build/obj/$o.o; done)
for spec in "$@"; do
  name=${spec%%:*}; extra=${spec#*:}; [ "$extra" = "$spec" ] && extra=""
  echo "== $name: $extra"
  # (compile and link apart, as the Makefile does: in one hipcc line the object file after rt_capi.hip is read as HIP source)
  ( /opt/rocm/bin/hipcc $FLAGS $extra -c -o ../../build/obj/rt_capi_$name.o rt_capi.hip &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o ../lib/exp/librt_hip_$name.so ../../build/obj/rt_capi_$name.o $RESTOBJS ) &
done
wait
ls -la ../lib/exp/
