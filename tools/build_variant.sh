#!/bin/bash
# Build an alternative libstreamflow_hip with extra -D flags for one source file (A/B of tuning numbers):
#   tools/build_variant.sh NAME corr.hip -DSF_CORR_NSTAGE=3     ->  streamflow_amd/csrc/build/variant_NAME.so
# and run with SF_HIP_LIB=streamflow_amd/csrc/build/variant_NAME.so
# Sources and compile flags are those of streamflow_amd.build: the variant differs from the shipped library by its -D only.
set -e
cd "$(dirname "$0")/.."
name=$1; src=$2; shift 2
B=streamflow_amd/csrc/build
python -m streamflow_amd.build > /dev/null
flags=$(python -c "from streamflow_amd import build; print(' '.join(f for f in build.FLAGS if not f.startswith('-Rpass')))")
sources=$(python -c "from streamflow_amd import build; print(' '.join(build.SOURCES))")
case " $sources " in *" $src "*) ;; *) echo "$src is not one of: $sources" >&2; exit 1;; esac
timeout 600 hipcc $flags "$@" -c streamflow_amd/csrc/$src -o $B/variant_${name}_${src%.hip}.o
objs=""
for f in $sources; do
  if [ "$f" = "$src" ]; then objs="$objs $B/variant_${name}_${src%.hip}.o"; else objs="$objs $B/${f%.hip}.o"; fi
done
hipcc --offload-arch=gfx950 -shared -fPIC $objs -o $B/variant_$name.so
echo $B/variant_$name.so
