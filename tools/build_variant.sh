#!/bin/bash
# Build libexa_raster from the csrc/ + include/ of a git revision into exavatar_release_amd/_variants/<name>.so
# (same flags as exavatar_release_amd/build.py), for A/B runs with EXA_RASTER_LIB on the GPU box.
# Usage: bash tools/build_variant.sh <git-rev> <name> [extra hipcc flags...]
set -e
REV=$1; NAME=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
mkdir -p $T/exavatar_release_amd/csrc $T/include $ROOT/exavatar_release_amd/_variants
if [ "$REV" = WORK ]; then      # the working tree (e.g. with -D flags that select an experimental code path)
  cp $ROOT/exavatar_release_amd/csrc/* $T/exavatar_release_amd/csrc/; cp $ROOT/include/exa_*.h $T/include/
else
  for f in $(git -C $ROOT ls-tree --name-only $REV exavatar_release_amd/csrc/); do git -C $ROOT show $REV:$f > $T/$f; done
  for h in $(git -C $ROOT ls-tree --name-only $REV include/); do git -C $ROOT show $REV:$h > $T/$h; done
fi
OBJS=""
# every .hip of the revision (the library must export what _lib.load() looks up), with the per-file flags of the working
# tree's build.py; at most 16 compilers at a time, and a failed compile ends the script
FPOFF=$(python3 - "$ROOT/exavatar_release_amd/build.py" <<'PY'
import importlib.util, sys
spec = importlib.util.spec_from_file_location('b', sys.argv[1]); b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
print(' '.join(n[:-4] for n, x in b.SOURCES.items() if '-ffp-contract=off' in x))
PY
)
PIDS=""; N=0
for f in $T/exavatar_release_amd/csrc/*.hip; do
  src=$(basename $f .hip)
  X=""; case " $FPOFF " in *" $src "*) X="-ffp-contract=off";; esac
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -fno-slp-vectorize -w $X "$@" -c $f -o $T/$src.o &
  PIDS="$PIDS $!"; OBJS="$OBJS $T/$src.o"; N=$((N + 1))
  if [ $N -ge 16 ]; then for p in $PIDS; do wait $p; done; PIDS=""; N=0; fi
done
for p in $PIDS; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/exavatar_release_amd/_variants/$NAME.so $OBJS
rm -rf $T
echo $ROOT/exavatar_release_amd/_variants/$NAME.so
