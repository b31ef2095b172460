#!/bin/bash
# Builds an experiment variant of libsvbrdf_hip.so into tools/_build/libsvbrdf_<tag>.so: csrc/Makefile's own build (every
# unit, its flags, its link line) with extra flags for every unit (e.g. -DSVBRDF_X=1).  The Makefile takes SCHED_MAIN=...
# SCHED_ADJOINT=... SCHED_ADJOINT_EXTRA=... SCHED_PHOTO=... from the environment.
#   bash tools/build_variant.sh <tag> [extra compiler flags...]
# SRC_DIR=<the csrc/ of a checkout of another revision> builds that revision for a same-box A/B against it; it has to be
# a revision with this layout (a unit per .hip file, LIBDIR overridable), i.e. this one or later.
set -e
tag=$1; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
src=${SRC_DIR:-$root/svbrdf_estimation_amd/csrc}
out=$root/tools/_build
make -C $src -B -j8 LIBDIR=$out/lib_$tag HIPFLAGS="$(make -s -C $src print-HIPFLAGS) $*"
cp $out/lib_$tag/libsvbrdf_hip.so $out/libsvbrdf_$tag.so
echo built $out/libsvbrdf_$tag.so
