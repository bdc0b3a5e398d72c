#!/bin/bash
# Builds an A/B variant of libsendslam_orb.so with extra compiler flags: build_variant.sh NAME [-DFLAG=V ...]
# -> send-slam_amd/lib/libexp_NAME.so (git-ignored); run with SENDSLAM_LIB=<that path>.  Sources and flags are the Makefile's.
set -e
R="$(cd "$(dirname "$0")/../.." && pwd)"
NAME="$1"; shift
cd "$R/send-slam_amd"
BASE="$(sed -n 's/^CXXFLAGS = //p' Makefile)"
make -s -B OUT="lib/libexp_$NAME.so" CXXFLAGS="$BASE $*"
echo "$R/send-slam_amd/lib/libexp_$NAME.so"
