#!/bin/bash
# usage: build_variant.sh <name> "<EXTRA flags>"   -> <repo>/build_variants/libvr_hip_<name>.so, <name>.log
# The sources, the flags and the rules are csrc/Makefile's (its VARIANT mode); this is the call and the summary line.
set -e
REPO="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
make -s -C "$REPO/volume-rendering_amd/csrc" VARIANT="$1" EXTRA="$2" >&2
grep -A12 "raymarch_kernelILi1ELi1ELi0ELi1" "$REPO/build_variants/$1.log" | grep -E "SGPRs:|VGPRs:|Occupancy|LDS Size" | head -4 | tr '\n' ' '; echo " <- $1"
