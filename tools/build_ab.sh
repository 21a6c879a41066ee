#!/usr/bin/env bash
# Build an A/B variant of the product library into a3-reliable-transport_amd/lib/ab/<name>.so
#   tools/build_ab.sh <name> [extra hipcc flags...]      (current source)
#   AB_REV=<git rev> tools/build_ab.sh <name> [flags]    (the kernel sources at a revision)
# The whole library, by the product's own Makefile with -DWTP_AB_BUILD=1 and the extra flags,
# in object and output directories of its own; AB_REV takes the csrc directory of that
# revision.  A variant must export what the product library exports, or this fails.
set -eu
cd "$(dirname "$0")/.."
name="$1"; shift
PKG=$PWD/a3-reliable-transport_amd
SRC=$PKG/csrc
if [ -n "${AB_REV:-}" ]; then
  TMP=$(mktemp -d)
  trap 'rm -rf "$TMP"' EXIT
  git archive "$AB_REV" a3-reliable-transport_amd/csrc | tar -x -C "$TMP"
  SRC=$TMP/a3-reliable-transport_amd/csrc
fi
OUT=$PKG/lib/ab/$name.so
rm -rf "$PKG/build/ab/$name"  # the flags are no prerequisite: never reuse a variant's objects
make -C "$PKG" -j"${AB_JOBS:-8}" CSRC="$SRC" BUILD="$PKG/build/ab/$name" LIB="$OUT" \
  EXTRA_HIPFLAGS="-DWTP_AB_BUILD=1 $*" "$OUT"
make -C "$PKG" -j"${AB_JOBS:-8}" "$PKG/lib/libwtp_crc32.so"
# (__hip_cuid_<hash> marks a compilation with its flags: one per translation unit, never the same)
syms() { nm -D --defined-only "$1" | awk '{print $NF}' | grep -v '^__hip_cuid_' | sort; }
if ! diff <(syms "$PKG/lib/libwtp_crc32.so") <(syms "$OUT"); then
  echo "build_ab: $OUT does not export what lib/libwtp_crc32.so exports (above: product <, variant >)" >&2
  exit 1
fi
echo "built a3-reliable-transport_amd/lib/ab/$name.so"
