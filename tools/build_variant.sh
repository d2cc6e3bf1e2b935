#!/bin/bash
# tools/build_variant.sh NAME FLAGS...: the engine built with extra compile flags into tools/variants/liblightning_amd_NAME.so
# (run the bench against it with LAMD_LIB_PATH; the shipped library and its stamps are not touched).  The translation units and their
# flags are those of lightning_amd/_build.py.
set -eu
cd "$(dirname "$0")/.."
python3 -m lightning_amd._build variant "$@"
ls -la "tools/variants/liblightning_amd_$1.so"
