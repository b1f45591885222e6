#!/bin/bash
# Builds syzkaller_amd/exp/lib$1.so: the whole library compiled under extra
# defines ($2, e.g. "-DSG_PT=8192 -DSG_FU=2"), for the A/B scripts
# (SG_LIB_PATH).  Every source sees the defines (objects under build_exp/$1),
# so a geometry knob cannot reach one stage only; the stock build is untouched.
set -e
make -s -C "$(dirname "$0")/../syzkaller_amd" ARCH=gfx950 BUILD="../build_exp/$1" LIB="exp/lib$1.so" \
  EXTRA_CXXFLAGS="$2"
