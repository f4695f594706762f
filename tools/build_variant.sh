#!/bin/bash
# Build libbmqcrc.so with extra -D flags into
# blazingmq_amd/lib/variant_<name>.so for a same-box A/B (tools/ab_swap.sh swaps it in for a second run).  The product
# build (libbmqcrc.so) is left untouched.  The flags the tree still reads:
# -DBMQCRC_TUNE_BITS=<bits> (csrc/bmqcrc_internal.h lists them) and the two
# timing diagnostics -DBMQCRC_FOLD_DIAG=1 / -DBMQCRC_PLAN_DIAG=3
# (csrc/crc32c_diag.h).  The A/B macros of rounds 2-6 are gone (DESIGN.md
# Appendix A names the last commit that builds them); to compare with such a
# build, build that commit's tree and copy its library here as variant_<name>.so.
#   usage: tools/build_variant.sh <name> -DFOO=1 ...
set -e
cd "$(dirname "$0")/.."
name=$1; shift
python3 - "$name" "$@" <<'PY'
import sys
sys.path.insert(0, '.')
from blazingmq_amd import build
build.build_product(force=True, defines=sys.argv[2:], target_name="variant_%s.so" % sys.argv[1])
PY
ls -la blazingmq_amd/lib/
