#!/bin/bash
# VGPR / SGPR / LDS / scratch of the kernels of one unit (gfx950), from the
# compiler's resource-usage remarks.  CPU only.
#   usage: [UNIT=crc32c_kernels] [FILTER='k_fold|k_plan'] tools/kernel_resources.sh [extra hipcc flags]
#   e.g.   UNIT=crc32c_put_pack FILTER=k_pack tools/kernel_resources.sh
cd "$(dirname "$0")/.."
UNIT=${UNIT:-crc32c_kernels}
FILTER=${FILTER:-k_fold|k_plan}
/opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 --offload-device-only -O3 -std=c++17 \
    -Iinclude -c blazingmq_amd/csrc/$UNIT.hip -o /tmp/bmqcrc_res.o \
    -Rpass-analysis=kernel-resource-usage "$@" 2>&1 |
    grep -E "Function Name|VGPRs:|AGPRs|ScratchSize|Occupancy|LDS Size" |
    sed -e 's/.*remark: //' | paste - - - - - - | grep -E "$FILTER"
