#!/bin/bash
# kept for the old name: the measurement build is tools/measure_lib.sh (gemm8 stamps + attention stamps)
exec "$(dirname "$0")/measure_lib.sh" "$@"
