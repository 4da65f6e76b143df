#!/bin/bash
# kept under its old name for callers that know it: tools/build_kbench.sh holds the flags and the link set of every harness
exec bash "$(dirname "$0")/build_kbench.sh" mfma
