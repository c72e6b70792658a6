#!/usr/bin/env bash
# One command, exit code = verdict (0 equal / 1 different / 2 no alleleCounter here): see tools/pin_allelecounter.py.
#   ALLELECOUNTER=/path/to/alleleCounter bash tools/pin_allelecounter.sh
cd "$(dirname "$0")/.."
[ -f clairs_to_amd/libclairsto_amd.so ] || python -c "import __graft_entry__ as g; g.build()" || exit 2
exec python tools/pin_allelecounter.py --allelecounter "${ALLELECOUNTER:-alleleCounter}" "$@"
