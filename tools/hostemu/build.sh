#!/bin/bash
# Rebuilds emulator libraries from the table of tools/hostemu/emulib.py: tools/hostemu/build.sh [zstd] [enc] [all] [serial] [emu] [xxh3] [size] [pack] [xxh_stream] [window] [lz4_accel] [snf_params] [lz4f_writer] [lzo]
# (all of these when none is named; also enc_stats, lockstep, entropy_unit, unit_oracle_enc).  The check_*.py scripts rebuild a stale library themselves.
exec python3 "$(dirname "$0")/emulib.py" "$@"
