#!/bin/bash
# Rebuilds the emulator libraries the check_*.py scripts load (the same commands tests/test_host_logic.py runs): tools/hostemu/build.sh [zstd] [enc] [all] [serial] [emu] [xxh3] [size] [pack] [xxh_stream] [window] [lz4_accel] [snf_params]
# The scripts load whatever library lies there -- after a change to a kernel source, build first.
cd "$(dirname "$0")/../.."
CLANG=$(command -v clang++ || echo /opt/rocm/lib/llvm/bin/clang++)
I="-I tools/hostemu -I include -I aircompressor_amd/csrc"
for t in ${@:-zstd enc all serial emu xxh3 size pack xxh_stream window lz4_accel snf_params}; do
  case $t in
    zstd)   $CLANG -O1 -std=c++17 -fPIC -shared $I -o tools/hostemu/libemu_zstd.so tools/hostemu/emu_zstd.cpp ;;
    enc)    $CLANG -O2 -std=c++17 -fPIC -shared -fno-omit-frame-pointer -fsanitize-coverage=inline-8bit-counters,trace-loads,trace-stores $I -o tools/hostemu/libemu_enc.so tools/hostemu/emu_enc.cpp ;;
    all)    $CLANG -O1 -std=c++17 -fPIC -shared $I -o tools/hostemu/libemu_all.so tools/hostemu/emu_all.cpp ;;
    serial) $CLANG -O1 -std=c++17 -fPIC -shared $I -o tools/hostemu/libemu_serial.so tools/hostemu/emu_serial.cpp ;;
    emu)    $CLANG -O1 -std=c++17 -fPIC -shared $I -o tools/hostemu/libemu.so tools/hostemu/emu.cpp ;;
    xxh3)   $CLANG -O1 -std=c++17 -fPIC -shared $I -o tools/hostemu/libemu_xxh3.so tools/hostemu/emu_xxh3.cpp ;;
    size)   $CLANG -O1 -std=c++17 -fPIC -shared $I -o tools/hostemu/libemu_size.so tools/hostemu/emu_size.cpp ;;
    pack)   $CLANG -O1 -std=c++17 -fPIC -shared $I -o tools/hostemu/libemu_pack.so tools/hostemu/emu_pack.cpp ;;
    window) $CLANG -O1 -std=c++17 -fPIC -shared $I -o tools/hostemu/libemu_window.so tools/hostemu/emu_window.cpp ;;
    lz4_accel) $CLANG -O2 -std=c++17 -fPIC -shared -fno-omit-frame-pointer -fsanitize-coverage=inline-8bit-counters,trace-loads,trace-stores $I -o tools/hostemu/libemu_lz4_accel.so tools/hostemu/emu_lz4_accel.cpp ;;
    snf_params) $CLANG -O2 -std=c++17 -fPIC -shared -fno-omit-frame-pointer -fsanitize-coverage=inline-8bit-counters,trace-loads,trace-stores -DSNF_PARAMS_WRITERS $I -o tools/hostemu/libemu_snf_params_w.so tools/hostemu/emu_snf_params.cpp &&
                $CLANG -O1 -std=c++17 -fPIC -shared $I -o tools/hostemu/libemu_snf_params_r.so tools/hostemu/emu_snf_params.cpp ;;
    xxh_stream) $CLANG -O1 -std=c++17 -fPIC -shared $I -o tools/hostemu/libemu_xxh_stream.so tools/hostemu/emu_xxh_stream.cpp ;;
  esac || exit 1
  echo "built $t"
done
