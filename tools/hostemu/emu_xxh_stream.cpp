// tools/hostemu/emu_xxh_stream.cpp -- the streaming hashers' kernels (xxhash_stream.hip) under the fiber emulator: reset, the quad update of
// XXH64 / XXH32 (quad_sync is a rendezvous of the quad here), the lane and wavefront updates of XXH3 (wave_sync, ballot and the cross-lane
// sums are rendezvous of the wave) and the digests.  Driven by check_xxh_stream.py.
#include "emu_preamble.h"
#include "../../aircompressor_amd/csrc/xxhash_stream.hip"
extern "C" long long emu_hash_state_size(int32_t algo) { return achip::hash_state_size(algo); }
extern "C" int emu_hash_states_reset(int32_t algo, void* states, int32_t n, uint64_t seed) { return (int)achip::launch_hash_states_reset(algo, states, n, seed, nullptr); }
extern "C" int emu_hash_states_update(int32_t algo, void* states, const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t n)
{
    return (int)achip::launch_hash_states_update(algo, states, srcBase, srcOff, srcLen, n, nullptr);
}
extern "C" int emu_hash_states_digest(int32_t algo, const void* states, int64_t* out, int32_t n) { return (int)achip::launch_hash_states_digest(algo, states, out, n, nullptr); }
