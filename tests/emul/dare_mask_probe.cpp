// dare_mask_probe.cpp - the mask helper of csrc/sm_dare.hpp (dare_mask8) at arbitrary 64-bit element indices, the
// counter's high word included, which no tensor of a test can reach (TEST INFRASTRUCTURE; built by tests/test_dare_host.py).
#include "../../shardmerge_amd/csrc/sm_dare.hpp"

extern "C" void dare_mask_probe(uint64_t key, uint32_t stream_id, uint32_t T, const uint64_t* j, int count, uint8_t* keep) {
    for (int i = 0; i < count; ++i) keep[i] = (uint8_t)((smhip::dare_mask8(key, stream_id, j[i], T) >> (j[i] & 7)) & 1u);
}
