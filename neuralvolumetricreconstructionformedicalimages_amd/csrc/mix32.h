// mix32.h -- the "lowbias32" integer finaliser behind every counter-based draw of the library: the ray jitter (naf_device.h), the
// Feistel permutation of the ray draw (draw_device.h) and the point draw of the volume sampler (volume_sample_device.h).  It
// includes nothing of HIP, so a host compiler reads it too.
#pragma once

#include <cstdint>

#include "host_device.h"

namespace naf {

NAF_HD uint32_t mix32(uint32_t h) {
    h ^= h >> 16; h *= 0x7feb352du;
    h ^= h >> 15; h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

}  // namespace naf
