// frames_host_check.cpp -- runs the per-pixel arithmetic of csrc/frames_device.h on the CPU and compares it with files the numpy oracle
// wrote, under AddressSanitizer / UBSan (tools/frames_host_check.py builds and drives it).  Every window lives
// on the heap in a vector of exactly size * size words, so a read one element outside is a sanitizer report.  The kernel's LDS
// staging and launch geometry are not compiled into this program; only the GPU tests cover them.  No GPU, no HIP.  Exit 0: everything
// equal; 1 beside a line that names the difference.  `dif` and `t_min` travel as the decimal uint32 of their float32 bits.
//
//   frames_host_check words n u16 raw.f32|raw.u16 dark.f32 flat.f32 marked.u8 want.u32       frames_transmission of n pixels; u16: 1 for uint16 raw
//   frames_host_check decide size N H W dif words.u32 want.u32 counts.u32                     reflected windows, frames_decide
//   frames_host_check tail n t_min flags t.f32 out.f32                                        frames_tail, written for the driver
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../neuralvolumetricreconstructionformedicalimages_amd/csrc/frames_device.h"
#include "host_check.h"

using namespace host_check;

namespace {

int differs(const char *what, size_t at, unsigned long long got, unsigned long long want) {
    std::printf("%s differs at %zu: %llu, the oracle has %llu\n", what, at, got, want);
    return 1;
}

uint32_t number(const char *text) { return (uint32_t)std::strtoul(text, nullptr, 10); }

template <uint32_t kSize>
int decide(uint32_t N, uint32_t H, uint32_t W, float dif, const std::vector<uint32_t> &words, const std::vector<uint32_t> &want,
           const std::vector<uint32_t> &want_counts) {
    constexpr int32_t h = kSize / 2;
    for (uint32_t i = 0; i < N; ++i) {
        uint32_t outliers = 0, bads = 0;
        for (uint32_t v = 0; v < H; ++v)
            for (uint32_t u = 0; u < W; ++u) {
                std::vector<uint32_t> window(kSize * kSize);                                     // exactly the window
                for (int32_t a = -h; a <= h; ++a)
                    for (int32_t b = -h; b <= h; ++b)
                        window[(a + h) * kSize + (b + h)] =
                            words.at(((size_t)i * H + naf::stripe_reflect((int32_t)v + a, H)) * W + naf::stripe_reflect((int32_t)u + b, W));
                const uint32_t got = naf::frames_bits(naf::frames_decide<kSize>(window.data(), kSize, dif, outliers, bads));
                const size_t at = ((size_t)i * H + v) * W + u;
                if (got != want[at]) return differs("repaired transmission", at, got, want[at]);
            }
        if (outliers != want_counts[2 * i]) return differs("outlier count", i, outliers, want_counts[2 * i]);
        if (bads != want_counts[2 * i + 1]) return differs("bad count", i, bads, want_counts[2 * i + 1]);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 9 && !std::strcmp(argv[1], "words")) {
        const size_t n = std::strtoul(argv[2], nullptr, 10);
        const bool u16 = number(argv[3]) != 0;
        std::vector<float> raw32(u16 ? 0 : n), dark(n), flat(n);
        std::vector<uint16_t> raw16(u16 ? n : 0);
        std::vector<uint8_t> marked(n);
        std::vector<uint32_t> want(n);
        if (!(u16 ? read_all(argv[4], raw16) : read_all(argv[4], raw32)) || !read_all(argv[5], dark) || !read_all(argv[6], flat) ||
            !read_all(argv[7], marked) || !read_all(argv[8], want))
            return kIoFailure;
        for (size_t i = 0; i < n; ++i) {
            const float x = u16 ? naf::frames_load(raw16.data(), i) : naf::frames_load(raw32.data(), i);
            const uint32_t got = naf::frames_transmission(x, dark[i], flat[i], marked[i] != 0);
            if (got != want[i]) return differs("window word", i, got, want[i]);
        }
        return 0;
    }
    if (argc == 10 && !std::strcmp(argv[1], "decide")) {
        const uint32_t size = number(argv[2]), N = number(argv[3]), H = number(argv[4]), W = number(argv[5]);
        const float dif = naf::frames_float(number(argv[6]));
        if (size > H || size > W || N == 0) return kBadArguments;
        const size_t n = (size_t)N * H * W;
        std::vector<uint32_t> words(n), want(n), want_counts(2 * (size_t)N);
        if (!read_all(argv[7], words) || !read_all(argv[8], want) || !read_all(argv[9], want_counts)) return kIoFailure;
        if (size == 3) return decide<3>(N, H, W, dif, words, want, want_counts);
        if (size == 5) return decide<5>(N, H, W, dif, words, want, want_counts);
        if (size == 7) return decide<7>(N, H, W, dif, words, want, want_counts);
        return kBadArguments;
    }
    if (argc == 7 && !std::strcmp(argv[1], "tail")) {
        const size_t n = std::strtoul(argv[2], nullptr, 10);
        const float t_min = naf::frames_float(number(argv[3]));
        const uint32_t flags = number(argv[4]);
        std::vector<float> t(n), out(n);
        if (!read_all(argv[5], t)) return kIoFailure;
        for (size_t i = 0; i < n; ++i) out[i] = naf::frames_tail(t[i], t_min, flags);
        return write_all(argv[6], out) ? 0 : kIoFailure;
    }
    return usage(argv[0], "words n u16 raw dark flat marked want | decide size N H W dif words want counts | tail n t_min flags t out");
}
