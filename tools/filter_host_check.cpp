// filter_host_check.cpp -- runs the per-output arithmetic of csrc/filter_device.h on the CPU, so that it can be compared with the
// float64 convolution and run under AddressSanitizer / UBSan (tools/filter_host_check.py builds and drives it).
// Every output is formed by a plain loop over the row: the kernel's LDS staging, its padded tap slots and the register window that
// slides the taps in csrc/filter.hip are not compiled into this program, and only the GPU tests cover them.  No GPU, no HIP.
//
//   filter_host_check n_views H W in.f32 taps.f32 pre.f32|- post.f32|- scale.f32|- col.f32|- out.f32
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../neuralvolumetricreconstructionformedicalimages_amd/csrc/filter_device.h"
#include "host_check.h"

using namespace host_check;

namespace {

bool read_optional(const char *path, size_t n, std::vector<float> &v, bool *present) {
    *present = std::strcmp(path, "-") != 0;
    if (!*present) return true;
    v.resize(n);
    return read_all(path, v);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 11) return usage(argv[0], "n_views H W in taps pre|- post|- scale|- col|- out");
    const uint32_t N = (uint32_t)std::atoi(argv[1]), H = (uint32_t)std::atoi(argv[2]), W = (uint32_t)std::atoi(argv[3]);
    if (N == 0 || H == 0 || W == 0) return kBadArguments;
    std::vector<float> in((size_t)N * H * W), taps(W), pre, post, scale, col, out(in.size()), x(W);
    bool has_pre, has_post, has_scale, has_col;
    if (!read_all(argv[4], in) || !read_all(argv[5], taps)) return kIoFailure;
    if (!read_optional(argv[6], (size_t)H * W, pre, &has_pre) || !read_optional(argv[7], (size_t)H * W, post, &has_post) ||
        !read_optional(argv[8], N, scale, &has_scale) || !read_optional(argv[9], (size_t)N * W, col, &has_col))
        return kIoFailure;
    for (uint32_t i = 0; i < N; ++i)
        for (uint32_t r = 0; r < H; ++r) {
            const size_t base = ((size_t)i * H + r) * W, wbase = (size_t)r * W, cbase = (size_t)i * W;
            for (uint32_t k = 0; k < W; ++k)
                x.at(k) = naf::filter_stage(in.at(base + k), has_pre, has_pre ? pre.at(wbase + k) : 1.0f, has_col,
                                            has_col ? col.at(cbase + k) : 1.0f);
            for (uint32_t n = 0; n < W; ++n)
                out.at(base + n) = naf::filter_finish(naf::filter_output(taps.data(), x.data(), W, n), has_post,
                                                      has_post ? post.at(wbase + n) : 1.0f, has_scale, has_scale ? scale.at(i) : 1.0f);
        }
    return write_all(argv[10], out) ? 0 : kIoFailure;
}
