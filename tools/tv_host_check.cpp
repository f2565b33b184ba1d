// tv_host_check.cpp -- runs the per-voxel arithmetic of csrc/tv_device.h on the CPU, so that it can be compared with the float64
// oracle and run under AddressSanitizer / UBSan (tools/tv_host_check.py builds and drives it).  The 13 values
// and the edge flags of every voxel are gathered here by a plain loop over flat indices: the kernel's LDS staging, halo and slot
// indexing in csrc/tv.hip are not compiled into this program, and only the GPU tests cover them.  No GPU, no HIP.
//
//   tv_host_check gradient n1 n2 n3 eps in.f32 grad.f32            writes g, prints "TV sum_g2"
//   tv_host_check descent  n1 n2 n3 eps step n_steps in.f32 out.f32   writes the volume after n_steps, prints the last step's sums
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../neuralvolumetricreconstructionformedicalimages_amd/csrc/tv_device.h"
#include "host_check.h"

using namespace host_check;

namespace {

struct Sums {
    double tv, g2;
};

// g of every voxel in volume order; the fp64 sums are taken in volume order too (the kernel's tree adds them in another order).
Sums gradient(const std::vector<float> &f, uint32_t n1, uint32_t n2, uint32_t n3, float eps, std::vector<float> &g) {
    const uint64_t s0 = (uint64_t)n2 * n3, s1 = n3, stride[3] = {s0, s1, 1};
    const uint32_t n[3] = {n1, n2, n3};
    Sums sums = {0.0, 0.0};
    for (uint32_t x = 0; x < n1; ++x)
        for (uint32_t y = 0; y < n2; ++y)
            for (uint32_t z = 0; z < n3; ++z) {
                const uint32_t v[3] = {x, y, z};
                const uint64_t at = x * s0 + y * s1 + z;
                naf::TvStencil st;
                st.c = f.at(at);
                for (int a = 0; a < 3; ++a) {
                    st.has_lo[a] = v[a] > 0;
                    st.has_hi[a] = v[a] + 1 < n[a];
                    st.lo[a] = st.has_lo[a] ? f.at(at - stride[a]) : 0.0f;
                    st.hi[a] = st.has_hi[a] ? f.at(at + stride[a]) : 0.0f;
                }
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b)
                        st.diag[a][b] = (a != b && st.has_hi[a] && st.has_lo[b]) ? f.at(at + stride[a] - stride[b]) : 0.0f;
                float m;
                const float gv = naf::tv_point(st, eps, &m);
                g.at(at) = gv;
                sums.tv += (double)m;
                sums.g2 += (double)gv * (double)gv;
            }
    return sums;
}

}  // namespace

int main(int argc, char **argv) {
    const bool grad = argc == 8 && !std::strcmp(argv[1], "gradient");
    const bool desc = argc == 10 && !std::strcmp(argv[1], "descent");
    if (!grad && !desc) return usage(argv[0], "gradient n1 n2 n3 eps in out | descent n1 n2 n3 eps step n_steps in out");
    const uint32_t n1 = (uint32_t)std::atoi(argv[2]), n2 = (uint32_t)std::atoi(argv[3]), n3 = (uint32_t)std::atoi(argv[4]);
    const float eps = (float)std::atof(argv[5]);
    if (n1 == 0 || n2 == 0 || n3 == 0 || !(eps > 0.0f)) return kBadArguments;
    std::vector<float> f((size_t)n1 * n2 * n3), g(f.size());
    if (!read_all(argv[grad ? 6 : 8], f)) return kIoFailure;
    Sums s = {0.0, 0.0};
    if (grad) {
        s = gradient(f, n1, n2, n3, eps, g);
        if (!write_all(argv[7], g)) return kIoFailure;
    } else {
        const float step = (float)std::atof(argv[6]);
        const int n_steps = std::atoi(argv[7]);
        for (int i = 0; i < n_steps; ++i) {
            s = gradient(f, n1, n2, n3, eps, g);
            const float scale = naf::tv_step_scale(s.g2, step);
            for (size_t k = 0; k < f.size(); ++k) f[k] = naf::tv_step_apply(f[k], g[k], scale);
        }
        if (!write_all(argv[9], f)) return kIoFailure;
    }
    std::printf("%.17g %.17g\n", s.tv, s.g2);
    return 0;
}
