// siddon_host_check.cpp -- walks the rays of a file through csrc/siddon_device.h on the CPU, so that the traversal can be compared
// with float64 and run under AddressSanitizer / UBSan (tools/siddon_host_check.py builds and drives it).  The
// volume is a heap block of exactly n1 * n2 * n3 floats, so the sanitizer sees any load outside it.  The kernels' own ray generation
// and tiling in csrc/siddon.hip are not compiled into this program; only the GPU tests cover them.  No GPU, no HIP.
//
//   siddon_host_check n1 n2 n3 dv1 dv2 dv3 n_rays volume.f32 rays.f32 out.f32
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../neuralvolumetricreconstructionformedicalimages_amd/csrc/siddon_device.h"

namespace {

bool read_all(const char *path, float *v, size_t n) {
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return false;
    const size_t got = std::fread(v, sizeof(float), n, fp);
    std::fclose(fp);
    return got == n;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 11) {
        std::fprintf(stderr, "usage: siddon_host_check n1 n2 n3 dv1 dv2 dv3 n_rays volume.f32 rays.f32 out.f32\n");
        return 2;
    }
    const uint32_t n1 = (uint32_t)std::atoi(argv[1]), n2 = (uint32_t)std::atoi(argv[2]), n3 = (uint32_t)std::atoi(argv[3]);
    const float dvoxel[3] = {std::strtof(argv[4], nullptr), std::strtof(argv[5], nullptr), std::strtof(argv[6], nullptr)};
    const size_t n_rays = (size_t)std::atoll(argv[7]), n_vox = (size_t)n1 * n2 * n3;
    if (n_vox == 0 || n_rays == 0) return 2;
    std::unique_ptr<float[]> volume(new float[n_vox]), rays(new float[n_rays * 8]), out(new float[n_rays]);
    if (!read_all(argv[8], volume.get(), n_vox) || !read_all(argv[9], rays.get(), n_rays * 8)) {
        std::fprintf(stderr, "siddon_host_check: short read\n");
        return 2;
    }
    naf::SiddonGrid grid;
    naf::siddon_grid(n1, n2, n3, dvoxel, &grid);
    const float *data = volume.get();
    for (size_t i = 0; i < n_rays; ++i) {
        const float *r = rays.get() + i * 8;
        out[i] = naf::siddon_line_integral(grid, r, r + 3, r[6], r[7], [data](uint64_t offset) { return data[offset]; });
    }
    FILE *fp = std::fopen(argv[10], "wb");
    if (!fp || std::fwrite(out.get(), sizeof(float), n_rays, fp) != n_rays) return 2;
    std::fclose(fp);
    return 0;
}
