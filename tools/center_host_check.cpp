// center_host_check.cpp -- runs the per-pixel arithmetic of csrc/center_device.h on the CPU under AddressSanitizer / UBSan
// (tools/center_host_check.py builds and drives it) and writes what it computed for the driver to compare with
// the numpy oracle.  Every filtered row lives on the heap in a vector of exactly W floats, so a read one element outside is a
// sanitizer report.  The kernel's LDS staging and launch geometry are not compiled into this program; only the GPU tests cover
// them.  No GPU, no HIP.  Floats travel as the decimal uint32 of their float32 bits.
//
//   center_host_check slices S N W K n parallel DSO DSD du ou dx dy ox oy q.f32 trig.f32 cand.f32 f.f32(out)
//   center_host_check metrics K n dx dy r f.f32 out.f64(out)
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../neuralvolumetricreconstructionformedicalimages_amd/csrc/center_device.h"
#include "host_check.h"

using namespace host_check;

namespace {

uint32_t number(const char *text) { return (uint32_t)std::strtoul(text, nullptr, 10); }
float real(const char *text) { return __builtin_bit_cast(float, number(text)); }

}  // namespace

int main(int argc, char **argv) {
    if (argc == 20 && !std::strcmp(argv[1], "slices")) {
        const uint32_t S = number(argv[2]), N = number(argv[3]), W = number(argv[4]), K = number(argv[5]), n = number(argv[6]);
        const int parallel = (int)number(argv[7]);
        const float DSO = real(argv[8]), DSD = real(argv[9]), du = real(argv[10]), ou = real(argv[11]), dx = real(argv[12]),
                    dy = real(argv[13]), ox = real(argv[14]), oy = real(argv[15]);
        if (!S || !N || !W || !K || !n || W > naf::kCenterMaxW || K > naf::kCenterMaxK || n > naf::kCenterMaxN) return kBadArguments;
        std::vector<float> q((size_t)S * N * W), trig(2 * (size_t)N), cand(K), f((size_t)S * K * n * n);
        if (!read_all(argv[16], q) || !read_all(argv[17], trig) || !read_all(argv[18], cand)) return kIoFailure;
        const float inv_du = 1.0f / du, half = 0.5f * (float)W - 0.5f;
        for (uint32_t s = 0; s < S; ++s) {
            std::vector<std::vector<float>> rows;                           // exactly the row, one heap block each
            for (uint32_t i = 0; i < N; ++i) rows.emplace_back(q.begin() + ((size_t)s * N + i) * W, q.begin() + ((size_t)s * N + i + 1) * W);
            for (uint32_t k0 = 0; k0 < K; k0 += naf::kCenterGroup) {
                const uint32_t count = std::min(naf::kCenterGroup, K - k0);
                float shift[naf::kCenterGroup] = {};
                for (uint32_t j = 0; j < count; ++j) shift[j] = cand[k0 + j] / du;
                for (uint32_t ix = 0; ix < n; ++ix)
                    for (uint32_t iy = 0; iy < n; ++iy) {
                        float acc[naf::kCenterGroup] = {};
                        const float x = naf::center_coord(ix, n, dx, ox), y = naf::center_coord(iy, n, dy, oy);
                        for (uint32_t i = 0; i < N; ++i) {
                            const naf::CenterTerm term = naf::center_term(parallel, x, y, trig[2 * i], trig[2 * i + 1], DSO, DSD, ou, inv_du, half);
                            naf::center_accumulate(acc, shift, count, rows[i].data(), W, term);
                        }
                        for (uint32_t j = 0; j < count; ++j) f[(((size_t)s * K + k0 + j) * n + ix) * n + iy] = acc[j];
                    }
            }
        }
        return write_all(argv[19], f) ? 0 : kIoFailure;
    }
    if (argc == 9 && !std::strcmp(argv[1], "metrics")) {
        const uint32_t K = number(argv[2]), n = number(argv[3]);
        const double dx = real(argv[4]), dy = real(argv[5]), r = real(argv[6]);
        if (!K || !n || n > naf::kCenterMaxN) return kBadArguments;
        std::vector<float> f((size_t)K * n * n);
        std::vector<double> out(2 * (size_t)K, 0.0);
        if (!read_all(argv[7], f)) return kIoFailure;
        for (uint32_t k = 0; k < K; ++k) {
            const std::vector<float> img(f.begin() + (size_t)k * n * n, f.begin() + (size_t)(k + 1) * n * n);
            for (uint32_t ix = 0; ix < n; ++ix)
                for (uint32_t iy = 0; iy < n; ++iy) {
                    if (!naf::center_in_mask(ix, iy, n, dx, dy, r)) continue;
                    const size_t p = (size_t)ix * n + iy;
                    out[2 * k] += naf::center_negativity(img[p]);
                    if (ix + 1 < n && naf::center_in_mask(ix + 1, iy, n, dx, dy, r)) out[2 * k + 1] += naf::center_step(img[p], img[p + n]);
                    if (iy + 1 < n && naf::center_in_mask(ix, iy + 1, n, dx, dy, r)) out[2 * k + 1] += naf::center_step(img[p], img[p + 1]);
                }
        }
        return write_all(argv[8], out) ? 0 : kIoFailure;
    }
    return usage(argv[0], "slices S N W K n parallel DSO DSD du ou dx dy ox oy q trig cand f | metrics K n dx dy r f out");
}
