// siddon_host_check.cpp -- runs the two walks of csrc/siddon_device.h (siddon_forward and siddon_transpose: include/naf_hip.h P6, P7
// and P8, DESIGN.md sections 20 to 22) on the CPU over the rays of a file, so that they can be compared with float64 and run under
// AddressSanitizer / UBSan (tools/siddon_host_check.py builds and drives it).  Every volume is a heap block of exactly n1 * n2 * n3
// floats, so the sanitizer sees any load or add outside it.
//
// Every comparison is made against one restatement of the walk that shares nothing with the grouped loops: a plain loop over
// siddon_span / siddon_begin / siddon_step that records (offset, len) per step, run for the trip count rounded up to whole groups
// (the grouped walk multiplies the exit voxel by the zero lengths of its padding, which is no no-op on an Inf or NaN voxel).
// Per ray it checks, bit for bit:
//   forward           the kind is siddon_span's; acc is the sequential fp32 sum of volume[offset] * len over the restated steps (0
//                     unless the span is ok);
//   forward with row  the same kind and acc, row the sequential sum of len, and row the plain walk's acc on a volume of ones;
//   value deposit     wanted() is y != 0; the (offset, len) it is called with are, in order, the restated steps of positive length
//                     (so the sent terms are y * len), and it is not called at all for y == 0, an empty or a non-finite span;
//   pair deposit      with a den: wanted() whatever y is, called with the same steps, y == 0 included; without a den: wanted() is
//                     y != 0, called with the same steps, and nothing reaches den.
// The deposits here record what siddon_transpose calls them with and add as csrc/projector_pair.h's do (den before num); the device
// deposits themselves, the kernels' ray generation and their tiling are not compiled into this program: the GPU tests cover them.
// No GPU, no HIP.
//
//   siddon_host_check n1 n2 n3 dv1 dv2 dv3 n_rays volume.f32 start.f32 rays.f32 values.f32 acc.f32 value_out.f32 num_out.f32 den_out.f32
// writes P6's result per ray (NaN for a non-finite span), start + the value deposits, and num and den from zero; prints
// "value <terms> num <terms> den <terms> mismatches <count>" and exits 1 on any mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../neuralvolumetricreconstructionformedicalimages_amd/csrc/siddon_device.h"
#include "host_check.h"

using namespace host_check;

namespace {

struct Term {
    uint64_t offset;
    float value;
};

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

size_t differences(const std::vector<Term> &a, const std::vector<Term> &b) {
    if (a.size() != b.size()) return 1;
    size_t n = 0;
    for (size_t k = 0; k < a.size(); ++k)
        if (a[k].offset != b[k].offset || !same_bits(a[k].value, b[k].value)) ++n;
    return n;
}

// The restatement: every step of the ray, ungrouped, for the padded trip count.  Nothing for a span that is not ok.
naf::SiddonKind restate(const naf::VoxelGrid &grid, const naf::SiddonRay &ray, std::vector<Term> &steps) {
    steps.clear();
    naf::SiddonSpan span;
    const naf::SiddonKind kind = naf::siddon_span(grid, ray.o, ray.d, ray.near, ray.far, span);
    if (kind != naf::kSiddonOk) return kind;
    naf::SiddonWalk walk;
    const uint32_t n = naf::siddon_begin(grid, span, walk);
    const uint32_t padded = (n + naf::kSiddonGroup - 1u) / naf::kSiddonGroup * naf::kSiddonGroup;
    for (uint32_t k = 0; k < padded; ++k) {
        uint64_t offset;
        float ds;
        naf::siddon_step(grid, span, walk, offset, ds);
        steps.push_back(Term{offset, ds * span.dn});
    }
    return kind;
}

// The deposits: csrc/projector_pair.h's rules with `+=` for the atomic, and a record of every call.
struct ValueDeposit {
    float *volume;
    float y;
    std::vector<Term> *called;
    bool wanted() const { return y != 0.0f; }
    void operator()(uint64_t offset, float len) const {
        called->push_back(Term{offset, len});
        volume[offset] += y * len;
    }
};

struct PairDeposit {
    float *num, *den;                                         // den may be null
    float y;
    std::vector<Term> *called;
    bool wanted() const { return y != 0.0f || den; }
    void operator()(uint64_t offset, float len) const {
        called->push_back(Term{offset, len});
        if (den) den[offset] += len;
        if (y != 0.0f) num[offset] += y * len;
    }
};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 16)
        return usage(argv[0], "n1 n2 n3 dv1 dv2 dv3 n_rays volume.f32 start.f32 rays.f32 values.f32 acc.f32 value_out.f32 num_out.f32 "
                              "den_out.f32");
    const uint32_t n1 = (uint32_t)std::atoi(argv[1]), n2 = (uint32_t)std::atoi(argv[2]), n3 = (uint32_t)std::atoi(argv[3]);
    const float dvoxel[3] = {std::strtof(argv[4], nullptr), std::strtof(argv[5], nullptr), std::strtof(argv[6], nullptr)};
    const size_t n_rays = (size_t)std::atoll(argv[7]), n_vox = (size_t)n1 * n2 * n3;
    if (n_vox == 0 || n_rays == 0) return kBadArguments;
    std::unique_ptr<float[]> volume(new float[n_vox]), ones(new float[n_vox]), value_out(new float[n_vox]);
    std::unique_ptr<float[]> num(new float[n_vox]()), den(new float[n_vox]()), num_alone(new float[n_vox]());
    std::unique_ptr<float[]> rays(new float[n_rays * 8]), values(new float[n_rays]), acc_out(new float[n_rays]);
    if (!read_all(argv[8], volume.get(), n_vox) || !read_all(argv[9], value_out.get(), n_vox) ||
        !read_all(argv[10], rays.get(), n_rays * 8) || !read_all(argv[11], values.get(), n_rays))
        return kIoFailure;
    for (size_t i = 0; i < n_vox; ++i) ones[i] = 1.0f;
    const naf::VoxelGrid grid = naf::voxel_grid(n1, n2, n3, dvoxel);
    const float *data = volume.get(), *one = ones.get();
    size_t value_total = 0, num_total = 0, den_total = 0, mismatches = 0;
    std::vector<Term> steps, positive, none, called;
    for (size_t i = 0; i < n_rays; ++i) {
        const float *r = rays.get() + i * 8;
        const naf::SiddonRay ray{{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, r[6], r[7]};
        const float y = values[i];
        const naf::SiddonKind kind = restate(grid, ray, steps);
        float acc_want = 0.0f, row_want = 0.0f;
        positive.clear();
        for (const Term &s : steps) {
            acc_want += data[s.offset] * s.value;
            row_want += s.value;
            if (s.value > 0.0f) positive.push_back(s);
        }
        // the forward walk, plain and with the row sum
        naf::SiddonIntegral plain, on_ones;
        naf::SiddonIntegralAndRow both;
        const auto load = [data](uint64_t offset) { return data[offset]; };
        if (naf::siddon_forward(grid, ray, load, plain) != kind || !same_bits(plain.acc, acc_want)) ++mismatches;
        if (naf::siddon_forward(grid, ray, load, both) != kind || !same_bits(both.acc, acc_want) || !same_bits(both.row, row_want))
            ++mismatches;
        if (naf::siddon_forward(grid, ray, [one](uint64_t offset) { return one[offset]; }, on_ones) != kind ||
            !same_bits(both.row, on_ones.acc))
            ++mismatches;
        acc_out[i] = kind == naf::kSiddonNotFinite ? __builtin_nanf("") : plain.acc;
        // the transpose walk: a deposit that declines is never called, one that accepts sees the steps of positive length
        const std::vector<Term> &if_y = y != 0.0f ? positive : none;
        called.clear();
        naf::siddon_transpose(grid, ray, ValueDeposit{value_out.get(), y, &called});
        mismatches += differences(called, if_y);
        value_total += called.size();
        called.clear();
        naf::siddon_transpose(grid, ray, PairDeposit{num.get(), den.get(), y, &called});
        mismatches += differences(called, positive);
        den_total += called.size();
        num_total += y != 0.0f ? called.size() : 0;
        called.clear();
        naf::siddon_transpose(grid, ray, PairDeposit{num_alone.get(), nullptr, y, &called});
        mismatches += differences(called, if_y);
    }
    // with and without a den the numerator got the same terms in the same order
    if (std::memcmp(num.get(), num_alone.get(), n_vox * sizeof(float)) != 0) ++mismatches;
    if (!write_all(argv[12], acc_out.get(), n_rays) || !write_all(argv[13], value_out.get(), n_vox) ||
        !write_all(argv[14], num.get(), n_vox) || !write_all(argv[15], den.get(), n_vox))
        return kIoFailure;
    std::printf("value %zu num %zu den %zu mismatches %zu\n", value_total, num_total, den_total, mismatches);
    return mismatches ? 1 : 0;
}
