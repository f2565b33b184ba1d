// host_check.h -- what the stand-alone programs tools/*_host_check.cpp share: reading and writing a file of exactly n elements, and
// the exit codes tools/host_check.py sees.  A program's own arithmetic loops and its argument layout stay in its .cpp.  No GPU, no HIP.
#pragma once

#include <cstddef>
#include <cstdio>
#include <vector>

namespace host_check {

// Exit codes: 0 for success, kBadArguments, kIoFailure (a file that cannot be opened, is too short or cannot be written); a
// program's own findings take the codes from 4 on, or 1 beside a line of output that names them.
constexpr int kBadArguments = 2, kIoFailure = 3;

// Prints "usage: <program> <forms>" and returns kBadArguments: `return host_check::usage(argv[0], "...")`.
inline int usage(const char *program, const char *forms) {
    std::fprintf(stderr, "usage: %s %s\n", program, forms);
    return kBadArguments;
}

// Exactly n elements from the start of a file; false if it cannot be opened or holds fewer.
template <typename T>
bool read_all(const char *path, T *v, size_t n) {
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return false;
    const size_t got = n ? std::fread(v, sizeof(T), n, fp) : 0;
    std::fclose(fp);
    return got == n;
}

template <typename T>
bool write_all(const char *path, const T *v, size_t n) {
    FILE *fp = std::fopen(path, "wb");
    if (!fp) return false;
    const size_t put = n ? std::fwrite(v, sizeof(T), n, fp) : 0;
    return std::fclose(fp) == 0 && put == n;
}

// The same over a vector that already has the size to read or write.
template <typename T>
bool read_all(const char *path, std::vector<T> &v) { return read_all(path, v.data(), v.size()); }

template <typename T>
bool write_all(const char *path, const std::vector<T> &v) { return write_all(path, v.data(), v.size()); }

}  // namespace host_check
