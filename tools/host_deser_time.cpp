// Host baseline of pm_pk_load_bytes (tools/pk_load_time.py): the host mirror's deser_g1 (polymath_amd/host/wire.hpp) on one
// thread over a file of packed 48-byte BLS12-381 records, with validate = 1 and 0.  Prints microseconds per point.
#include <chrono>
#include <cstdio>
#include <fstream>
#include <iterator>
#include "../polymath_amd/host/wire.hpp"

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_deser_time records.bin\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    pmhost::Bytes b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const size_t count = b.size() / 48;
    for (int validate = 1; validate >= 0; --validate) {
        pmhost::Reader rd(b.data(), count * 48);
        size_t inf = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t i = 0; i < count; ++i) inf += pmhost::deser_g1<pm::BlsCurve>(rd, validate != 0).inf;
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("host deser_g1 validate=%d: %zu points, %.1f us/point (%zu at infinity)\n", validate, count, us / count, inf);
    }
    return 0;
}
