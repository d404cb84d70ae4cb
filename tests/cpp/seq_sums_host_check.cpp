// seq_sums_host_check.cpp -- the library's host loop of the reference-order sums (host_math.hpp track_sums_reference_order) on rows read from a file:
// what tests/test_seq_sums_cpu.py holds the numpy reference of the sequential-sum tests to.  Stand-alone host program (g++ -ffp-contract=off).
//   seq_sums_host_check IN OUT
//   IN : int32 npix, npix x 14 float32 ({J0[6], r0, J1[6], r1} per pixel), npix int32 (pair_t: >= 0 marks the accepted pixels)
//   OUT: for rows_per_pixel 1, then 2: JTJ[36], JTr[6] as float32 and the number of accepted pixels as uint32
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host_math.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    int32_t npix = 0;
    if (!in || std::fread(&npix, 4, 1, in) != 1 || npix < 0) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    std::vector<float> rows((size_t)npix * 14);
    std::vector<int> pair_t((size_t)npix);
    if (std::fread(rows.data(), 4, rows.size(), in) != rows.size() || std::fread(pair_t.data(), 4, pair_t.size(), in) != pair_t.size()) {
        std::fprintf(stderr, "%s is too short\n", argv[1]);
        return 1;
    }
    std::fclose(in);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    for (int rpp = 1; rpp <= 2; ++rpp) {
        float JTJ[36], JTr[6];
        size_t n = 0;
        op_host::track_sums_reference_order(rows.data(), pair_t.data(), (size_t)npix, rpp, JTJ, JTr, &n);
        const uint32_t count = (uint32_t)n;
        if (std::fwrite(JTJ, 4, 36, out) != 36 || std::fwrite(JTr, 4, 6, out) != 6 || std::fwrite(&count, 4, 1, out) != 1) return 1;
    }
    return std::fclose(out) == 0 ? 0 : 1;
}
