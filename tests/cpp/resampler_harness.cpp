// resampler_harness.cpp -- DAB_Resampler (dab-radio_amd/host/dab/tx/dab_resampler.h) driven from a file, for
// tests/test_gpu_resample_class.py (built by build()):
//   resampler_harness <params.bin> <in.c64> <out.bin> <wrap 0|1> <seek> <u8_scale, 0 = complex float> <n_out> [<n_out> ...]
// params.bin = one dabgpu_resample_stream; the calls' outputs are written back to back (odd lengths: unaligned spans into one vector).
// Prints the design error and, per call, the input span InputNeeded reports.
#include <cstdio>
#include <cstdlib>
#include <complex>
#include <vector>

#include "dab/tx/dab_resampler.h"

static std::vector<char> slurp(const char* path) {
    std::vector<char> v;
    FILE* fp = fopen(path, "rb");
    if (!fp) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(fp);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: see the source\n"); return 2; }
    try {
        const auto pb = slurp(argv[1]);
        const auto ib = slurp(argv[2]);
        if (pb.size() != sizeof(dabgpu_resample_stream) || ib.size() % 8) { fprintf(stderr, "bad input sizes\n"); return 2; }
        const dabgpu_resample_stream& P = *reinterpret_cast<const dabgpu_resample_stream*>(pb.data());
        const tcb::span<const std::complex<float>> in(reinterpret_cast<const std::complex<float>*>(ib.data()), ib.size() / 8);
        const bool wrap = atoi(argv[4]) != 0;
        const float scale = (float)atof(argv[6]);
        DAB_Resampler rs(P);
        printf("design_error %.9e\n", rs.DesignError());
        if (rs.Apply({}, {}, wrap)) return 3;                              // an empty input is refused, not run
        rs.Seek(strtoull(argv[5], nullptr, 10));
        FILE* fo = fopen(argv[3], "wb");
        if (!fo) return 2;
        for (int a = 7; a < argc; a++) {
            const size_t n = (size_t)atoll(argv[a]);
            int64_t first; uint64_t count;
            rs.InputNeeded(n, first, count);
            printf("span %lld %llu\n", (long long)first, (unsigned long long)count);
            if (scale == 0.0f) {
                std::vector<std::complex<float>> out(n);
                if (!rs.Apply(out, in, wrap)) return 3;
                fwrite(out.data(), 8, n, fo);
            } else {
                std::vector<uint8_t> out(2 * n);
                if (!rs.ApplyU8(out, in, wrap, scale)) return 3;
                fwrite(out.data(), 2, n, fo);
            }
        }
        fclose(fo);
        printf("position %llu\n", (unsigned long long)rs.Position());
    } catch (const std::exception& ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
