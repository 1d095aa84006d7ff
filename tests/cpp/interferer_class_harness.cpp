// interferer_class_harness.cpp -- DAB_Interferer (dab-radio_amd/host/dab/tx/dab_interferer.h) driven from files, block by block, for
// tests/test_gpu_interferer_class.py (built by build()):
//   interferer_class_harness <params.bin> <shapes.bin> <in.c64 | -> <out.bin> <seek> <u8_scale, 0 = complex float> <n> [<n> ...]
// params.bin = one dabgpu_interferer_stream, shapes.bin = 0..4 dabgpu_interferer_shape; block k takes the next n samples of the input
// ("-": no input, the interferer alone); the blocks' outputs are written back to back.  A block of 0 samples first tries sizes that differ.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <complex>
#include <vector>

#include "dab/tx/dab_interferer.h"

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
        const auto sb = slurp(argv[2]);
        const bool alone = strcmp(argv[3], "-") == 0;
        const auto ib = alone ? std::vector<char>() : slurp(argv[3]);
        if (pb.size() != sizeof(dabgpu_interferer_stream) || sb.size() % sizeof(dabgpu_interferer_shape) || ib.size() % 8) { fprintf(stderr, "bad input sizes\n"); return 2; }
        const dabgpu_interferer_stream& P = *reinterpret_cast<const dabgpu_interferer_stream*>(pb.data());
        const tcb::span<const dabgpu_interferer_shape> shapes(reinterpret_cast<const dabgpu_interferer_shape*>(sb.data()), sb.size() / sizeof(dabgpu_interferer_shape));
        const std::complex<float>* in = reinterpret_cast<const std::complex<float>*>(ib.data());
        const float scale = (float)atof(argv[6]);
        DAB_Interferer itf(P, shapes);
        {   // sizes that differ are refused, not run
            std::vector<std::complex<float>> a(4), b(3);
            std::vector<uint8_t> c(7);
            if (itf.Apply(a, b) || itf.ApplyU8(c, {}, 1.0f) || itf.ApplyU8({c.data(), 6}, a, 1.0f)) return 3;
        }
        itf.Seek(strtoull(argv[5], nullptr, 10));
        FILE* fo = fopen(argv[4], "wb");
        if (!fo) return 2;
        size_t at = 0;
        for (int a = 7; a < argc; a++) {
            const size_t n = (size_t)atoll(argv[a]);
            if (!alone && at + n > ib.size() / 8) { fprintf(stderr, "input too short\n"); return 2; }
            const tcb::span<const std::complex<float>> x = alone ? tcb::span<const std::complex<float>>() : tcb::span<const std::complex<float>>(in + at, n);
            if (scale == 0.0f) {
                std::vector<std::complex<float>> out(n);
                if (!itf.Apply(out, x)) return 3;
                fwrite(out.data(), 8, n, fo);
            } else {
                std::vector<uint8_t> out(2 * n);
                if (!itf.ApplyU8(out, x, scale)) return 3;
                fwrite(out.data(), 2, n, fo);
            }
            at += n;
        }
        fclose(fo);
    } catch (const std::exception& ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
