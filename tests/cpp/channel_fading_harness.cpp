// channel_fading_harness.cpp -- DAB_Channel_Model::SetFading (dab-radio_amd/host/dab/tx/dab_channel_model.h) driven from files, for
// tests/test_gpu_channel_fading_class.py (built by build()):
//   channel_fading_harness <params.bin> <spec.bin> <in.c64> <out.bin> <wrap 0|1> <seek> <u8_scale, 0 = complex float> <calls before SetFading> <n_out> [<n_out> ...]
// params.bin = one dabgpu_channel_stream, spec.bin = one dabgpu_channel_fading_spec; the calls' outputs are written back to back.  With
// <calls before SetFading> = -1 SetFading is never called: the class of before.
#include <cstdio>
#include <cstdlib>
#include <complex>
#include <vector>

#include "dab/tx/dab_channel_model.h"

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
    if (argc < 10) { fprintf(stderr, "usage: see the source\n"); return 2; }
    try {
        const auto pb = slurp(argv[1]), sb = slurp(argv[2]), ib = slurp(argv[3]);
        if (pb.size() != sizeof(dabgpu_channel_stream) || sb.size() != sizeof(dabgpu_channel_fading_spec) || ib.size() % 8) { fprintf(stderr, "bad input sizes\n"); return 2; }
        const dabgpu_channel_stream& P = *reinterpret_cast<const dabgpu_channel_stream*>(pb.data());
        const dabgpu_channel_fading_spec& S = *reinterpret_cast<const dabgpu_channel_fading_spec*>(sb.data());
        const tcb::span<const std::complex<float>> in(reinterpret_cast<const std::complex<float>*>(ib.data()), ib.size() / 8);
        const bool wrap = atoi(argv[5]) != 0;
        const float scale = (float)atof(argv[7]);
        const int before = atoi(argv[8]);
        DAB_Channel_Model ch(P);
        ch.Seek(strtoull(argv[6], nullptr, 10));
        FILE* fo = fopen(argv[4], "wb");
        if (!fo) return 2;
        for (int a = 9; a < argc; a++) {
            if (a - 9 == before) ch.SetFading(S);
            const size_t n = (size_t)atoll(argv[a]);
            if (scale == 0.0f) {
                std::vector<std::complex<float>> out(n);
                if (!ch.Apply(out, in, wrap)) return 3;
                fwrite(out.data(), 8, n, fo);
            } else {
                std::vector<uint8_t> out(2 * n);
                if (!ch.ApplyU8(out, in, wrap, scale)) return 3;
                fwrite(out.data(), 2, n, fo);
            }
        }
        fclose(fo);
    } catch (const std::exception& ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
