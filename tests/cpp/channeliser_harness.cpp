// channeliser_harness.cpp -- DAB_Channeliser and DAB_Stream_Channeliser (dab-radio_amd/host/dab/tx/dab_channeliser.h) driven from files,
// for tests/test_gpu_channelise_class.py (built by build()):
//   channeliser_harness split   <decim> <channels.bin> <in.c64> <out.c64> <wrap 0|1> <start> <seek> <n_out> [<n_out> ...]
//   channeliser_harness combine <decim> <channels.bin> <in.c64> <out.bin> <wrap 0|1> <start> <seek> <u8_scale, 0 = complex float> <n_out> [...]
//   channeliser_harness stream  <decim> <channels.bin> <in.c64> <out.c64> <block> [<block> ...]      (the block sizes are cycled)
//   channeliser_harness cstream <decim> <channels.bin> <in.c64> <out.c64> <block> [<block> ...]      (DAB_Stream_Combiner; in.c64 = the rows back to back)
// channels.bin = dabgpu_channeliser_channel records (stream 0).  split / combine write each call's rows back to back; stream writes every
// channel's whole output, channel by channel.  Prints the design error and, per split, the input span InputNeeded reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <complex>
#include <vector>

#include "dab/tx/dab_channeliser.h"

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
    if (argc < 7) { fprintf(stderr, "usage: see the source\n"); return 2; }
    try {
        const int decim = atoi(argv[2]);
        const auto cb = slurp(argv[3]);
        const auto ib = slurp(argv[4]);
        if (cb.empty() || cb.size() % sizeof(dabgpu_channeliser_channel) || ib.size() % 8) { fprintf(stderr, "bad input sizes\n"); return 2; }
        std::vector<dabgpu_channeliser_channel> channels(cb.size() / sizeof(dabgpu_channeliser_channel));
        memcpy(channels.data(), cb.data(), cb.size());
        const tcb::span<const std::complex<float>> in(reinterpret_cast<const std::complex<float>*>(ib.data()), ib.size() / 8);
        FILE* fo = fopen(argv[5], "wb");
        if (!fo) return 2;
        if (!strcmp(argv[1], "stream")) {
            DAB_Stream_Channeliser sc(decim, channels);
            printf("design_error %.9e\n", sc.DesignError());
            std::vector<std::vector<std::complex<float>>> out;
            size_t at = 0;
            for (int a = 6; at < in.size(); a = (a + 1 < argc) ? a + 1 : 6) {
                const size_t n = std::min((size_t)atoll(argv[a]), in.size() - at);
                sc.Process(in.subspan(at, n), out);
                at += n;
            }
            for (const auto& row : out) fwrite(row.data(), 8, row.size(), fo);
            printf("outputs %zu\n", out.empty() ? (size_t)0 : out[0].size());
        } else if (!strcmp(argv[1], "cstream")) {
            DAB_Stream_Combiner sc(decim, channels);
            const size_t rows = channels.size(), len = in.size() / rows;
            std::vector<std::complex<float>> out, block;
            size_t at = 0;
            for (int a = 6; at < len; a = (a + 1 < argc) ? a + 1 : 6) {
                const size_t n = std::min((size_t)atoll(argv[a]), len - at);
                block.resize(rows * n);
                for (size_t c = 0; c < rows; c++) std::copy(in.begin() + (long)(c * len + at), in.begin() + (long)(c * len + at + n), block.begin() + (long)(c * n));
                sc.Process(block, out);
                at += n;
            }
            fwrite(out.data(), 8, out.size(), fo);
            printf("outputs %zu\n", out.size());
        } else {
            const bool split = !strcmp(argv[1], "split"), wrap = atoi(argv[6]) != 0;
            if (argc < (split ? 10 : 11)) { fprintf(stderr, "usage: see the source\n"); return 2; }
            DAB_Channeliser ch(decim, channels, atoll(argv[7]));
            printf("design_error %.9e\n", ch.DesignError());
            if (ch.Split({}, {}, wrap) || ch.Combine({}, {}, wrap)) return 3;   // an empty input is refused, not run
            ch.Seek(strtoull(argv[8], nullptr, 10));
            const float scale = split ? 0.0f : (float)atof(argv[9]);
            for (int a = split ? 9 : 10; a < argc; a++) {
                const size_t n = (size_t)atoll(argv[a]);
                if (split) {
                    int64_t first; uint64_t count;
                    ch.InputNeeded(n, first, count);
                    printf("span %lld %llu\n", (long long)first, (unsigned long long)count);
                    std::vector<std::complex<float>> out(n * channels.size());
                    if (!ch.Split(out, in, wrap)) return 3;
                    fwrite(out.data(), 8, out.size(), fo);
                } else if (scale == 0.0f) {
                    std::vector<std::complex<float>> out(n);
                    if (!ch.Combine(out, in, wrap)) return 3;
                    fwrite(out.data(), 8, n, fo);
                } else {
                    std::vector<uint8_t> out(2 * n);
                    if (!ch.CombineU8(out, in, wrap, scale)) return 3;
                    fwrite(out.data(), 2, n, fo);
                }
            }
            printf("position %llu\n", (unsigned long long)ch.Position());
        }
        fclose(fo);
    } catch (const std::exception& ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
