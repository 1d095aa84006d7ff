// channel_ber_harness.cpp -- DAB_Channel_BER (dab-radio_amd/host/dab/quality/dab_channel_ber.h) driven from a file, for
// tests/test_gpu_ber_class.py (built by build()):
//   channel_ber_harness <in.bin> <out.bin>
// in.bin = records of { int32 kind (0 FIB group, 1 sub-channel), dabgpu_subchannel, uint32 n_bits, uint32 n_bytes, soft bits, bytes };
// out.bin = one dabgpu_ber_result per record, then { uint64 total bits, uint64 total errors, double rate }.  A record with wrong sizes
// must be refused (false) and leaves an all-ones result.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dab/quality/dab_channel_ber.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: channel_ber_harness <in.bin> <out.bin>\n"); return 2; }
    std::vector<char> in;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) in.insert(in.end(), buf, buf + n);
    fclose(fp);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    try {
        DAB_Channel_BER ber;
        size_t at = 0;
        while (at < in.size()) {
            int32_t kind; dabgpu_subchannel sc; uint32_t n_bits, n_bytes;
            if (at + 4 + sizeof(sc) + 8 > in.size()) return 2;
            memcpy(&kind, &in[at], 4); at += 4;
            memcpy(&sc, &in[at], sizeof(sc)); at += sizeof(sc);
            memcpy(&n_bits, &in[at], 4); at += 4;
            memcpy(&n_bytes, &in[at], 4); at += 4;
            if (at + n_bits + n_bytes > in.size()) return 2;
            const tcb::span<const viterbi_bit_t> bits(reinterpret_cast<const viterbi_bit_t*>(&in[at]), n_bits);
            const tcb::span<const uint8_t> bytes(reinterpret_cast<const uint8_t*>(&in[at + n_bits]), n_bytes);
            at += (size_t)n_bits + n_bytes;
            dabgpu_ber_result r;
            memset(&r, 0xFF, sizeof(r));
            const bool ok = kind == 0 ? ber.MeasureFIBGroup(bits, bytes, r) : ber.MeasureSubchannel(sc, bits, bytes, r);
            if (!ok) memset(&r, 0xFF, sizeof(r));
            fwrite(&r, sizeof(r), 1, fo);
        }
        const uint64_t tot[2] = {ber.GetTotalBits(), ber.GetTotalErrors()};
        const double rate = ber.GetBitErrorRate();
        fwrite(tot, 8, 2, fo);
        fwrite(&rate, 8, 1, fo);
        ber.Reset();
        if (ber.GetTotalBits() != 0 || ber.GetBitErrorRate() != 0.0) return 3;
    } catch (const std::exception& ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    fclose(fo);
    return 0;
}
