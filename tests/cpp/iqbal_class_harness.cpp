// iqbal_class_harness.cpp -- DAB_Stream_IQ_Balancer and DAB_IQ_Balancer (dab-radio_amd/host/ofdm/dab_iq_balancer.h) driven from files,
// block by block, for tests/test_gpu_iqbal_class.py (built by build()):
//   iqbal_class_harness <params.bin> <in.c64> <out.bin> <state.bin> <chunk_samples> <prime 0|1> <n> [<n> ...]
// params.bin = one dabgpu_iqbal_stream; block k gives the next n samples of the input to Process(); Flush() follows the last block; the
// outputs are written back to back, the final record to state.bin, and "iq chunks=N rejection_db=X" goes to stdout.  First, sizes that
// DAB_IQ_Balancer::Apply refuses, a MEASURE off a tile edge, a chunk that is no multiple of 1024 and Process() behind Flush() are tried.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <complex>
#include <stdexcept>
#include <vector>

#include "ofdm/dab_iq_balancer.h"

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
        if (pb.size() != sizeof(dabgpu_iqbal_stream) || ib.size() % 8) { fprintf(stderr, "bad input sizes\n"); return 2; }
        const dabgpu_iqbal_stream& P = *reinterpret_cast<const dabgpu_iqbal_stream*>(pb.data());
        const std::complex<float>* in = reinterpret_cast<const std::complex<float>*>(ib.data());
        const size_t chunk = (size_t)atoll(argv[5]);
        const bool prime = atoi(argv[6]) != 0;
        {   // an empty input and an output of another size are refused, not run; a MEASURE off a tile edge throws and leaves the state alone
            DAB_IQ_Balancer one(P, 2048);
            std::vector<std::complex<float>> a(2048, {1.0f, -1.0f}), b(40);
            if (one.Apply(a, {}, DABGPU_IQBAL_APPLY) || one.Apply(b, a, DABGPU_IQBAL_APPLY)) return 3;
            one.Seek(5);
            bool threw = false;
            try { one.Apply({}, a, DABGPU_IQBAL_MEASURE); } catch (const std::runtime_error&) { threw = true; }
            const dabgpu_iqbal_record R = one.State();
            if (!threw || R.N != 0.0f || R.calls_refused != 1 || R.valid != 0) return 5;
            threw = false;
            try { one.Apply({}, {a.data(), 1000}, DABGPU_IQBAL_MEASURE); } catch (const std::runtime_error&) { threw = true; }
            if (!threw) return 5;
            threw = false;
            try { DAB_Stream_IQ_Balancer bad(P, 1000); } catch (const std::runtime_error&) { threw = true; }
            if (!threw) return 5;
            DAB_Stream_IQ_Balancer ended(P, 1024);
            std::vector<std::complex<float>> o;
            ended.Process({a.data(), 40}, o);
            ended.Flush(o);
            threw = false;
            try { ended.Process({a.data(), 40}, o); } catch (const std::runtime_error&) { threw = true; }
            if (!threw || o.size() != 40) return 5;
        }
        DAB_Stream_IQ_Balancer balancer(P, chunk, prime);
        std::vector<std::complex<float>> out;
        size_t at = 0;
        for (int a = 7; a < argc; a++) {
            const size_t n = (size_t)atoll(argv[a]);
            if (at + n > ib.size() / 8) { fprintf(stderr, "input too short\n"); return 2; }
            balancer.Process({in + at, n}, out);
            if (out.size() > at + n) return 4;                  // (never ahead of its input)
            at += n;
        }
        balancer.Flush(out);
        const dabgpu_iqbal_record R = balancer.State();
        FILE* fo = fopen(argv[3], "wb");
        if (!fo) return 2;
        fwrite(out.data(), 8, out.size(), fo);
        fclose(fo);
        fo = fopen(argv[4], "wb");
        if (!fo) return 2;
        fwrite(&R, sizeof(R), 1, fo);
        fclose(fo);
        printf("iq chunks=%llu rejection_db=%.2f\n", (unsigned long long)balancer.Chunks(), DAB_IQ_Balancer::FrontEndRejectionDb(R));
    } catch (const std::exception& ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
