// noise_class_harness.cpp -- DAB_Noise_Estimator into DAB_Diversity_Combiner for tests/test_gpu_noise_class.py: two branches of n frames.
//   noise_class_harness <dir> <n_frames> <fine_time_offset>
// Reads <dir>/null<b>.c32 ([n][5208 + fine_time_offset] complex float: each frame from where its NULL was expected to the end of its
// phase reference symbol), freq<b>.bin ([n] float), dq<b>.bin ([n][75][1536] complex float), scale<b>.bin ([n] float) for b = 0, 1.
// Every frame of every branch goes through DAB_Noise_Estimator::Estimate; the records' weights are the weights of
// DAB_Diversity_Combiner::Combine.  Writes rec<b>.bin ([n] dabgpu_noise_record), combined.bin ([n][230400] int8), combined_scale.bin,
// live.bin.  One line on stdout: frames=N
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ofdm/dab_diversity_combiner.h"
#include "ofdm/dab_noise_estimator.h"

template <class T>
static std::vector<T> load(const std::string& path, size_t count) {
    std::vector<T> v(count);
    std::ifstream in(path, std::ios::binary);
    in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
    if (!in || (size_t)in.gcount() != count * sizeof(T)) { std::fprintf(stderr, "cannot read %zu items of %s\n", count, path.c_str()); std::exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s dir n_frames fine_time_offset\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const size_t n = (size_t)std::atol(argv[2]);
    const int fto = std::atoi(argv[3]);
    const size_t span = DAB_Noise_Estimator::NB_SAMPLES + (size_t)fto, frame = 75 * 1536;
    DAB_Noise_Estimator est;
    std::vector<dabgpu_noise_record> rec[2];
    std::vector<std::complex<float>> dq[2];
    std::vector<float> scale[2];
    for (int b = 0; b < 2; b++) {
        const std::string s = std::to_string(b);
        const auto iq = load<std::complex<float>>(dir + "/null" + s + ".c32", n * span);
        const auto freq = load<float>(dir + "/freq" + s + ".bin", n);
        dq[b] = load<std::complex<float>>(dir + "/dq" + s + ".bin", n * frame);
        scale[b] = load<float>(dir + "/scale" + s + ".bin", n);
        rec[b].resize(n);
        for (size_t i = 0; i < n; i++)
            if (!est.Estimate(tcb::span<const std::complex<float>>(iq.data() + i * span, span), freq[i], fto, rec[b][i])) {
                std::fprintf(stderr, "Estimate refused frame %zu of branch %d\n", i, b); return 1;
            }
        std::ofstream(dir + "/rec" + s + ".bin", std::ios::binary).write(reinterpret_cast<const char*>(rec[b].data()), (std::streamsize)(n * sizeof(dabgpu_noise_record)));
        // wrong sizes and offsets are refused without touching the device, the record left all zero
        dabgpu_noise_record r;
        if (est.Estimate(tcb::span<const std::complex<float>>(iq.data(), span - 1), 0.0f, fto, r) || r.weight != 0.0f || r.valid != 0u ||
            est.Estimate(tcb::span<const std::complex<float>>(iq.data(), span), 0.0f, -1, r) || est.Estimate(tcb::span<const std::complex<float>>(iq.data(), span), 0.0f, 1544, r)) {
            std::fprintf(stderr, "a short span or an offset outside the range was accepted\n"); return 1;
        }
    }
    DAB_Diversity_Combiner comb(2);
    std::vector<viterbi_bit_t> bits(DABGPU_NB_FRAME_BITS);
    std::ofstream f_c(dir + "/combined.bin", std::ios::binary), f_ck(dir + "/combined_scale.bin", std::ios::binary), f_m(dir + "/live.bin", std::ios::binary);
    for (size_t i = 0; i < n; i++) {
        const tcb::span<const std::complex<float>> p[2] = {{dq[0].data() + i * frame, frame}, {dq[1].data() + i * frame, frame}};
        const float k[2] = {scale[0][i], scale[1][i]}, w[2] = {rec[0][i].weight, rec[1][i].weight};
        if (!comb.Combine(p, k, w, bits)) { std::fprintf(stderr, "Combine refused frame %zu\n", i); return 1; }
        f_c.write(reinterpret_cast<const char*>(bits.data()), (std::streamsize)bits.size());
        const float ck = comb.GetScale(); const uint32_t m = comb.GetLiveMask();
        f_ck.write(reinterpret_cast<const char*>(&ck), sizeof(ck)); f_m.write(reinterpret_cast<const char*>(&m), sizeof(m));
    }
    std::printf("frames=%zu\n", n);
    return 0;
}
