// dd_profile_class_harness.cpp -- DAB_DD_Profile into DAB_Diversity_Combiner's band-weight overload for
// tests/test_gpu_dd_profile_class.py: one receiver, n frames in sequence.
//   dd_profile_class_harness <dir> <n_frames> <alpha>
// Reads <dir>/dq.bin ([n][75][1536] complex float), scale.bin ([n] float), exclude.bin ([48] words).  The object excludes those carriers,
// smooths with alpha and is updated frame after frame; every frame's weights are the band weights of Combine over the one branch.
// Writes weights.bin ([n][128] float), profile.bin ([n][128]: the state behind each frame), mean.bin ([n]), combined.bin ([n][230400]
// int8), combined_scale.bin ([n]), again.bin ([128]: frame 0's weights once more after Reset) and plain.bin ([128]: frame 0's weights
// once more with the exclusion taken away again).  One line on stdout: frames=N
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ofdm/dab_dd_profile.h"
#include "ofdm/dab_diversity_combiner.h"

template <class T>
static std::vector<T> load(const std::string& path, size_t count) {
    std::vector<T> v(count);
    std::ifstream in(path, std::ios::binary);
    in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
    if (!in || (size_t)in.gcount() != count * sizeof(T)) { std::fprintf(stderr, "cannot read %zu items of %s\n", count, path.c_str()); std::exit(2); }
    return v;
}
template <class T>
static void put(std::ofstream& f, const T* p, size_t count) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)(count * sizeof(T))); }

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s dir n_frames alpha\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const size_t n = (size_t)std::atol(argv[2]);
    const float alpha = std::strtof(argv[3], nullptr);
    const size_t frame = DAB_DD_Profile::NB_PRODUCTS;
    const auto dq = load<std::complex<float>>(dir + "/dq.bin", n * frame);
    const auto scale = load<float>(dir + "/scale.bin", n);
    const auto exclude = load<uint32_t>(dir + "/exclude.bin", 48);
    DAB_DD_Profile prof;
    float w[128], again[128];
    // what is refused changes nothing
    if (prof.SetAlpha(0.0f) || prof.SetAlpha(1.5f) || prof.SetAlpha(std::strtof("nan", nullptr)) ||
        prof.SetExclude(tcb::span<const uint32_t>(exclude.data(), 47)) || prof.Update(tcb::span<const std::complex<float>>(dq.data(), frame - 1), w) ||
        prof.Update(tcb::span<const std::complex<float>>(dq.data(), frame), tcb::span<float>(w, 127)) || prof.IsValid()) {
        std::fprintf(stderr, "a wrong alpha, table or span was accepted\n"); return 1;
    }
    if (!prof.SetAlpha(alpha) || !prof.SetExclude(exclude)) { std::fprintf(stderr, "alpha or table refused\n"); return 1; }
    DAB_Diversity_Combiner comb(1);
    std::vector<viterbi_bit_t> bits(DABGPU_NB_FRAME_BITS);
    std::ofstream f_w(dir + "/weights.bin", std::ios::binary), f_p(dir + "/profile.bin", std::ios::binary), f_m(dir + "/mean.bin", std::ios::binary),
        f_c(dir + "/combined.bin", std::ios::binary), f_k(dir + "/combined_scale.bin", std::ios::binary), f_a(dir + "/again.bin", std::ios::binary),
        f_n(dir + "/plain.bin", std::ios::binary);
    for (size_t i = 0; i < n; i++) {
        if (!prof.Update(tcb::span<const std::complex<float>>(dq.data() + i * frame, frame), w) || !prof.IsValid()) {
            std::fprintf(stderr, "Update refused frame %zu\n", i); return 1;
        }
        put(f_w, w, 128); put(f_p, prof.GetProfile().data(), 128);
        const float m = prof.GetMeanNoise();
        put(f_m, &m, 1);
        const tcb::span<const std::complex<float>> p[1] = {{dq.data() + i * frame, frame}};
        const tcb::span<const float> bw[1] = {{w, 128}};
        const float k[1] = {scale[i]};
        if (!comb.Combine(p, k, tcb::span<const float>(), bw, bits)) { std::fprintf(stderr, "Combine refused frame %zu\n", i); return 1; }
        put(f_c, bits.data(), bits.size());
        const float ck = comb.GetScale();
        put(f_k, &ck, 1);
    }
    prof.Reset();
    if (prof.IsValid() || !prof.Update(tcb::span<const std::complex<float>>(dq.data(), frame), again)) { std::fprintf(stderr, "Reset\n"); return 1; }
    put(f_a, again, 128);
    prof.Reset();
    if (!prof.SetExclude(tcb::span<const uint32_t>()) || !prof.Update(tcb::span<const std::complex<float>>(dq.data(), frame), again)) {
        std::fprintf(stderr, "SetExclude()\n"); return 1;
    }
    put(f_n, again, 128);
    std::printf("frames=%zu\n", n);
    return 0;
}
