// sym_profile_class_harness.cpp -- DAB_Symbol_Profile into DAB_Diversity_Combiner's symbol-weight overload for
// tests/test_gpu_sym_profile_class.py: one receiver, n frames in sequence.
//   sym_profile_class_harness <dir> <n_frames>
// Reads <dir>/dq.bin ([n][75][1536] complex float), scale.bin ([n] float), band.bin ([n][128] float: band weights from elsewhere).  Every
// frame's symbol weights go into Combine over the one branch, once alone and once on top of the frame's band weights.
// Writes weights.bin ([n][75] float), noise.bin ([n][75]), ref.bin ([n]), valid.bin ([n] int32), combined.bin and combined_banded.bin
// ([n][230400] int8 each), combined_scale.bin ([n]), and zero.bin ([75]: the weights of an all-zero frame).  One line on stdout: frames=N
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ofdm/dab_diversity_combiner.h"
#include "ofdm/dab_symbol_profile.h"

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
    if (argc != 3) { std::fprintf(stderr, "usage: %s dir n_frames\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const size_t n = (size_t)std::atol(argv[2]);
    const size_t frame = DAB_Symbol_Profile::NB_PRODUCTS;
    const auto dq = load<std::complex<float>>(dir + "/dq.bin", n * frame);
    const auto scale = load<float>(dir + "/scale.bin", n);
    const auto band = load<float>(dir + "/band.bin", n * 128);
    DAB_Symbol_Profile prof;
    DAB_Diversity_Combiner comb(1);
    std::vector<viterbi_bit_t> bits(DABGPU_NB_FRAME_BITS);
    float v[75];
    // what is refused changes nothing
    if (prof.Update(tcb::span<const std::complex<float>>(dq.data(), frame - 1), v) ||
        prof.Update(tcb::span<const std::complex<float>>(dq.data(), frame), tcb::span<float>(v, 74)) || prof.IsValid()) {
        std::fprintf(stderr, "a wrong span was accepted\n"); return 1;
    }
    {
        const tcb::span<const std::complex<float>> p[1] = {{dq.data(), frame}};
        const tcb::span<const float> short_sym[1] = {{v, 74}}, short_band[1] = {{band.data(), 127}}, sym[1] = {{v, 75}};
        const float k[1] = {scale[0]};
        if (comb.Combine(p, k, tcb::span<const float>(), tcb::span<const tcb::span<const float>>(), short_sym, bits) ||
            comb.Combine(p, k, tcb::span<const float>(), short_band, sym, bits) ||
            comb.Combine(p, k, tcb::span<const float>(), tcb::span<const tcb::span<const float>>(), tcb::span<const tcb::span<const float>>(), bits)) {
            std::fprintf(stderr, "a wrong table was accepted\n"); return 1;
        }
    }
    std::ofstream f_w(dir + "/weights.bin", std::ios::binary), f_q(dir + "/noise.bin", std::ios::binary), f_r(dir + "/ref.bin", std::ios::binary),
        f_v(dir + "/valid.bin", std::ios::binary), f_c(dir + "/combined.bin", std::ios::binary), f_b(dir + "/combined_banded.bin", std::ios::binary),
        f_k(dir + "/combined_scale.bin", std::ios::binary), f_z(dir + "/zero.bin", std::ios::binary);
    for (size_t i = 0; i < n; i++) {
        if (!prof.Update(tcb::span<const std::complex<float>>(dq.data() + i * frame, frame), v)) { std::fprintf(stderr, "Update refused frame %zu\n", i); return 1; }
        put(f_w, v, 75); put(f_q, prof.GetSymbolNoise().data(), 75);
        const float r = prof.GetRefNoise();
        const int32_t ok = prof.IsValid() ? 1 : 0;
        put(f_r, &r, 1); put(f_v, &ok, 1);
        const tcb::span<const std::complex<float>> p[1] = {{dq.data() + i * frame, frame}};
        const tcb::span<const float> bw[1] = {{band.data() + i * 128, 128}}, sym[1] = {{v, 75}};
        const float k[1] = {scale[i]};
        if (!comb.Combine(p, k, tcb::span<const float>(), tcb::span<const tcb::span<const float>>(), sym, bits)) { std::fprintf(stderr, "Combine refused frame %zu\n", i); return 1; }
        put(f_c, bits.data(), bits.size());
        const float ck = comb.GetScale();
        put(f_k, &ck, 1);
        if (!comb.Combine(p, k, tcb::span<const float>(), bw, sym, bits)) { std::fprintf(stderr, "Combine (banded) refused frame %zu\n", i); return 1; }
        put(f_b, bits.data(), bits.size());
    }
    const std::vector<std::complex<float>> zero(frame);
    if (!prof.Update(zero, v) || prof.IsValid() || prof.GetRefNoise() != 0.0f) { std::fprintf(stderr, "an all-zero frame was not skipped\n"); return 1; }
    put(f_z, v, 75);
    std::printf("frames=%zu\n", n);
    return 0;
}
