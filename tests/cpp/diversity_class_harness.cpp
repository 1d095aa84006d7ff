// diversity_class_harness.cpp -- DAB_Diversity_Combiner behind two OFDM_Demod mirrors for tests/test_gpu_diversity_class.py: two complex-float
// captures of one transmission, each through a mode I OFDM_Demod of its own under SetSoftDecision(DABGPU_SOFT_CSI, level); per delivered
// frame the branch's GetFrameDataVec() and GetSoftScale() are kept, frame i of branch 0 is paired with frame i of branch 1, and the pairs go
// through DAB_Diversity_Combiner::Combine.
//   diversity_class_harness <iq0.c32> <iq1.c32> <out_dir> <block_size> <level> <w0> <w1>
// Writes <out_dir>/dq<b>.bin ([frames][75][1536] complex float), scale<b>.bin ([frames] float), own<b>.bin (the branch's own soft bits),
// combined.bin ([pairs][230400] int8), combined_scale.bin ([pairs] float), live.bin ([pairs] uint32).  The last pair is combined a second time
// with branch 1 absent (an empty span): combined_single.bin.  One line on stdout: frames0=N frames1=M pairs=P
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ofdm/dab_diversity_combiner.h"
#include "ofdm/ofdm_helpers.h"

int main(int argc, char** argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: %s iq0.c32 iq1.c32 out_dir block_size level w0 w1\n", argv[0]); return 2; }
    const std::string out = argv[3];
    const size_t block = (size_t)std::atol(argv[4]);
    const float level = (float)std::atof(argv[5]);
    const float w[2] = {(float)std::atof(argv[6]), (float)std::atof(argv[7])};
    const size_t frame = 75 * 1536;
    std::vector<std::vector<std::complex<float>>> dq[2];
    std::vector<float> scale[2];
    for (int b = 0; b < 2; b++) {
        std::ifstream in(argv[1 + b], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1 + b]); return 2; }
        auto demod = Create_OFDM_Demodulator(1);
        demod->SetSoftDecision(DABGPU_SOFT_CSI, level);
        demod->EnableDebugBuffers(true);
        std::ofstream f_own(out + "/own" + std::to_string(b) + ".bin", std::ios::binary);
        demod->On_OFDM_Frame().Attach([&](tcb::span<const viterbi_bit_t> bits) {
            const auto v = demod->GetFrameDataVec();
            dq[b].emplace_back(v.begin(), v.begin() + (std::ptrdiff_t)frame);
            scale[b].push_back(demod->GetSoftScale());
            f_own.write(reinterpret_cast<const char*>(bits.data()), (std::streamsize)bits.size());
        });
        std::vector<std::complex<float>> buf(block);
        for (;;) {
            in.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)(block * sizeof(std::complex<float>)));
            const size_t got = (size_t)in.gcount() / sizeof(std::complex<float>);
            if (got == 0) break;
            demod->Process(tcb::span<const std::complex<float>>(buf.data(), got));
        }
        demod->Synchronize();
        std::ofstream f_dq(out + "/dq" + std::to_string(b) + ".bin", std::ios::binary), f_k(out + "/scale" + std::to_string(b) + ".bin", std::ios::binary);
        for (auto& d : dq[b]) f_dq.write(reinterpret_cast<const char*>(d.data()), (std::streamsize)(frame * sizeof(std::complex<float>)));
        f_k.write(reinterpret_cast<const char*>(scale[b].data()), (std::streamsize)(scale[b].size() * sizeof(float)));
    }
    const size_t pairs = dq[0].size() < dq[1].size() ? dq[0].size() : dq[1].size();
    DAB_Diversity_Combiner comb(2);
    std::vector<viterbi_bit_t> bits(DABGPU_NB_FRAME_BITS);
    std::ofstream f_c(out + "/combined.bin", std::ios::binary), f_ck(out + "/combined_scale.bin", std::ios::binary), f_m(out + "/live.bin", std::ios::binary),
        f_s(out + "/combined_single.bin", std::ios::binary);
    for (size_t i = 0; i < pairs; i++) {
        const tcb::span<const std::complex<float>> p[2] = {dq[0][i], dq[1][i]};
        const float k[2] = {scale[0][i], scale[1][i]};
        if (!comb.Combine(p, k, w, bits)) { std::fprintf(stderr, "Combine refused pair %zu\n", i); return 1; }
        f_c.write(reinterpret_cast<const char*>(bits.data()), (std::streamsize)bits.size());
        const float ck = comb.GetScale(); const uint32_t m = comb.GetLiveMask();
        f_ck.write(reinterpret_cast<const char*>(&ck), sizeof(ck)); f_m.write(reinterpret_cast<const char*>(&m), sizeof(m));
        if (i + 1 == pairs) {
            const tcb::span<const std::complex<float>> q[2] = {dq[0][i], {}};
            if (!comb.Combine(q, k, tcb::span<const float>(), bits) || comb.GetLiveMask() != 1u) { std::fprintf(stderr, "single-branch pair refused\n"); return 1; }
            f_s.write(reinterpret_cast<const char*>(bits.data()), (std::streamsize)bits.size());
        }
    }
    // wrong sizes are refused without touching the device
    const tcb::span<const std::complex<float>> one[1] = {pairs ? tcb::span<const std::complex<float>>(dq[0][0]) : tcb::span<const std::complex<float>>()};
    const float k1[1] = {1.0f};
    if (comb.Combine(one, k1, tcb::span<const float>(), bits)) { std::fprintf(stderr, "one branch accepted by a combiner of two\n"); return 1; }
    std::printf("frames0=%zu frames1=%zu pairs=%zu\n", dq[0].size(), dq[1].size(), pairs);
    return 0;
}
