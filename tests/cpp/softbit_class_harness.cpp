// softbit_class_harness.cpp -- OFDM_Demod::SetSoftDecision for tests/test_gpu_softbits_class.py: a complex-float capture through one mode I
// OFDM_Demod in blocks; per delivered frame the 230400 soft bits go to <out_dir>/frame_bits.bin and (coarse, fine, fine time offset) to
// <out_dir>/states.bin.
//   softbit_class_harness <iq.c32> <out_dir> <block_size> <policy> <level> <others> <when>
// others: that many further OFDM_Demod objects are alive when the receiver is made (with the default rule the second mode I receiver of a
//         process joins the receiver bank)
// when:   before = SetSoftDecision before the first Process() call; after = after the last one (on a bank member: refused); never
// One line on stdout: frames=N member_at_creation=0|1 member_at_end=0|1 refused=0|1 [error=...]
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "ofdm/ofdm_helpers.h"

int main(int argc, char** argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: %s iq.c32 out_dir block_size policy level others before|after|never\n", argv[0]); return 2; }
    const std::string out = argv[2], when = argv[7];
    const size_t block = (size_t)std::atol(argv[3]);
    const int policy = std::atoi(argv[4]), others = std::atoi(argv[6]);
    const float level = (float)std::atof(argv[5]);
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<std::unique_ptr<OFDM_Demod>> idle;
    for (int k = 0; k < others; k++) idle.push_back(Create_OFDM_Demodulator(1));
    auto demod = Create_OFDM_Demodulator(1);
    const int member0 = demod->IsBankMember() ? 1 : 0;
    int refused = 0, n_frames = 0;
    std::string error;
    auto set = [&] {
        try { demod->SetSoftDecision(policy, level); }
        catch (const std::exception& ex) { refused = 1; error = ex.what(); }
    };
    if (when == "before") set();
    std::ofstream f_bits(out + "/frame_bits.bin", std::ios::binary), f_st(out + "/states.bin", std::ios::binary);
    demod->On_OFDM_Frame().Attach([&](tcb::span<const viterbi_bit_t> bits) {
        n_frames++;
        f_bits.write(reinterpret_cast<const char*>(bits.data()), (std::streamsize)bits.size());
        const float st[3] = {demod->GetCoarseFrequencyOffset(), demod->GetFineFrequencyOffset(), (float)demod->GetFineTimeOffset()};
        f_st.write(reinterpret_cast<const char*>(st), sizeof(st));
    });
    std::vector<std::complex<float>> buf(block);
    if (!refused)
        for (;;) {
            in.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)(block * sizeof(std::complex<float>)));
            const size_t got = (size_t)in.gcount() / sizeof(std::complex<float>);
            if (got == 0) break;
            demod->Process(tcb::span<const std::complex<float>>(buf.data(), got));
        }
    demod->Synchronize();
    if (when == "after") set();
    std::printf("frames=%d member_at_creation=%d member_at_end=%d refused=%d%s%s\n", n_frames, member0, demod->IsBankMember() ? 1 : 0, refused,
                refused ? " error=" : "", error.c_str());
    return 0;
}
