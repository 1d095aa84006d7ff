// dabgpu_simulate_transmitter.cpp -- the reference's examples/simulate_transmitter.cpp over the MI355X transmitter: one OFDM frame of
// DVB-scrambler bytes (:26-40, :150-159), modulated once on the device straight to 8-bit IQ (OFDM_Modulator::ProcessBlock, the optional
// frequency shift and QuantisedIQ<uint8_t> of :161-178 in one dabgpu_ofdm_modulate_frames_host_sync call), then written again and again
// like the reference's `while (true)` (:102) until a write fails.
//
//   -m, --transmission-mode MODE   1..4 (default 1)
//   -f, --frequency HZ             shift of the 8-bit IQ signal (default 0; f_norm = HZ / 2.048e6)
//   -o, --output FILE              default stdout
//   --frames N                     (not in the reference) stop after N frames
#include <stdio.h>
#include <stdlib.h>
#include <complex>
#include <stdexcept>
#include <string>
#include <vector>

#include "dab/dabgpu_shared_context.h"
#include "dabgpu.h"
#include "ofdm/dab_ofdm_params_ref.h"
#include "ofdm/dab_prs_ref.h"

// scrambler that is used for DVB transmissions (simulate_transmitter.cpp:26-40)
class Scrambler
{
private:
    uint16_t reg = 0;
public:
    uint16_t syncword = 0b0000000010101001;
    void Reset() { reg = syncword; }
    uint8_t Process() {
        uint8_t v = static_cast<uint8_t>(((reg ^ (reg << 1)) >> 8) & 0xFF);
        reg = (reg << 8) | v;
        return v;
    }
};

struct Args {
    int transmission_mode = 1;
    float frequency = 0.0f;
    std::string output_filename;
    long long frames = -1;             // < 0: until a write fails
};

static void usage(const char* argv0) {
    fprintf(stderr, "usage: %s [-m|--transmission-mode 1..4] [-f|--frequency HZ] [-o|--output FILE] [--frames N]\n"
                    "Simulates an OFDM transmitter sending random data (8-bit IQ at 2.048 MHz; default output stdout)\n", argv0);
}

static bool parse_args(int argc, char** argv, Args& args) {
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&]() -> std::string {
            if (i + 1 >= argc) throw std::runtime_error("missing value for " + a);
            return argv[++i];
        };
        if (a == "-m" || a == "--transmission-mode") args.transmission_mode = std::stoi(value());
        else if (a == "-f" || a == "--frequency") args.frequency = std::stof(value());
        else if (a == "-o" || a == "--output") args.output_filename = value();
        else if (a == "--frames") args.frames = std::stoll(value());
        else if (a == "-h" || a == "--help") return false;
        else throw std::runtime_error("unknown argument: " + a);
    }
    if (args.transmission_mode < 1 || args.transmission_mode > 4) throw std::runtime_error("--transmission-mode must be one of 1,2,3,4");
    return true;
}

int main(int argc, char** argv) {
    Args args;
    try {
        if (!parse_args(argc, argv, args)) { usage(argv[0]); return 1; }
    } catch (const std::exception& ex) {
        fprintf(stderr, "%s\n", ex.what());
        usage(argv[0]);
        return 1;
    }

    FILE* fp_out = stdout;
    if (!args.output_filename.empty()) {
        fp_out = fopen(args.output_filename.c_str(), "wb+");
        if (fp_out == nullptr) {
            fprintf(stderr, "Failed to open output file: '%s'\n", args.output_filename.c_str());
            return 1;
        }
    }

    try {
        const auto params = get_DAB_OFDM_params(args.transmission_mode);
        auto prs_fft_ref = std::vector<std::complex<float>>(params.nb_fft);
        get_DAB_PRS_reference(args.transmission_mode, prs_fft_ref);
        const size_t frame_size = params.nb_null_period + params.nb_symbol_period * params.nb_frame_symbols;
        const size_t nb_frame_bytes = (params.nb_frame_symbols - 1) * params.nb_data_carriers * 2 / 8;

        // generate random digital data (:150-159)
        auto frame_bytes_buf = std::vector<uint8_t>(nb_frame_bytes);
        auto scrambler = Scrambler();
        scrambler.Reset();
        for (size_t i = 0; i < nb_frame_bytes; i++) frame_bytes_buf[i] = scrambler.Process();

        // modulation, frequency shift (:167-171, only for a non-zero frequency) and quantisation on the device
        const float frequency_norm = (args.frequency != 0.0f) ? args.frequency / 2.048e6f : 0.0f;
        auto quantised = std::vector<uint8_t>(2 * frame_size);
        const int st = dabgpu_ofdm_modulate_frames_host_sync(dabgpu_shared_context(), args.transmission_mode, frame_bytes_buf.data(),
                                                             DABGPU_TX_PAYLOAD_REFERENCE, 1, reinterpret_cast<const float*>(prs_fft_ref.data()),
                                                             frequency_norm, quantised.data(), DABGPU_IQ_RAW_U8);
        if (st != DABGPU_OK) {
            fprintf(stderr, "Failed to create the OFDM frame: %s -- %s\n", dabgpu_strerror(st), dabgpu_last_error());
            return 1;
        }
        for (long long k = 0; args.frames < 0 || k < args.frames; k++) {
            const size_t nb_write = fwrite(quantised.data(), 2, frame_size, fp_out);
            if (nb_write != frame_size) {
                fprintf(stderr, "Failed to write out frame %zu/%zu\n", nb_write, frame_size);
                break;
            }
        }
    } catch (const std::exception& ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    if (fp_out != stdout) fclose(fp_out);
    else fflush(fp_out);
    return 0;
}
