// dabgpu_radio_cli.cpp -- command-line front end of the MI355X hot path with the option names of the reference's
// `basic_radio_app_cli` (examples/basic_radio_app.cpp:48-140) for the stages this library owns:
//
//   --configuration ofdm      IQ capture file  -> OFDM_Demod -> frame soft bits (or packed hard bytes) file
//   --configuration dab       frame bit file   -> FIC_Decoder / MSC_Decoder -> FIB bytes / sub-channel bytes files
//   --configuration dab+ofdm  both, bits handed over in memory
//
// The reference's application layer above the channel decoder (FIG parsing, database, audio, scraper, GUI) is not
// part of this library; where basic_radio_app hands the frame bits to BasicRadio, this tool writes what
// BasicRadio's first stage produces (basic_radio.cpp:41-65): the CRC-checked FIBs and, for sub-channels given
// explicitly with --radio-subchannel, the decoded logical frames.
//
// --tii (not in the reference; include/dabgpu.h "TII"): a TII_Decoder is fed inside the frame observer from the head of
// GetCorrelationTimeBuffer() -- the NULL period that follows the delivered frame, cut with that frame's timing, so the fine time offset it
// is given is 0 -- and GetNetFrequencyOffset(); GetFineTimeOffset() and GetTotalFramesDesync() go into the printed line and the reset rule.
// It skips the first frame after every acquisition (DABGPU_TII_SETTLE_FRAMES), accumulates, and every --tii-frames accumulated frames
// (default 8) prints one line on stdout:
//   tii frames=N fine_time=T net_freq=F: P:C/STRENGTH ...          (?:C/0xMASK/STRENGTH for a comb whose mask is no pattern)
// The reader must not overwrite the buffer's head while the observer reads it, so with --tii every Process() call is followed by
// Synchronize() and --ofdm-block-size may not exceed one frame less a NULL period.
//
// --snr (not in the reference; include/dabgpu.h "Noise estimate"): a DAB_Noise_Estimator is fed from the same buffer as --tii, under the same
// restrictions.  The frame observer keeps a copy of the buffer's head, the NULL period that follows the delivered frame; the phase reference
// symbol that belongs to it is the one BEHIND it, which the reader has not seen yet.  So the estimate is made on the reading thread, after the
// Synchronize() that follows the NEXT Process() call: by then the 2552 samples behind that NULL are in the buffer (a block holds at least
// that many), and they stay there until the next frame ends (two blocks are shorter than a frame), which the unchanged head confirms.  The
// window is cut with the delivered frame's timing, so the fine time offset given is 0; the rotation is GetNetFrequencyOffset().  One line
// per frame on stdout:
//   snr frame=N noise=NOISE signal=SIGNAL snr_db=DB
// N = frames read when the NULL was kept, NOISE = noise_power (per sample), SIGNAL = signal_power / 2048 - noise_power (the symbol's mean
// power per sample less the noise in it), DB = 10 log10(SIGNAL / NOISE).  The NULL behind the first frame after an acquisition is skipped,
// as for --tii; so is a frame without a finite estimate.  --ofdm-block-size from 2552 to 98304.
//
// --ber (not in the reference; include/dabgpu.h "Channel BER"): the channel decode stage prints one line per frame to stdout,
//   ber frame=N fic=ERRORS/BITS sub0=ERRORS/BITS ...
// the channel bit errors of the frame's four FIB groups and of each sub-channel's CIFs that were decoded (0/0 while the time
// de-interleaver fills).  The decoder classes stay as they are: the stage decodes each FIB group once more for its 96 bytes with the received
// CRCs, keeps the last 16 CIFs of every sub-channel on the host, de-interleaves by index and hands both to DAB_Channel_BER.
//
// --soft-bits normalised|csi [--soft-level L] (not in the reference; include/dabgpu.h "Soft-decision policy"): csi hands the decoders
// channel-state weighted soft bits (OFDM_Demod::SetSoftDecision), level L in [1, 127], default 64; normalised, the default, is the
// reference's.  Transmission mode I and the OFDM stage only.
//
// --soft-bits banded [--alpha A] [--soft-level L] (include/dabgpu.h "Noise profile", "Banded receive diversity"): the demodulator runs under
// the csi policy; inside the frame observer the head of GetCorrelationTimeBuffer() -- the NULL behind the delivered frame, as --tii reads it:
// fine time offset 0, rotation GetNetFrequencyOffset() -- goes to DAB_Noise_Profile::Update (smoothing A in (0, 1], default 0.25), and the 128
// band weights with GetFrameDataVec() and GetSoftScale() to DAB_Diversity_Combiner::Combine with one branch; the combined soft bits take the
// place of the demodulator's for the decoders and the output file.  A frame whose profile is not valid keeps the demodulator's own csi
// bits.  The restrictions are --tii's: Synchronize() after every Process(), --ofdm-block-size up to 193952, not with --input-rate or
// --channel-offset-hz.
//
// --soft-bits banded-dd [--alpha A] [--soft-level L] (include/dabgpu.h "Decision-directed noise profile"): the banded path with DAB_DD_Profile in
// the profile's place: the band weights come from the delivered frame's own products (GetFrameDataVec()), not from the NULL behind it, so an
// interferer that is silent during the NULL symbol (gated, TDMA) is still weighted down.  Options and restrictions are banded's.
//
// --symbol-weights (include/dabgpu.h "Symbol noise profile", "Symbol-weighted receive diversity"; with --soft-bits csi, banded or banded-dd):
// the delivered frame's own products (GetFrameDataVec()) go to DAB_Symbol_Profile::Update, and its 75 symbol weights to
// DAB_Diversity_Combiner::Combine on top of what the policy gives: under csi the frame goes through the one-branch combiner with no band
// table, under banded and banded-dd the weights join the band weights (a frame whose band profile is not valid still takes the symbol
// weights alone).  A frame whose symbol profile is not valid is treated as without the flag.  This answers wideband bursts of a symbol or
// longer; FIC symbols under a burst stay lost.  Refused with --soft-bits normalised: that policy divides every product by its own
// amplitude, which is what the weights act on.
//
// --track-clock [GAIN] [--clock-report] (include/dabgpu.h "Sampling-clock tracker"; with --soft-bits csi, banded or banded-dd): the delivered
// frame's own products (GetFrameDataVec()) are copied and go through DAB_Clock_Tracker::Track (loop gain GAIN in (0, 1], default 1; taken
// only where the next argument is a number), which estimates the ramp a sampling-clock error leaves over the carriers, carries the slope
// from frame to frame (across resynchronisations too) and de-rotates the copy.  Everything else that reads products reads the copy: the
// decision-directed and symbol profiles and the one-branch combiner, through which the frame then always goes -- under plain csi with
// no table at all, as --symbol-weights does.  --clock-report prints one "clock frame=N ppm=X valid=V" line per frame, ppm in the sign of
// dabgpu_simulate_transmitter --clock-ppm.  Refused with --soft-bits normalised: that path has no products to de-rotate, its soft bits
// are made inside the demodulator.
//
// --blank [THRESHOLD] (not in the reference; include/dabgpu.h "Impulse blanker"): every block of samples at 2.048 MHz -- behind --input-rate
// and --channel-offset-hz -- goes through a DAB_Stream_Blanker with dabgpu_blanker_defaults() (threshold 3 unless given) in front of
// OFDM_Demod, which so runs 800 samples behind the input; the rest is flushed at the end of the input.  One "blank blocks=N of M" line
// follows the ofdm line.  Transmission mode I and the OFDM stage only.  The blanker emits whole blocks of 32 samples, so a call to the
// demodulator may be up to 31 samples longer than the block just read: with --tii or --soft-bits banded --ofdm-block-size may not exceed
// 193920, with --snr 98272.  THRESHOLD is taken only where the next argument is a number ("--blank -i FILE" and "--blank abc" leave it at 3;
// "abc" is then an unknown argument).  Absent: no blanker is made and the tool does what it did.
//
// --iq-balance [TIME_CONSTANT_FRAMES] (not in the reference; include/dabgpu.h "IQ balance"): the readers' complex samples go first -- ahead of
// --input-rate, --channel-offset-hz and --blank -- through a DAB_Stream_IQ_Balancer, which removes the DC term and the mirror image of a
// zero-IF front end blindly: a frame's worth of samples at the capture's rate (rounded up to whole tiles of 1024) is measured, then mapped
// with the coefficients that include it, so the first frame is corrected already; the rest is flushed at the end of the input.  The
// estimator's memory is TIME_CONSTANT_FRAMES frames (16 unless given; taken only where the next argument is a number, as --blank's).  The
// OFDM stage only.  --iq-report prints one "iq frame=N dc=RE,IM w=RE,IM irr_db=X" line per measured frame on stdout: the DC term, the image
// coefficient w = K2 / conj(K1) and the front end's own rejection -20 log10 |w|, computed on the host.  Absent: no balancer is made and
// the tool does what it did.
//
// --input-rate HZ (not in the reference; include/dabgpu.h "Resampler"): the capture's sample rate, e.g. 2400000, 2560000, 3072000 or 4096000.
// Every block is resampled to 2.048 MHz on the device between the format conversion and OFDM_Demod (DAB_Stream_Resampler: the outputs do
// not depend on the block size).  Absent or 2048000: no resampler is made and the tool does what it did.
//
// --channel-offset-hz F, together with --input-rate HZ (include/dabgpu.h "Channeliser"): the capture is a wideband one, HZ from 2048000 to
// 32768000, and the block to receive lies F Hz from its centre.  Every block is split by D = dabgpu_channeliser_decim_for(HZ) at offset F
// (DAB_Stream_Channeliser) between the format conversion and the resampler, which then takes HZ / D to 2.048 MHz and is absent where HZ / D
// is 2.048 MHz already (8192000: D = 4, no resampler; 10000000: D = 4, then 2.5 -> 2.048 MS/s).  The filter's edges are the block's own
// (768 kHz) and its neighbour's (944 kHz) at the rate the split leaves.  With F = 0 and HZ below 4096000 no channeliser is made: the
// resampler alone, as without the option.
//
// Output files are byte-for-byte what the reference writes with the same options (frame bits: 230400 int8 per frame,
// or 28800 bytes per frame with --ofdm-output-hard-bytes, LSB first).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <complex>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "app_helpers/app_iq_readers.h"
#include "app_helpers/app_viterbi_convert_block.h"
#include "dab/constants/dab_parameters.h"
#include "dab/fic/fic_decoder.h"
#include "dab/msc/msc_decoder.h"
#include "dab/dabgpu_shared_context.h"
#include "dab/quality/dab_channel_ber.h"
#include "dab/tx/dab_channeliser.h"
#include "dab/tx/dab_resampler.h"
#include "ofdm/dab_blanker.h"
#include "ofdm/dab_iq_balancer.h"
#include "ofdm/ofdm_helpers.h"
#include "ofdm/tii_decoder.h"
#include "ofdm/dab_noise_estimator.h"
#include "ofdm/dab_dd_profile.h"
#include "ofdm/dab_clock_tracker.h"
#include "ofdm/dab_symbol_profile.h"
#include "ofdm/dab_noise_profile.h"
#include "ofdm/dab_diversity_combiner.h"

struct Args {
    std::string input_file;
    int transmission_mode = 1;
    bool is_ofdm_used = true;
    bool is_dab_used = true;
    std::string ofdm_input_mode = "raw_u8";
    size_t ofdm_block_size = 65536;
    bool ofdm_disable_coarse_freq = false;
    bool ofdm_enable_output = false;
    std::string ofdm_output;
    bool ofdm_output_hard_bytes = false;
    bool radio_input_hard_bytes = false;
    std::string radio_fib_output;
    std::string radio_msc_output = "subchannel_";
    std::vector<Subchannel> subchannels;
    bool tii = false;
    int tii_frames = 8;
    bool snr = false;
    double input_rate = 2.048e6;
    bool channelise = false;
    double channel_offset_hz = 0.0;
    bool ber = false;
    int soft_policy = DABGPU_SOFT_NORMALISED;
    float soft_level = 64.0f;
    bool soft_level_given = false;
    bool soft_banded = false;
    bool symbol_weights = false;                     // --symbol-weights: DAB_Symbol_Profile's weights into the one-branch combiner
    bool track_clock = false, clock_report = false;  // --track-clock: DAB_Clock_Tracker in front of everything that reads the products
    float clock_gain = 1.0f;
    bool soft_banded_dd = false;                     // (with soft_banded: the decision-directed profile in the NULL-based one's place)
    float alpha = 0.25f;
    bool alpha_given = false;
    bool blank = false;
    float blank_threshold = 3.0f;
    bool iq_balance = false, iq_report = false;
    double iq_frames = 16.0;
};

static void usage(const char* argv0) {
    fprintf(stderr,
        "usage: %s [-i FILE] [--transmission-mode 1] [--configuration dab+ofdm|ofdm|dab]\n"
        "  [--ofdm-input-mode MODE] [--ofdm-block-size SAMPLES] [--ofdm-disable-coarse-freq]\n"
        "  [--ofdm-enable-output] [--ofdm-output FILE] [--ofdm-output-hard-bytes]\n"
        "  [--radio-input-hard-bytes] [--radio-fib-output FILE]\n"
        "  [--radio-subchannel START,LENGTH,EEP_LEVEL(1-4),EEP_TYPE(A|B) | START,LENGTH,uep,UEP_INDEX]...\n"
        "  [--radio-msc-output PREFIX] [--tii] [--tii-frames N] [--snr] [--input-rate HZ] [--channel-offset-hz F] [--ber]\n"
        "  [--soft-bits normalised|csi|banded|banded-dd] [--soft-level 1..127] [--alpha A] [--symbol-weights] [--blank [THRESHOLD]]\n"
        "  [--track-clock [GAIN]] [--clock-report]\n"
        "  [--iq-balance [TIME_CONSTANT_FRAMES]] [--iq-report]\n"
        "MODE: ", argv0);
    for (const auto& m : iq_read_modes) fprintf(stderr, "%s ", m.c_str());
    fprintf(stderr, "\n");
}

static Subchannel parse_subchannel(const std::string& text, size_t id) {
    std::vector<std::string> f;
    size_t a = 0;
    for (;;) {
        const size_t b = text.find(',', a);
        f.push_back(text.substr(a, b == std::string::npos ? b : b - a));
        if (b == std::string::npos) break;
        a = b + 1;
    }
    if (f.size() != 4) throw std::runtime_error("--radio-subchannel expects 4 comma separated fields: '" + text + "'");
    Subchannel sc((subchannel_id_t)id);
    sc.start_address = (subchannel_addr_t)std::stoi(f[0]);
    sc.length = (subchannel_size_t)std::stoi(f[1]);
    if (f[2] == "uep") {
        sc.is_uep = true;
        sc.uep_prot_index = (uep_protection_index_t)std::stoi(f[3]);
    } else {
        const int level = std::stoi(f[2]);
        if (level < 1 || level > 4) throw std::runtime_error("EEP level must be 1..4: '" + text + "'");
        sc.eep_prot_level = (eep_protection_level_t)(level - 1);
        if (f[3] == "A" || f[3] == "a") sc.eep_type = EEP_Type::TYPE_A;
        else if (f[3] == "B" || f[3] == "b") sc.eep_type = EEP_Type::TYPE_B;
        else throw std::runtime_error("EEP type must be A or B: '" + text + "'");
    }
    sc.is_complete = true;
    return sc;
}

static bool parse_args(int argc, char** argv, Args& args) {
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&](void) -> std::string {
            if (i + 1 >= argc) throw std::runtime_error("missing value after " + a);
            return argv[++i];
        };
        if (a == "-i" || a == "--input") args.input_file = value();
        else if (a == "--transmission-mode") args.transmission_mode = std::stoi(value());
        else if (a == "--configuration") {
            const std::string c = value();
            if (c == "dab+ofdm") { args.is_ofdm_used = true; args.is_dab_used = true; }
            else if (c == "ofdm") { args.is_ofdm_used = true; args.is_dab_used = false; }
            else if (c == "dab") { args.is_ofdm_used = false; args.is_dab_used = true; }
            else throw std::runtime_error("unknown configuration '" + c + "'");
        }
        else if (a == "--ofdm-input-mode") args.ofdm_input_mode = value();
        else if (a == "--ofdm-block-size") args.ofdm_block_size = (size_t)std::stoull(value());
        else if (a == "--ofdm-total-threads" || a == "--radio-total-threads") (void)value();     // accepted, no effect
        else if (a == "--ofdm-disable-coarse-freq") args.ofdm_disable_coarse_freq = true;
        else if (a == "--ofdm-enable-output") args.ofdm_enable_output = true;
        else if (a == "--ofdm-output") args.ofdm_output = value();
        else if (a == "--ofdm-output-hard-bytes") args.ofdm_output_hard_bytes = true;
        else if (a == "--radio-input-hard-bytes") args.radio_input_hard_bytes = true;
        else if (a == "--radio-fib-output") args.radio_fib_output = value();
        else if (a == "--radio-msc-output") args.radio_msc_output = value();
        else if (a == "--radio-subchannel") { const auto v = value(); args.subchannels.push_back(parse_subchannel(v, args.subchannels.size())); }
        else if (a == "--tii") args.tii = true;
        else if (a == "--snr") args.snr = true;
        else if (a == "--tii-frames") { args.tii_frames = std::stoi(value()); args.tii = true; }
        else if (a == "--ber") args.ber = true;
        else if (a == "--soft-bits") {
            const std::string p = value();
            if (p == "normalised") args.soft_policy = DABGPU_SOFT_NORMALISED;
            else if (p == "csi") args.soft_policy = DABGPU_SOFT_CSI;
            else if (p == "banded") { args.soft_policy = DABGPU_SOFT_CSI; args.soft_banded = true; }
            else if (p == "banded-dd") { args.soft_policy = DABGPU_SOFT_CSI; args.soft_banded = true; args.soft_banded_dd = true; }
            else throw std::runtime_error("unknown soft-bit policy '" + p + "' (normalised, csi, banded or banded-dd)");
        }
        else if (a == "--symbol-weights") args.symbol_weights = true;
        else if (a == "--clock-report") args.clock_report = true;
        else if (a == "--track-clock") {
            args.track_clock = true;
            char* end = nullptr;                                                  // the value is optional, as --blank's
            if (i + 1 < argc) {
                const float t = std::strtof(argv[i + 1], &end);
                if (end != argv[i + 1] && *end == '\0') { args.clock_gain = t; i++; }
            }
        }
        else if (a == "--alpha") { args.alpha = std::stof(value()); args.alpha_given = true; }
        else if (a == "--soft-level") { args.soft_level = std::stof(value()); args.soft_level_given = true; }
        else if (a == "--iq-report") args.iq_report = true;
        else if (a == "--iq-balance") {
            args.iq_balance = true;
            char* end = nullptr;                                                  // the value is optional, as --blank's
            if (i + 1 < argc) {
                const double t = std::strtod(argv[i + 1], &end);
                if (end != argv[i + 1] && *end == '\0') { args.iq_frames = t; i++; }
            }
        }
        else if (a == "--blank") {
            args.blank = true;
            char* end = nullptr;                                                  // the value is optional: taken only where the next argument is a number
            if (i + 1 < argc) {
                const float t = std::strtof(argv[i + 1], &end);
                if (end != argv[i + 1] && *end == '\0') { args.blank_threshold = t; i++; }
            }
        }
        else if (a == "--input-rate") args.input_rate = std::stod(value());
        else if (a == "--channel-offset-hz") { args.channel_offset_hz = std::stod(value()); args.channelise = true; }
        else if (a == "-h" || a == "--help") return false;
        else throw std::runtime_error("unknown argument '" + a + "'");
    }
    if (args.ber && !args.is_dab_used) throw std::runtime_error("--ber needs the channel decode stage");
    if ((args.iq_balance || args.iq_report) && !args.is_ofdm_used) throw std::runtime_error("--iq-balance needs the OFDM stage");
    if (args.iq_report && !args.iq_balance) throw std::runtime_error("--iq-report needs --iq-balance");
    if (args.iq_balance && !(args.iq_frames >= 0.25 && args.iq_frames <= 1e6)) throw std::runtime_error("--iq-balance: a time constant of 0.25 .. 1e6 frames");
    if (args.blank && !args.is_ofdm_used) throw std::runtime_error("--blank needs the OFDM stage");
    if (args.blank && args.transmission_mode != 1) throw std::runtime_error("--blank is available in transmission mode 1 only");
    if (args.blank && !(args.blank_threshold > 1.0f && args.blank_threshold <= 1024.0f)) throw std::runtime_error("--blank: a threshold above 1, up to 1024");
    if (args.soft_policy != DABGPU_SOFT_NORMALISED && !args.is_ofdm_used) throw std::runtime_error("--soft-bits needs the OFDM stage");
    if (args.soft_level_given && args.soft_policy != DABGPU_SOFT_CSI) throw std::runtime_error("--soft-level needs --soft-bits csi");
    if (!(args.soft_level >= 1.0f && args.soft_level <= 127.0f)) throw std::runtime_error("--soft-level: a level from 1 to 127");
    if (args.symbol_weights && args.soft_policy != DABGPU_SOFT_CSI)
        throw std::runtime_error("--symbol-weights needs --soft-bits csi, banded or banded-dd: the normalised policy divides every product by its own amplitude, "
                                 "which is what the weights act on");
    if (args.track_clock && args.soft_policy != DABGPU_SOFT_CSI)
        throw std::runtime_error("--track-clock needs --soft-bits csi, banded or banded-dd: under the normalised policy the soft bits are made inside the "
                                 "demodulator and there are no products to de-rotate");
    if (args.track_clock && !(args.clock_gain > 0.0f && args.clock_gain <= 1.0f)) throw std::runtime_error("--track-clock: a gain above 0, up to 1");
    if (args.clock_report && !args.track_clock) throw std::runtime_error("--clock-report needs --track-clock");
    if (args.alpha_given && !args.soft_banded) throw std::runtime_error("--alpha needs --soft-bits banded");
    if (!(args.alpha > 0.0f && args.alpha <= 1.0f)) throw std::runtime_error("--alpha: above 0, up to 1");
    if (args.soft_banded && args.ofdm_block_size > 196608 - 2656) throw std::runtime_error("--soft-bits banded: --ofdm-block-size may not exceed 193952");
    if (args.soft_banded && args.channelise) throw std::runtime_error("--channel-offset-hz is not available with --soft-bits banded");
    if (args.soft_banded && args.input_rate != 2.048e6) throw std::runtime_error("--input-rate is not available with --soft-bits banded (resampled blocks may exceed --ofdm-block-size)");
    if (args.snr && !args.is_ofdm_used) throw std::runtime_error("--snr needs the OFDM stage");
    if (args.snr && (args.ofdm_block_size < 2552 || args.ofdm_block_size > 98304)) throw std::runtime_error("--snr: --ofdm-block-size from 2552 to 98304");
    if (args.tii && !args.is_ofdm_used) throw std::runtime_error("--tii needs the OFDM stage");
    if (args.tii && args.tii_frames < 1) throw std::runtime_error("--tii-frames must be positive");
    if (args.tii && args.ofdm_block_size > 196608 - 2656) throw std::runtime_error("--tii: --ofdm-block-size may not exceed 193952");
    // the blanker hands OFDM_Demod whole blocks of 32 samples: up to 31 samples more than the block just read
    if (args.blank && (args.soft_banded || args.tii) && args.ofdm_block_size > 196608 - 2656 - 32)
        throw std::runtime_error("--blank with --tii or --soft-bits banded: --ofdm-block-size may not exceed 193920");
    if (args.blank && args.snr && args.ofdm_block_size > 98304 - 32) throw std::runtime_error("--blank with --snr: --ofdm-block-size may not exceed 98272");
    if (args.channelise) {
        if (!(args.input_rate >= 2.048e6 && args.input_rate <= 8 * 4.096e6)) throw std::runtime_error("--channel-offset-hz: --input-rate 2048000 .. 32768000 samples per second");
        if (!(std::fabs(args.channel_offset_hz) <= 0.5 * args.input_rate)) throw std::runtime_error("--channel-offset-hz: within half of --input-rate either way");
        if (!args.is_ofdm_used) throw std::runtime_error("--channel-offset-hz needs the OFDM stage");
        if (args.tii) throw std::runtime_error("--channel-offset-hz is not available with --tii");
        if (args.snr) throw std::runtime_error("--channel-offset-hz is not available with --snr");
        if (args.channel_offset_hz == 0.0 && args.input_rate < 4.096e6) args.channelise = false;       // the resampler alone
    }
    if (!args.channelise && !(args.input_rate >= 1.024e6 && args.input_rate <= 4.096e6))
        throw std::runtime_error("--input-rate: 1024000 .. 4096000 samples per second");
    if (args.input_rate != 2.048e6 && !args.is_ofdm_used) throw std::runtime_error("--input-rate needs the OFDM stage");
    if (args.input_rate != 2.048e6 && args.tii) throw std::runtime_error("--input-rate is not available with --tii (resampled blocks may exceed --ofdm-block-size)");
    if (args.input_rate != 2.048e6 && args.snr) throw std::runtime_error("--input-rate is not available with --snr (resampled blocks may exceed --ofdm-block-size)");
    if (args.transmission_mode != 1) throw std::runtime_error("only transmission mode I is implemented");
    if (args.ofdm_block_size == 0) throw std::runtime_error("--ofdm-block-size must be positive");
    return true;
}

// BasicRadio's first stage (basic_radio.cpp:41-65, basic_fic_runner.cpp:34-49, basic_dab_plus_channel.cpp:47-51)
class ChannelDecodeStage {
private:
    const DAB_Parameters m_params;
    FIC_Decoder m_fic;
    std::vector<std::unique_ptr<MSC_Decoder>> m_msc;
    FILE* m_fib_out = nullptr;
    std::vector<FILE*> m_msc_out;
    // --ber: the meter, each sub-channel as the C ABI describes it and its last 16 CIFs (slot = CIF count mod 16)
    std::unique_ptr<DAB_Channel_BER> m_ber;
    std::vector<dabgpu_subchannel> m_ber_sc;
    std::vector<std::vector<viterbi_bit_t>> m_ber_ring;
    std::vector<viterbi_bit_t> m_ber_bits;
    size_t m_ber_cifs = 0;
    // what CIF_Deinterleaver delivers for the CIF filed last: bit i from the CIF that is 15 - bitrev4(i mod 16) CIFs older
    void BerDeinterleave(size_t k, size_t newest) {
        static const int delay[16] = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15};
        const size_t n = (size_t)m_ber_sc[k].length * 64;
        m_ber_bits.resize(n);
        for (size_t i = 0; i < n; i++) m_ber_bits[i] = m_ber_ring[k][((newest + 16 - (size_t)(15 - delay[i & 15])) & 15) * n + i];
    }
public:
    size_t total_frames = 0, total_fibs = 0, total_fib_groups_failed = 0;
    std::vector<size_t> total_msc_bytes;
    ChannelDecodeStage(const Args& args)
    : m_params(get_dab_parameters(args.transmission_mode)),
      m_fic((size_t)m_params.nb_fib_cif_bits, (size_t)m_params.nb_fibs_per_cif) {
        if (!args.radio_fib_output.empty()) {
            m_fib_out = fopen(args.radio_fib_output.c_str(), "wb");
            if (!m_fib_out) throw std::runtime_error("cannot open " + args.radio_fib_output);
        }
        m_fic.OnFIB().Attach([this](tcb::span<const uint8_t> fib) {
            total_fibs++;
            if (m_fib_out) fwrite(fib.data(), 1, fib.size(), m_fib_out);
        });
        for (size_t k = 0; k < args.subchannels.size(); k++) {
            m_msc.push_back(std::make_unique<MSC_Decoder>(args.subchannels[k]));
            const std::string path = args.radio_msc_output + std::to_string(k) + ".bin";
            FILE* f = fopen(path.c_str(), "wb");
            if (!f) throw std::runtime_error("cannot open " + path);
            m_msc_out.push_back(f);
            total_msc_bytes.push_back(0);
        }
        if (args.ber) {
            m_ber = std::make_unique<DAB_Channel_BER>();
            for (const Subchannel& s : args.subchannels) {
                m_ber_sc.push_back({(int)s.start_address, (int)s.length, s.is_uep ? 1 : 0, (int)s.uep_prot_index, (int)s.eep_prot_level,
                                    s.eep_type == EEP_Type::TYPE_B ? 1 : 0});
                m_ber_ring.emplace_back((size_t)16 * (size_t)s.length * 64);
            }
        }
    }
    ~ChannelDecodeStage() {
        if (m_fib_out) fclose(m_fib_out);
        for (FILE* f : m_msc_out) fclose(f);
    }
    size_t frame_bits() const { return (size_t)m_params.nb_frame_bits; }
    void Process(tcb::span<const viterbi_bit_t> bits) {
        if (bits.size() != (size_t)m_params.nb_frame_bits) return;                      // basic_radio.cpp:42-47
        total_frames++;
        auto fic_bits = bits.subspan(0, (size_t)m_params.nb_fic_bits);
        auto msc_bits = bits.subspan((size_t)m_params.nb_fic_bits, (size_t)m_params.nb_msc_bits);
        for (int c = 0; c < m_params.nb_cifs; c++) {
            const size_t before = total_fibs;
            m_fic.DecodeFIBGroup(fic_bits.subspan((size_t)c * m_params.nb_fib_cif_bits, (size_t)m_params.nb_fib_cif_bits), (size_t)c);
            if (total_fibs - before != (size_t)m_params.nb_fibs_per_cif) total_fib_groups_failed++;
        }
        uint64_t fic_err = 0, fic_n = 0;
        std::vector<uint64_t> sub_err(m_msc.size(), 0), sub_n(m_msc.size(), 0);
        if (m_ber && m_params.nb_fib_cif_bits == DABGPU_NB_FIB_GROUP_BITS) {
            for (int c = 0; c < m_params.nb_cifs; c++) {
                const auto group = fic_bits.subspan((size_t)c * DABGPU_NB_FIB_GROUP_BITS, DABGPU_NB_FIB_GROUP_BITS);
                uint8_t bytes[96]; uint32_t mask = 0; uint64_t path = 0;
                const int st = dabgpu_fic_decode_group_host_sync(dabgpu_shared_context(), group.data(), bytes, &mask, &path, dabgpu_tie_rule_from_env());
                if (st != DABGPU_OK) throw std::runtime_error(std::string("--ber: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
                dabgpu_ber_result r;
                if (m_ber->MeasureFIBGroup(group, tcb::span<const uint8_t>(bytes, 96), r)) { fic_err += r.n_errors; fic_n += r.n_bits; }
            }
        }
        for (int c = 0; c < m_params.nb_cifs; c++) {
            auto cif = msc_bits.subspan((size_t)c * m_params.nb_cif_bits, (size_t)m_params.nb_cif_bits);
            for (size_t k = 0; k < m_msc.size(); k++) {
                auto bytes = m_msc[k]->DecodeCIF(cif);
                if (m_ber) {
                    const size_t n = (size_t)m_ber_sc[k].length * 64, slot = m_ber_cifs & 15;
                    memcpy(&m_ber_ring[k][slot * n], cif.data() + (size_t)m_ber_sc[k].start_address * 64, n);
                    if (!bytes.empty() && m_ber_cifs >= 15) {
                        BerDeinterleave(k, slot);
                        dabgpu_ber_result r;
                        if (m_ber->MeasureSubchannel(m_ber_sc[k], m_ber_bits, tcb::span<const uint8_t>(bytes.data(), bytes.size()), r)) {
                            sub_err[k] += r.n_errors; sub_n[k] += r.n_bits;
                        }
                    }
                }
                if (bytes.empty()) continue;                                            // time de-interleaver still filling
                fwrite(bytes.data(), 1, bytes.size(), m_msc_out[k]);
                total_msc_bytes[k] += bytes.size();
            }
            m_ber_cifs++;
        }
        if (m_ber) {
            printf("ber frame=%zu fic=%llu/%llu", total_frames - 1, (unsigned long long)fic_err, (unsigned long long)fic_n);
            for (size_t k = 0; k < m_msc.size(); k++) printf(" sub%zu=%llu/%llu", k, (unsigned long long)sub_err[k], (unsigned long long)sub_n[k]);
            printf("\n");
        }
    }
};

static int run(const Args& args) {
    FILE* fp_in = stdin;
    if (!args.input_file.empty()) {
        fp_in = fopen(args.input_file.c_str(), "rb");
        if (!fp_in) { fprintf(stderr, "Failed to open input file: '%s'\n", args.input_file.c_str()); return 1; }
    }
    FILE* fp_ofdm_out = nullptr;
    if (args.is_ofdm_used && args.ofdm_enable_output) {
        fp_ofdm_out = stdout;
        if (!args.ofdm_output.empty()) {
            fp_ofdm_out = fopen(args.ofdm_output.c_str(), "wb");
            if (!fp_ofdm_out) { fprintf(stderr, "Failed to open output file: '%s'\n", args.ofdm_output.c_str()); return 1; }
        }
    }
    std::unique_ptr<ChannelDecodeStage> radio;
    if (args.is_dab_used) radio = std::make_unique<ChannelDecodeStage>(args);

    if (args.is_ofdm_used) {
        std::shared_ptr<DeviceIQFileReader> reader;
        try {
            reader = get_iq_file_reader_from_mode_string(fp_in, args.ofdm_input_mode);
        } catch (const std::exception& ex) {
            fprintf(stderr, "Failed to parse OFDM IQ file with format: %s\n%s\n", args.ofdm_input_mode.c_str(), ex.what());
            return 1;
        }
        auto demod = Create_OFDM_Demodulator(args.transmission_mode);
        demod->GetConfig().sync.is_coarse_freq_correction = !args.ofdm_disable_coarse_freq;
        if (args.soft_policy != DABGPU_SOFT_NORMALISED) demod->SetSoftDecision(args.soft_policy, args.soft_level);
        std::vector<uint8_t> hard;
        // --soft-bits banded: the profile of the NULL symbols, the one-branch combiner and the frame's combined soft bits
        std::unique_ptr<DAB_Noise_Profile> profile;
        std::unique_ptr<DAB_DD_Profile> dd_profile;                                  // --soft-bits banded-dd: in its place
        std::unique_ptr<DAB_Diversity_Combiner> combiner;
        std::vector<viterbi_bit_t> banded_bits;
        int banded_desync = 0;
        size_t banded_frames = 0, banded_kept = 0;
        if (args.soft_banded) {
            if (args.soft_banded_dd) { dd_profile = std::make_unique<DAB_DD_Profile>(); dd_profile->SetAlpha(args.alpha); }
            else { profile = std::make_unique<DAB_Noise_Profile>(); profile->SetAlpha(args.alpha); }
        }
        // --symbol-weights: the profile of the frame's product rows; its weights join the band weights, or go alone
        std::unique_ptr<DAB_Symbol_Profile> sym_profile;
        size_t sym_frames = 0, sym_kept = 0;
        if (args.symbol_weights) sym_profile = std::make_unique<DAB_Symbol_Profile>();
        // --track-clock: the frame's products are copied, de-rotated, and read from the copy by everything below
        std::unique_ptr<DAB_Clock_Tracker> clock;
        std::vector<std::complex<float>> clock_products;
        size_t clock_frames = 0, clock_kept = 0;
        if (args.track_clock) { clock = std::make_unique<DAB_Clock_Tracker>(args.clock_gain); clock_products.resize(DAB_Clock_Tracker::NB_PRODUCTS); }
        if (args.soft_banded || args.symbol_weights || args.track_clock) {
            combiner = std::make_unique<DAB_Diversity_Combiner>(1);
            banded_bits.resize(DABGPU_NB_FRAME_BITS);
            demod->EnableDebugBuffers(true);                                         // the products of every frame, from the first
        }
        std::unique_ptr<TII_Decoder> tii;
        if (args.tii) tii = std::make_unique<TII_Decoder>(args.transmission_mode);
        int tii_desync = 0;
        // --snr: the NULL kept by the observer, the frame it follows, frames since the acquisition, Process() calls since it was kept
        std::unique_ptr<DAB_Noise_Estimator> snr;
        if (args.snr) snr = std::make_unique<DAB_Noise_Estimator>();
        std::vector<std::complex<float>> snr_null;
        int snr_frame = 0, snr_desync = 0, snr_since_acquisition = 0, snr_calls = 0;
        auto snr_poll = [&]() {                                                      // on the reading thread, behind Synchronize()
            if (snr_null.empty() || snr_calls++ == 0) return;                        // (the call that delivered the frame may end inside its window)
            const auto corr = demod->GetCorrelationTimeBuffer();
            dabgpu_noise_record rec;
            if (demod->GetTotalFramesDesync() == snr_desync && std::equal(snr_null.begin(), snr_null.end(), corr.begin()) &&
                snr->Estimate(corr, demod->GetNetFrequencyOffset(), 0, rec) && rec.valid) {
                const double noise = rec.noise_power, signal = (double)rec.signal_power / 2048.0 - noise;
                printf("snr frame=%d noise=%.6g signal=%.6g snr_db=%.2f\n", snr_frame, noise, signal, 10.0 * std::log10(signal / noise));
            }
            snr_null.clear();
        };
        demod->On_OFDM_Frame().Attach([&](tcb::span<const viterbi_bit_t> demod_bits) {
            tcb::span<const viterbi_bit_t> bits = demod_bits;
            if (profile || dd_profile || sym_profile || clock) {
                if ((profile || dd_profile) && demod->GetTotalFramesDesync() != banded_desync) {
                    banded_desync = demod->GetTotalFramesDesync();
                    if (profile) profile->Reset(); else dd_profile->Reset();
                }
                float w[DABGPU_NOISE_PROFILE_BANDS], v[DABGPU_SYM_PROFILE_SYMBOLS];
                // (the buffer has the reference's size, 75 x 2048; the products are its first 75 x 1536)
                tcb::span<const std::complex<float>> products[1] = {demod->GetFrameDataVec().first((size_t)75 * 1536)};
                if (clock) {
                    std::copy(products[0].begin(), products[0].end(), clock_products.begin());
                    const bool tracked = clock->Track(clock_products);
                    if (tracked) clock_frames++; else clock_kept++;
                    if (args.clock_report) printf("clock frame=%d ppm=%.3f valid=%d\n", demod->GetTotalFramesRead(), clock->GetPpm(), tracked ? 1 : 0);
                    products[0] = clock_products;
                }
                const bool banded = (profile || dd_profile) &&
                                    (profile ? (profile->Update(demod->GetCorrelationTimeBuffer().first(2656), 0, demod->GetNetFrequencyOffset(), w) && profile->IsValid())
                                             : (dd_profile->Update(products[0], w) && dd_profile->IsValid()));
                const bool weighted = sym_profile && sym_profile->Update(products[0], v) && sym_profile->IsValid();
                const tcb::span<const float> band_weights[1] = {{w, (size_t)DABGPU_NOISE_PROFILE_BANDS}};
                const tcb::span<const float> symbol_weights[1] = {{v, (size_t)DABGPU_SYM_PROFILE_SYMBOLS}};
                const float scale[1] = {demod->GetSoftScale()};
                bool combined = false;
                if (weighted)
                    combined = combiner->Combine(products, scale, tcb::span<const float>(),
                                                 banded ? tcb::span<const tcb::span<const float>>(band_weights) : tcb::span<const tcb::span<const float>>(),
                                                 symbol_weights, banded_bits);
                else if (banded)
                    combined = combiner->Combine(products, scale, tcb::span<const float>(), band_weights, banded_bits);
                else if (clock)
                    combined = combiner->Combine(products, scale, tcb::span<const float>(), banded_bits);
                if (combined) bits = banded_bits;
                if (profile || dd_profile) { if (combined && banded) banded_frames++; else banded_kept++; }
                if (sym_profile) { if (combined && weighted) sym_frames++; else sym_kept++; }
            }
            if (snr) {
                if (demod->GetTotalFramesDesync() != snr_desync) { snr_desync = demod->GetTotalFramesDesync(); snr_since_acquisition = 0; }
                snr_null.clear();
                if (snr_since_acquisition++ > 0) {
                    const auto null_region = demod->GetCorrelationTimeBuffer().first(2656);
                    snr_null.assign(null_region.begin(), null_region.end());
                    snr_frame = demod->GetTotalFramesRead(); snr_calls = 0;
                }
            }
            if (tii) {
                if (demod->GetTotalFramesDesync() != tii_desync) { tii_desync = demod->GetTotalFramesDesync(); tii->Reset(); }
                const auto null_region = demod->GetCorrelationTimeBuffer().first(2656);
                const float net = demod->GetNetFrequencyOffset();
                const bool decide = (tii->GetTotalFrames() + 1) % args.tii_frames == 0;
                if (tii->Process(null_region, net, 0, decide) && decide) {
                    printf("tii frames=%d fine_time=%d net_freq=%.6g:", tii->GetTotalFrames(), demod->GetFineTimeOffset(), (double)net);
                    for (const auto& r : tii->GetRecords()) {
                        if (r.main_id >= 0) printf(" %d:%d/%.1f", r.main_id, r.sub_id, (double)r.strength);
                        else printf(" ?:%d/0x%02X/%.1f", r.sub_id, r.mask, (double)r.strength);
                    }
                    printf("\n");
                }
            }
            if (fp_ofdm_out) {
                if (args.ofdm_output_hard_bytes) {
                    hard.resize(bits.size() / 8);
                    convert_viterbi_bits_to_bytes(bits.first(hard.size() * 8), hard);
                    fwrite(hard.data(), 1, hard.size(), fp_ofdm_out);
                } else {
                    fwrite(bits.data(), 1, bits.size(), fp_ofdm_out);
                }
            }
            if (radio) radio->Process(bits);
        });
        std::vector<std::complex<float>> block(args.ofdm_block_size);               // OFDM_Block::run, app_ofdm_blocks.h:45-57
        std::unique_ptr<DAB_Stream_Resampler> resampler;
        std::vector<std::complex<float>> resampled;
        std::unique_ptr<DAB_Stream_Channeliser> channeliser;
        std::vector<std::vector<std::complex<float>>> split;
        double block_rate = args.input_rate;
        if (args.channelise) {
            const int decim = DAB_Channeliser::DecimFor(args.input_rate);
            block_rate = args.input_rate / (double)decim;
            // the block's edge (768 kHz) and its neighbour's (944 kHz) in cycles per sample of the rate the split leaves: 0.375 / 0.4609375 at 2.048 MS/s
            channeliser = std::make_unique<DAB_Stream_Channeliser>(decim, std::vector<dabgpu_channeliser_channel>{DAB_Channeliser::Channel(args.channel_offset_hz, args.input_rate)},
                                                                   768000.0 / block_rate, 944000.0 / block_rate);
            fprintf(stderr, "channeliser: decimation %d, %.0f samples per second per block, design error %.3g\n", decim, block_rate, channeliser->DesignError());
            if (channeliser->DesignError() > 1e-4)
                fprintf(stderr, "warning: that is above the 1e-4 the design holds at 2048000 samples per second per block (the transition between the "
                                "block's edge and its neighbour's is narrower at this rate)\n");
        }
        if (block_rate != 2.048e6) resampler = std::make_unique<DAB_Stream_Resampler>(DAB_Resampler::StepWord(block_rate, 2.048e6));
        // --blank: the impulse blanker between the 2.048 MHz samples and the demodulator, `reach` samples behind its input
        std::unique_ptr<DAB_Stream_Blanker> blanker;
        std::vector<std::complex<float>> blanked;
        if (args.blank) blanker = std::make_unique<DAB_Stream_Blanker>(DAB_Blanker::Defaults(args.blank_threshold));
        auto feed = [&](tcb::span<const std::complex<float>> x) {
            if (!blanker) { demod->Process(x); return; }
            blanked.clear();
            blanker->Process(x, blanked);
            if (!blanked.empty()) demod->Process(blanked);
        };
        // --iq-balance: first on the readers' samples, a frame's worth of the capture's rate at a time
        std::unique_ptr<DAB_Stream_IQ_Balancer> balancer;
        std::vector<std::complex<float>> balanced;
        uint64_t iq_reported = 0;
        if (args.iq_balance) {
            const size_t frame = ((size_t)std::ceil(196608.0 * args.input_rate / 2.048e6) + DABGPU_IQBAL_TILE - 1) & ~(size_t)(DABGPU_IQBAL_TILE - 1);
            balancer = std::make_unique<DAB_Stream_IQ_Balancer>(DAB_IQ_Balancer::Defaults(args.iq_frames * (double)frame), frame, true);
        }
        auto iq_report = [&]() {
            if (!args.iq_report || balancer->Chunks() == iq_reported) return;
            iq_reported = balancer->Chunks();
            const dabgpu_iqbal_record R = balancer->State();
            printf("iq frame=%llu dc=%.6g,%.6g w=%.6g,%.6g irr_db=%.2f\n", (unsigned long long)iq_reported, (double)R.d_re, (double)R.d_im, (double)R.w_re,
                   (double)R.w_im, DAB_IQ_Balancer::FrontEndRejectionDb(R));
        };
        auto ingest = [&](tcb::span<const std::complex<float>> x) {
            if (channeliser) {
                split.clear();
                channeliser->Process(x, split);
                if (!split.empty() && !split[0].empty()) {
                    if (resampler) {
                        resampled.clear();
                        resampler->Process(split[0], resampled);
                        if (!resampled.empty()) feed(resampled);
                    } else feed(split[0]);
                }
            } else if (resampler) {
                resampled.clear();
                resampler->Process(x, resampled);
                if (!resampled.empty()) feed(resampled);
            } else
            feed(x);
        };
        // what the balancer emits (a frame's worth at a time) goes on in pieces of the block size, so that the observers below see the calls
        // they see without it
        auto ingest_balanced = [&]() {
            for (size_t at = 0; at < balanced.size(); at += block.size()) {
                ingest(tcb::span<const std::complex<float>>(balanced.data() + at, std::min(block.size(), balanced.size() - at)));
                if (tii || snr || profile) demod->Synchronize();
                if (snr) snr_poll();
            }
        };
        for (;;) {
            const size_t length = reader->read(block);
            if (length == 0) break;
            if (balancer) {
                balanced.clear();
                balancer->Process(tcb::span<const std::complex<float>>(block.data(), length), balanced);
                iq_report();
                ingest_balanced();
            } else
            ingest(tcb::span<const std::complex<float>>(block.data(), length));
            if (tii || snr || profile) demod->Synchronize();                                   // the observer reads the head of the correlation buffer
            if (snr) snr_poll();
            if (length != block.size()) break;
        }
        if (balancer) {                                                                      // the end of the input: what the balancer still holds
            balanced.clear();
            balancer->Flush(balanced);
            ingest_balanced();
        }
        if (blanker) {                                                                       // the end of the input: what the blanker still holds
            blanked.clear();
            blanker->Flush(blanked);
            if (!blanked.empty()) demod->Process(blanked);
        }
        demod->Synchronize();
        fprintf(stderr, "ofdm: frames_read=%d frames_desync=%d coarse=%.6g fine=%.6g\n", demod->GetTotalFramesRead(),
                demod->GetTotalFramesDesync(), demod->GetCoarseFrequencyOffset(), demod->GetFineFrequencyOffset());
        if (profile || dd_profile) fprintf(stderr, "banded: frames_combined=%zu frames_kept_csi=%zu\n", banded_frames, banded_kept);
        if (sym_profile) fprintf(stderr, "symbols: frames_weighted=%zu frames_kept=%zu\n", sym_frames, sym_kept);
        if (clock) fprintf(stderr, "clock: frames_tracked=%zu frames_kept=%zu ppm=%.3f\n", clock_frames, clock_kept, clock->GetPpm());
        if (blanker) fprintf(stderr, "blank blocks=%llu of %llu\n", (unsigned long long)blanker->BlankedBlocks(), (unsigned long long)blanker->TotalBlocks());
    } else {
        std::vector<viterbi_bit_t> bits(radio->frame_bits());                         // Basic_Radio_Block::run, app_radio_blocks.h:31-38
        std::vector<uint8_t> packed(bits.size() / 8);
        for (;;) {
            if (args.radio_input_hard_bytes) {
                if (fread(packed.data(), 1, packed.size(), fp_in) != packed.size()) break;
                convert_viterbi_bytes_to_bits(packed, bits);
            } else {
                if (fread(bits.data(), 1, bits.size(), fp_in) != bits.size()) break;
            }
            radio->Process(bits);
        }
    }
    if (radio) {
        fprintf(stderr, "radio: frames=%zu fibs_crc_ok=%zu fib_groups_with_failures=%zu", radio->total_frames, radio->total_fibs,
                radio->total_fib_groups_failed);
        for (size_t k = 0; k < radio->total_msc_bytes.size(); k++) fprintf(stderr, " subchannel%zu_bytes=%zu", k, radio->total_msc_bytes[k]);
        fprintf(stderr, "\n");
    }
    if (fp_ofdm_out && fp_ofdm_out != stdout) fclose(fp_ofdm_out);
    if (fp_in != stdin) fclose(fp_in);
    return 0;
}

int main(int argc, char** argv) {
    Args args;
    try {
        if (!parse_args(argc, argv, args)) { usage(argv[0]); return 0; }
        return run(args);
    } catch (const std::exception& ex) {
        fprintf(stderr, "error: %s\n", ex.what());
        return 1;
    }
}
