// dabgpu_simulate_transmitter.cpp -- the reference's examples/simulate_transmitter.cpp over the MI355X transmitter: one OFDM frame of
// DVB-scrambler bytes (:26-40, :150-159), modulated once on the device straight to 8-bit IQ (OFDM_Modulator::ProcessBlock, the optional
// frequency shift and QuantisedIQ<uint8_t> of :161-178 in one dabgpu_ofdm_modulate_frames_host_sync call), then written again and again
// like the reference's `while (true)` (:102) until a write fails.
//
//   -m, --transmission-mode MODE   1..4 (default 1)
//   -f, --frequency HZ             shift of the 8-bit IQ signal (default 0; f_norm = HZ / 2.048e6)
//   -o, --output FILE              default stdout
//   --frames N                     (not in the reference) stop after N frames
// Channel-coded frames (not in the reference, mode I; include/dabgpu.h "Channel encoder"): with any of the options below every frame is
// encoded from FIB bodies and sub-channel bytes (dabgpu_tx_bank_transmit_frames_host_sync) and a receiver decodes what was sent.
//   --subchannel START:LENGTH:PROT repeatable; capacity units; PROT = eepL-A | eepL-B (L = 1..4) or uepROW (row 0..63 of table 8)
//   --fib-file FILE                FIB bodies, 30 bytes each, 12 per frame, read cyclically (tools/dabfig.py writes them)
//   --payload-file FILE            the CIFs' input records (the sub-channels' bytes back to back in list order), read cyclically
//   --seed N                       random FIB bodies / payload where no file is given (default 1)
// Channel (not in the reference; include/dabgpu.h "Channel model", DAB_Channel_Model): with any of the options below the frames are
// modulated to complex float, passed through the channel on the device and quantised there; without them the output is byte for byte
// what it was.  The stream position runs on from frame to frame: the oscillator keeps its phase and the noise never repeats.
//   --snr-db DB                    white Gaussian noise; noise_sigma = sqrt(P / (2 * 10^(DB / 10))) per component with
//                                  P = nb_data_carriers * sum |tap|^2, the mean power of the modulator's symbols (NULL excluded) after the taps
//   --cfo-hz HZ                    carrier offset from the channel's 64-bit oscillator (cycles per sample = HZ / 2.048e6)
//   --timing-offset N              the signal N samples late (N >= 0 with channel-coded frames: they are produced one at a time)
//   --tap DELAY:RE:IM              repeatable, up to 8; delay in samples 0..2047; default one tap 0:1:0
//   --noise-seed N                 default 1
// Resampler (include/dabgpu.h "Resampler", DAB_Stream_Resampler): behind the channel, so that the noise is resampled too, as at a receiver's ADC.
//   --output-rate HZ               samples per second of the output (default 2048000; 1024000 .. 4096000), e.g. 2400000 for a tuner's capture
//   --clock-ppm X                  the ADC's sample period X ppm longer than nominal: step = 2048000 / HZ * (1 + X 1e-6) input samples per output
//   --frac-delay D                 the samples taken D of a 2.048 MHz sample late, 0 <= D < 1
// With any of them a frame's worth of input gives about 196608 / step samples; the last taps of a frame's last samples come with the next frame.
// Wideband capture (include/dabgpu.h "Channeliser", DAB_Stream_Combiner): behind the channel and the resampler, the combiner puts the block
// and up to 7 neighbours onto one stream at D times the output rate, as a wideband tuner would write them.
//   --wideband D                   1..8; the output has D x the samples (D x 2048000 per second, or D x --output-rate)
//   --centre-offset-hz F           the block lies F Hz above the centre of the capture (default 0)
//   --neighbour OFFSET_HZ:LEVEL_DB repeatable, up to 7: a block OFFSET_HZ from the wanted one, LEVEL_DB above it.  Neighbour k carries the
//                                  wanted block's own stream 50001 + 70006 k samples late (zeros before): the same frames, other content
//                                  at every instant
// The u8 scale leaves the sum of the blocks four standard deviations of head room, 127.5 / (4 sqrt(carriers / 2 x (1 + sum 10^(LEVEL_DB / 10)))),
// and is never above the single block's scale (no neighbour: the single block's bytes).  The quantiser truncates, as the modulator's does:
// its mean of half a step is a carrier at the CAPTURE's centre, which lies inside a block unless --centre-offset-hz puts it between two;
// the head room rule keeps it 13 dB under a block 20 dB below its neighbours.  The last 72 D / 2 - 1 samples of a frame's worth come with
// the next frame.
// Fading (include/dabgpu.h "Channel model, fading taps", DAB_Channel_Model::SetFading): taps with a Rayleigh or Rice gain and Doppler.
//   --doppler-hz F                 maximum Doppler shift, 0..1000 Hz; with it every tap fades (Rayleigh) unless --tap-kind says otherwise
//   --fading-seed S                default 1
//   --profile tu6|ra6|sfn2         taps and kinds of a preset (as recalled from COST 207, delays rounded to samples); not with --tap
//   --tap-kind K:static|rayleigh|rice:KDB   kind of tap K (list order, from 0); rice:KDB = Rice factor in dB, line of sight at cos 0.7
// Without --doppler-hz, or with --doppler-hz 0 and every tap static, no fading bank is made: the code path and the bytes are those of the
// channel options above.
// Interferer (include/dabgpu.h "Interferer", DAB_Interferer): behind the channel and in front of the resampler and the combiner, so that it is
// resampled and channelised like the noise.  IS_DB is the source's power, while its gate is on, relative to the signal power P that --snr-db
// refers to.
//   --interferer tone:OFFSET_HZ:IS_DB            repeatable, up to 4 in all: a carrier OFFSET_HZ from the block's centre
//   --interferer band:OFFSET_HZ:WIDTH_HZ:IS_DB   band-limited Gaussian noise WIDTH_HZ wide (8000 .. 2048000) around OFFSET_HZ
//   --interferer white:IS_DB                     white Gaussian noise over the whole sampled band (with a gate: bursts)
//   --interferer-gate PERIOD:ON[:OFFSET]         for the --interferer before it: on for ON of every PERIOD samples, from sample OFFSET on
//   --interferer-seed N                          default 1
// Front end (not in the reference; include/dabgpu.h "IQ balance", DAB_IQ_Balancer): the gain and phase error between I and Q and the DC
// term of a zero-IF tuner, applied last before the quantiser: behind the channel, the resampler and --wideband / --neighbour, so that a
// neighbour's mirror image lands where the tuner would put it.
//   --iq-imbalance GAIN_DB:PHASE_DEG   Q against I: -20..20 dB, -45..45 degrees; y = K1 x + K2 conj(x), K1 = (1 + g e^{-j phi}) / 2,
//                                      K2 = (1 - g e^{j phi}) / 2; 0.42:3 rejects the mirror frequency by 29 dB
//   --dc-offset RE:IM                  added behind it, in the units of the samples before the u8 scale (a data carrier has amplitude 1)
// TII (not in the reference, mode I; include/dabgpu.h "TII"):
//   --tii P:C[:AMP]                repeatable, up to 4: a transmitter with main id P (0..69), sub id C (0..23) and amplitude AMP (default 1 =
//                                  the power of a data carrier) fills the NULL period of every other frame, the first one included; the
//                                  frames between keep their zeros.  Not with channel-coded frames.
#include <stdio.h>
#include <stdlib.h>
#include <complex>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include <math.h>
#include <cmath>
#include <memory>

#include "dab/dabgpu_shared_context.h"
#include "dab/tx/dab_channel_model.h"
#include "dab/tx/dab_channeliser.h"
#include "dab/tx/dab_interferer.h"
#include "dab/tx/dab_resampler.h"
#include "dabgpu.h"
#include "ofdm/dab_iq_balancer.h"
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
    // channel-coded frames
    bool coded = false;
    std::vector<dabgpu_subchannel> subchannels;
    std::string fib_filename, payload_filename;
    unsigned long long seed = 1;
    // channel
    bool channel = false;
    bool have_snr = false;
    double snr_db = 0.0, cfo_hz = 0.0;
    long long timing_offset = 0;
    unsigned long long noise_seed = 1;
    struct Tap { int delay; float re, im; };
    std::vector<Tap> taps;
    // fading
    bool have_doppler = false;
    double doppler_hz = 0.0;
    unsigned long long fading_seed = 1;
    std::string profile;
    struct TapKind { int tap; int kind; float rice_k; };
    std::vector<TapKind> tap_kinds;
    std::vector<dabgpu_tii_tx> tii;
    // interferer: behind the channel, in front of the resampler
    struct Interferer { int kind; bool white; double offset_hz, width_hz, is_db; unsigned long long gate_period, gate_on; long long gate_offset; };
    std::vector<Interferer> interferers;
    unsigned long long interferer_seed = 1;
    // resampler: behind the channel
    bool resample = false;
    double clock_ppm = 0.0, frac_delay = 0.0, output_rate = 2.048e6;
    // combiner: behind the channel and the resampler
    int wideband = 0;
    double centre_offset_hz = 0.0;
    struct Neighbour { double offset_hz, level_db; };
    std::vector<Neighbour> neighbours;
    // front end: last before the quantiser
    bool front_end = false;
    double iq_gain_db = 0.0, iq_phase_deg = 0.0, dc_re = 0.0, dc_im = 0.0;
};

// --iq-imbalance / --dc-offset: the tuner's widely-linear map on the samples on their way to the quantiser
struct FrontEnd {
    DAB_IQ_Balancer bank;
    std::vector<uint8_t> bytes;
    explicit FrontEnd(const Args& args)
        : bank(DAB_IQ_Balancer::Impairment(args.iq_gain_db, args.iq_phase_deg, {args.dc_re, args.dc_im}), DABGPU_IQBAL_TILE) {}
    // the next samples of the output stream, quantised and written; false when a write fails
    bool Write(tcb::span<const std::complex<float>> x, float u8_scale, FILE* fp_out) {
        if (x.empty()) return true;
        bytes.resize(2 * x.size());
        bank.ApplyU8(bytes, x, u8_scale);
        const size_t nb_write = fwrite(bytes.data(), 2, x.size(), fp_out);
        if (nb_write != x.size()) { fprintf(stderr, "Failed to write out frame %zu/%zu\n", nb_write, x.size()); return false; }
        return true;
    }
};
static std::unique_ptr<FrontEnd> make_front_end(const Args& args) {
    if (!args.front_end) return nullptr;
    return std::make_unique<FrontEnd>(args);
}

// the wideband capture behind the channel and the resampler (include/dabgpu.h "Channeliser"): the block at --centre-offset-hz and its
// --neighbour blocks, which carry the block's own stream a fixed count of samples late, combined at --wideband times the block rate
struct Wideband {
    std::unique_ptr<DAB_Stream_Combiner> combiner;
    std::vector<size_t> delay;                                 // per row, in block samples (row 0: the wanted block, 0)
    std::vector<std::complex<float>> history, rows;            // the last max(delay) samples of the stream; the rows of one call
    std::vector<std::complex<float>> combined;                 // with a front end behind the combiner: its output as complex float
    std::vector<uint8_t> bytes;
    float u8_scale = 1.0f;
    Wideband(const Args& args, float block_u8_scale, int nb_carriers) {
        const double block_rate = args.output_rate, rate = block_rate * args.wideband;
        std::vector<dabgpu_channeliser_channel> channels{DAB_Channeliser::Channel(args.centre_offset_hz, rate)};
        delay.push_back(0);
        double power = 1.0;
        for (size_t k = 0; k < args.neighbours.size(); k++) {
            channels.push_back(DAB_Channeliser::Channel(args.centre_offset_hz + args.neighbours[k].offset_hz, rate, args.neighbours[k].level_db));
            delay.push_back(50001 + 70006 * k);
            power += std::pow(10.0, args.neighbours[k].level_db / 10.0);
        }
        // the block's edge (768 kHz) and its neighbour's (944 kHz) in cycles per sample of the block rate: 0.375 / 0.4609375 at 2.048 MS/s
        combiner = std::make_unique<DAB_Stream_Combiner>(args.wideband, channels, 768000.0 / block_rate, 944000.0 / block_rate);
        if (combiner->DesignError() > 1e-4)
            fprintf(stderr, "warning: at %.0f samples per second per block the combiner's 72 x %d taps reach %.3g (passband deviation + stopband level), "
                            "above the 1e-4 the design holds at 2048000\n", block_rate, args.wideband, combiner->DesignError());
        history.assign(delay.back(), std::complex<float>(0.0f, 0.0f));
        u8_scale = (float)std::min((double)block_u8_scale, 127.5 / (4.0 * std::sqrt(0.5 * (double)nb_carriers * power)));
    }
    // the next samples of the block stream through the combiner to the file; false when a write fails
    bool Write(tcb::span<const std::complex<float>> block, FILE* fp_out, FrontEnd* front = nullptr) {
        const size_t n = block.size(), H = history.size();
        history.insert(history.end(), block.begin(), block.end());          // stream samples (now - H) .. (now + n)
        rows.resize(delay.size() * n);
        for (size_t k = 0; k < delay.size(); k++) std::copy(history.begin() + (long)(H - delay[k]), history.begin() + (long)(H - delay[k] + n), rows.begin() + (long)(k * n));
        history.erase(history.begin(), history.begin() + (long)n);
        if (front) {
            combined.clear();
            combiner->Process(rows, combined);
            return front->Write(combined, u8_scale, fp_out);
        }
        bytes.clear();
        combiner->ProcessU8(rows, bytes, u8_scale);
        const size_t nb_write = fwrite(bytes.data(), 2, bytes.size() / 2, fp_out);
        if (nb_write != bytes.size() / 2) { fprintf(stderr, "Failed to write out frame %zu/%zu\n", nb_write, bytes.size() / 2); return false; }
        return true;
    }
};
static std::unique_ptr<Wideband> make_wideband(const Args& args, float block_u8_scale, int nb_carriers) {
    if (args.wideband == 0) return nullptr;
    return std::make_unique<Wideband>(args, block_u8_scale, nb_carriers);
}
// one frame of the channel's output on its way out: through the resampler where there is one, then the combiner
static bool write_wideband(Wideband& wide, DAB_Stream_Resampler* rs, tcb::span<const std::complex<float>> frame, std::vector<std::complex<float>>& resampled, FILE* fp_out,
                           FrontEnd* front = nullptr) {
    if (!rs) return wide.Write(frame, fp_out, front);
    resampled.clear();
    rs->Process(frame, resampled);
    return resampled.empty() ? true : wide.Write(resampled, fp_out, front);
}

// the receiver's ADC behind the channel (include/dabgpu.h "Resampler"): --output-rate HZ samples per second, its sample period --clock-ppm
// longer than nominal, the samples taken --frac-delay of a 2.048 MHz sample late
static std::unique_ptr<DAB_Stream_Resampler> make_resampler(const Args& args) {
    if (!args.resample) return nullptr;
    const uint64_t step = DAB_Resampler::StepWord(2.048e6, args.output_rate, args.clock_ppm);
    if (step == 0) throw std::runtime_error("--output-rate / --clock-ppm: not a sample rate");
    return std::make_unique<DAB_Stream_Resampler>(step, args.frac_delay);
}
// one frame of the 2.048 MHz stream through the resampler to the file; false when a write fails
static bool write_resampled(DAB_Stream_Resampler& rs, tcb::span<const std::complex<float>> frame, float u8_scale, std::vector<uint8_t>& bytes, FILE* fp_out,
                            FrontEnd* front = nullptr, std::vector<std::complex<float>>* resampled = nullptr) {
    if (front) {
        resampled->clear();
        rs.Process(frame, *resampled);
        return front->Write(*resampled, u8_scale, fp_out);
    }
    bytes.clear();
    rs.ProcessU8(frame, bytes, u8_scale);
    const size_t nb_write = fwrite(bytes.data(), 2, bytes.size() / 2, fp_out);
    if (nb_write != bytes.size() / 2) { fprintf(stderr, "Failed to write out frame %zu/%zu\n", nb_write, bytes.size() / 2); return false; }
    return true;
}

// the channel's parameters for a mode with nb_carriers data carriers
static dabgpu_channel_stream channel_params(const Args& args, int nb_carriers) {
    dabgpu_channel_stream P = {};
    P.freq_q64 = DAB_Channel_Model::FrequencyWord(args.cfo_hz);
    P.start = args.timing_offset;
    P.seed = args.noise_seed;
    P.gain = 1.0f;
    std::vector<Args::Tap> taps = args.taps;
    if (!args.profile.empty()) {
        dabgpu_channel_stream pp = {};
        dabgpu_channel_fading_spec ps = {};
        if (dabgpu_channel_profile(args.profile.c_str(), &pp, &ps) != DABGPU_OK) throw std::runtime_error(std::string("--profile: ") + dabgpu_last_error());
        for (int k = 0; k < pp.n_taps; k++) taps.push_back({pp.tap_delay[k], pp.tap_re[k], pp.tap_im[k]});
    }
    if (taps.empty()) taps.push_back({0, 1.0f, 0.0f});
    if (taps.size() > DABGPU_CHANNEL_MAX_TAPS) throw std::runtime_error("--tap: at most 8 taps");
    double h2 = 0.0;
    P.n_taps = (int)taps.size();
    for (size_t k = 0; k < taps.size(); k++) {
        P.tap_delay[k] = taps[k].delay; P.tap_re[k] = taps[k].re; P.tap_im[k] = taps[k].im;
        h2 += (double)taps[k].re * taps[k].re + (double)taps[k].im * taps[k].im;
    }
    P.noise_sigma = args.have_snr ? DAB_Channel_Model::NoiseSigma((double)nb_carriers * h2, args.snr_db) : 0.0f;
    return P;
}

// the interferer of the options for a signal of the channel's parameters (nullptr: none): every band source brings its own shape
static std::unique_ptr<DAB_Interferer> make_interferer(const Args& args, const dabgpu_channel_stream& cp, int nb_carriers) {
    if (args.interferers.empty()) return nullptr;
    double h2 = 0.0;
    for (int k = 0; k < cp.n_taps; k++) h2 += (double)cp.tap_re[k] * cp.tap_re[k] + (double)cp.tap_im[k] * cp.tap_im[k];
    dabgpu_interferer_stream P = {};
    std::vector<dabgpu_interferer_shape> shapes;
    P.seed = args.interferer_seed;
    P.n_sources = (int)args.interferers.size();
    for (size_t k = 0; k < args.interferers.size(); k++) {
        const Args::Interferer& I = args.interferers[k];
        dabgpu_interferer_source& S = P.source[k];
        S.kind = I.kind;
        S.shape = -1;
        if (I.kind == DABGPU_INTERFERER_BAND && !I.white) { S.shape = (int)shapes.size(); shapes.push_back(DAB_Interferer::Shape(I.width_hz)); }
        S.amp = DAB_Interferer::Amplitude((double)nb_carriers * h2, I.is_db);
        S.freq_q64 = DAB_Interferer::FrequencyWord(I.offset_hz);
        S.gate_period = I.gate_period; S.gate_on = I.gate_on; S.gate_offset = I.gate_offset;
    }
    return std::make_unique<DAB_Interferer>(P, shapes);
}

// tone:OFFSET_HZ:IS_DB | band:OFFSET_HZ:WIDTH_HZ:IS_DB | white:IS_DB
static Args::Interferer parse_interferer(const std::string& v) {
    std::vector<std::string> f;
    for (size_t at = 0;;) {
        const size_t c = v.find(':', at);
        f.push_back(v.substr(at, c == std::string::npos ? c : c - at));
        if (c == std::string::npos) break;
        at = c + 1;
    }
    if (f[0] == "tone" && f.size() == 3) return {DABGPU_INTERFERER_TONE, false, std::stod(f[1]), 0.0, std::stod(f[2]), 0, 0, 0};
    if (f[0] == "band" && f.size() == 4) return {DABGPU_INTERFERER_BAND, false, std::stod(f[1]), std::stod(f[2]), std::stod(f[3]), 0, 0, 0};
    if (f[0] == "white" && f.size() == 2) return {DABGPU_INTERFERER_BAND, true, 0.0, 0.0, std::stod(f[1]), 0, 0, 0};
    throw std::runtime_error("--interferer wants tone:OFFSET_HZ:IS_DB, band:OFFSET_HZ:WIDTH_HZ:IS_DB or white:IS_DB, got " + v);
}

// PERIOD:ON[:OFFSET] onto the interferer before it
static void parse_interferer_gate(const std::string& v, Args& args) {
    if (args.interferers.empty()) throw std::runtime_error("--interferer-gate applies to the --interferer before it");
    const size_t a = v.find(':'), b = v.find(':', a == std::string::npos ? a : a + 1);
    if (a == std::string::npos) throw std::runtime_error("--interferer-gate wants PERIOD:ON[:OFFSET], got " + v);
    Args::Interferer& I = args.interferers.back();
    I.gate_period = std::stoull(v.substr(0, a));
    I.gate_on = std::stoull(v.substr(a + 1, b == std::string::npos ? b : b - a - 1));
    I.gate_offset = b == std::string::npos ? 0 : std::stoll(v.substr(b + 1));
}

// the fading spec of the options; false: no tap fades (no fading bank is made)
static bool fading_spec(const Args& args, const dabgpu_channel_stream& P, dabgpu_channel_fading_spec& S) {
    S = dabgpu_channel_fading_spec{};
    if (!args.have_doppler) {
        if (!args.tap_kinds.empty() || !args.profile.empty()) throw std::runtime_error("--profile and --tap-kind want --doppler-hz");
        return false;
    }
    S.doppler_cycles = args.doppler_hz / 2.048e6;
    S.seed = args.fading_seed;
    if (!args.profile.empty()) {
        dabgpu_channel_stream pp = {};
        dabgpu_channel_profile(args.profile.c_str(), &pp, &S);             // (kinds, rice_k, los_cos; the name was checked with the taps)
        S.doppler_cycles = args.doppler_hz / 2.048e6; S.seed = args.fading_seed;
    } else
        for (int k = 0; k < P.n_taps; k++) S.kind[k] = DABGPU_TAP_FADING;
    for (const auto& t : args.tap_kinds) {
        if (t.tap < 0 || t.tap >= P.n_taps) throw std::runtime_error("--tap-kind: tap " + std::to_string(t.tap) + " of " + std::to_string(P.n_taps));
        S.kind[t.tap] = t.kind; S.rice_k[t.tap] = t.rice_k; S.los_cos[t.tap] = t.rice_k > 0.0f ? 0.7f : 0.0f;
    }
    bool any = false;
    for (int k = 0; k < P.n_taps; k++) any = any || S.kind[k] == DABGPU_TAP_FADING;
    return any;
}

// K:static | K:rayleigh | K:rice:KDB
static Args::TapKind parse_tap_kind(const std::string& v) {
    const size_t a = v.find(':');
    if (a == std::string::npos) throw std::runtime_error("--tap-kind wants K:static|rayleigh|rice:KDB, got " + v);
    const int tap = std::stoi(v.substr(0, a));
    const std::string kind = v.substr(a + 1);
    if (kind == "static") return {tap, DABGPU_TAP_STATIC, 0.0f};
    if (kind == "rayleigh") return {tap, DABGPU_TAP_FADING, 0.0f};
    if (kind.rfind("rice:", 0) == 0) return {tap, DABGPU_TAP_FADING, (float)std::pow(10.0, std::stod(kind.substr(5)) / 10.0)};
    throw std::runtime_error("--tap-kind wants K:static|rayleigh|rice:KDB, got " + v);
}

// DELAY:RE:IM
static Args::Tap parse_tap(const std::string& v) {
    const size_t a = v.find(':'), b = v.find(':', a == std::string::npos ? a : a + 1);
    if (a == std::string::npos || b == std::string::npos) throw std::runtime_error("--tap wants DELAY:RE:IM, got " + v);
    return {std::stoi(v.substr(0, a)), std::stof(v.substr(a + 1, b - a - 1)), std::stof(v.substr(b + 1))};
}

// P:C[:AMP]
static dabgpu_tii_tx parse_tii(const std::string& v) {
    const size_t a = v.find(':'), b = v.find(':', a == std::string::npos ? a : a + 1);
    if (a == std::string::npos) throw std::runtime_error("--tii wants P:C[:AMP], got " + v);
    const int p = std::stoi(v.substr(0, a)), c = std::stoi(v.substr(a + 1, b == std::string::npos ? b : b - a - 1));
    if (p < 0 || p >= DABGPU_TII_NB_MAIN || c < 0 || c >= DABGPU_TII_COMBS) throw std::runtime_error("--tii: main id 0..69 and sub id 0..23, got " + v);
    return {(uint8_t)p, (uint8_t)c, b == std::string::npos ? 1.0f : std::stof(v.substr(b + 1))};
}

// START:LENGTH:PROT
static dabgpu_subchannel parse_subchannel(const std::string& v) {
    const size_t a = v.find(':'), b = v.find(':', a == std::string::npos ? a : a + 1);
    if (a == std::string::npos || b == std::string::npos) throw std::runtime_error("--subchannel wants START:LENGTH:PROT, got " + v);
    dabgpu_subchannel sc = {};
    sc.start_address = std::stoi(v.substr(0, a));
    sc.length = std::stoi(v.substr(a + 1, b - a - 1));
    const std::string prot = v.substr(b + 1);
    if (prot.rfind("uep", 0) == 0 && prot.size() > 3) { sc.is_uep = 1; sc.uep_prot_index = std::stoi(prot.substr(3)); }
    else if (prot.size() == 6 && prot.rfind("eep", 0) == 0 && prot[4] == '-' && (prot[5] == 'A' || prot[5] == 'B') && prot[3] >= '1' && prot[3] <= '4') {
        sc.eep_prot_level = prot[3] - '1'; sc.eep_type = prot[5] == 'B';
    } else throw std::runtime_error("--subchannel: protection " + prot + " (eepL-A, eepL-B or uepROW)");
    return sc;
}

// a file's bytes, or n random ones; read cyclically
struct ByteSource {
    std::vector<uint8_t> bytes;
    size_t at = 0;
    ByteSource(const std::string& filename, std::mt19937_64& rng, size_t n_random) {
        if (filename.empty()) {
            bytes.resize(n_random);
            for (auto& b : bytes) b = (uint8_t)(rng() & 0xFF);
            return;
        }
        FILE* fp = fopen(filename.c_str(), "rb");
        if (!fp) throw std::runtime_error("Failed to open input file: '" + filename + "'");
        uint8_t buf[65536];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
        fclose(fp);
        if (bytes.empty()) throw std::runtime_error("Input file is empty: '" + filename + "'");
    }
    void read(uint8_t* dst, size_t n) { for (size_t i = 0; i < n; i++) { dst[i] = bytes[at]; at = (at + 1) % bytes.size(); } }
};

// frames channel coded on the device from the FIB bodies and the payload; mode I
static int run_coded(const Args& args, FILE* fp_out) {
    if (args.transmission_mode != 1) throw std::runtime_error("channel-coded frames are transmission mode I only");
    const int n_sub = (int)args.subchannels.size();
    dabgpu_tx_bank* bank = nullptr;
    int st = dabgpu_tx_bank_create(dabgpu_shared_context(), 1, n_sub ? args.subchannels.data() : nullptr, n_sub, &bank);
    if (st != DABGPU_OK) { fprintf(stderr, "Failed to create the channel encoder: %s -- %s\n", dabgpu_strerror(st), dabgpu_last_error()); return 1; }
    std::vector<dabgpu_tx_sub_plan> plans((size_t)n_sub + 1);
    uint32_t cif_in = 0;
    dabgpu_tx_encode_plan(n_sub ? args.subchannels.data() : nullptr, n_sub, plans.data(), &cif_in, nullptr, 0, nullptr, nullptr);
    std::mt19937_64 rng(args.seed);
    // (random data: 64 frames' worth, then it repeats)
    ByteSource fibs(args.fib_filename, rng, 64 * 360), payload(args.payload_filename, rng, 64 * 4 * (size_t)cif_in + 1);
    const float frequency_norm = (args.frequency != 0.0f) ? args.frequency / 2.048e6f : 0.0f;
    std::vector<uint8_t> fib(360), pay(4 * (size_t)cif_in + 4), quantised(2 * (size_t)DABGPU_NB_FRAME_SAMPLES);
    // channel: the frames come one at a time, so the channel sees a window of the previous and the current frame and `start` moves with it
    const size_t S = DABGPU_NB_FRAME_SAMPLES;
    std::unique_ptr<DAB_Channel_Model> channel;
    dabgpu_channel_stream cp = {};
    std::vector<std::complex<float>> window;
    if (args.channel) {
        if (args.timing_offset < 0) throw std::runtime_error("--timing-offset must be >= 0 with channel-coded frames");
        cp = channel_params(args, 1536);
        channel = std::make_unique<DAB_Channel_Model>(cp);
        dabgpu_channel_fading_spec spec;
        if (fading_spec(args, cp, spec)) channel->SetFading(spec);
        window.assign(2 * S, std::complex<float>(0.0f, 0.0f));
    }
    auto interferer = make_interferer(args, cp, 1536);
    auto resampler = make_resampler(args);
    const float u8_scale = (1.0f / 1536.0f * 4.0f) * 127.5f;
    auto wide = make_wideband(args, u8_scale, 1536);
    auto front = make_front_end(args);
    std::vector<std::complex<float>> impaired((resampler || wide || interferer || front) ? S : 0), resampled;
    int rc = 0;
    for (long long k = 0; args.frames < 0 || k < args.frames; k++) {
        fibs.read(fib.data(), 360);
        payload.read(pay.data(), 4 * (size_t)cif_in);
        if (channel) {
            std::copy(window.begin() + (long)S, window.end(), window.begin());
            st = dabgpu_tx_bank_transmit_frames_host_sync(bank, fib.data(), pay.data(), 1, frequency_norm, window.data() + S, DABGPU_IQ_RAW_F32L);
            if (st == DABGPU_OK) {
                dabgpu_channel_stream now = cp;
                now.start = cp.start + (k - 1) * (long long)S;             // window sample 0 = stream sample (k - 1) S
                channel->SetParams(now);
                if (resampler || wide || interferer || front) channel->Apply(impaired, window, false);
                else channel->ApplyU8(quantised, window, false, u8_scale);
                if (interferer && (resampler || wide || front)) interferer->Apply(impaired, impaired);
                else if (interferer) interferer->ApplyU8(quantised, impaired, u8_scale);
            }
        } else
        st = dabgpu_tx_bank_transmit_frames_host_sync(bank, fib.data(), pay.data(), 1, frequency_norm, quantised.data(), DABGPU_IQ_RAW_U8);
        if (st != DABGPU_OK) { fprintf(stderr, "Failed to create the OFDM frame: %s -- %s\n", dabgpu_strerror(st), dabgpu_last_error()); rc = 1; break; }
        if (wide) {
            if (!write_wideband(*wide, resampler.get(), impaired, resampled, fp_out, front.get())) break;
            continue;
        }
        if (resampler) {
            if (!write_resampled(*resampler, impaired, u8_scale, quantised, fp_out, front.get(), &resampled)) break;
            continue;
        }
        if (front) {                                                         // (--iq-imbalance makes the channel: `impaired` holds the frame)
            if (!front->Write(impaired, u8_scale, fp_out)) break;
            continue;
        }
        const size_t nb_write = fwrite(quantised.data(), 2, DABGPU_NB_FRAME_SAMPLES, fp_out);
        if (nb_write != DABGPU_NB_FRAME_SAMPLES) { fprintf(stderr, "Failed to write out frame %zu/%d\n", nb_write, DABGPU_NB_FRAME_SAMPLES); break; }
    }
    dabgpu_tx_bank_destroy(bank);
    return rc;
}

static void usage(const char* argv0) {
    fprintf(stderr, "usage: %s [-m|--transmission-mode 1..4] [-f|--frequency HZ] [-o|--output FILE] [--frames N]\n"
                    "          [--subchannel START:LENGTH:eepL-A|eepL-B|uepROW]... [--fib-file FILE] [--payload-file FILE] [--seed N]\n"
                    "          [--snr-db DB] [--cfo-hz HZ] [--timing-offset N] [--tap DELAY:RE:IM]... [--noise-seed N] [--tii P:C[:AMP]]...\n"
                    "          [--doppler-hz F] [--fading-seed S] [--profile tu6|ra6|sfn2] [--tap-kind K:static|rayleigh|rice:KDB]...\n"
                    "          [--interferer tone:OFFSET_HZ:IS_DB|band:OFFSET_HZ:WIDTH_HZ:IS_DB|white:IS_DB]... [--interferer-gate PERIOD:ON[:OFFSET]]\n"
                    "          [--interferer-seed N] [--clock-ppm X] [--frac-delay D] [--output-rate HZ]\n"
                    "          [--wideband D] [--centre-offset-hz F] [--neighbour OFFSET_HZ:LEVEL_DB]...\n"
                    "          [--iq-imbalance GAIN_DB:PHASE_DEG] [--dc-offset RE:IM]\n"
                    "Simulates an OFDM transmitter sending random data (8-bit IQ at 2.048 MHz; default output stdout);\n"
                    "with --subchannel / --fib-file / --payload-file / --seed the frames are channel coded (mode I) from that data;\n"
                    "with --snr-db / --cfo-hz / --timing-offset / --tap / --noise-seed the signal passes a channel on the device before it is\n"
                    "quantised: taps (default 0:1:0, delays 0..2047 samples), carrier offset, delay, white Gaussian noise with\n"
                    "  noise_sigma = sqrt(P / (2 * 10^(DB / 10))) per component, P = nb_data_carriers * sum |tap|^2\n"
                    "(the mean power of the modulator's symbols after the taps; the NULL period is not counted);\n"
                    "with --doppler-hz F (0..1000) the taps fade (Rayleigh; --tap-kind sets single taps static or Rice with a factor in dB,\n"
                    "--profile takes taps and kinds from a preset as recalled from COST 207), unit mean power each, seeded by --fading-seed;\n"
                    "with --interferer (up to 4) a carrier, a band of Gaussian noise or white noise is added behind the channel, IS_DB relative to the\n"
                    "signal power P of --snr-db while its --interferer-gate (on for ON of every PERIOD samples) is on, seeded by --interferer-seed;\n"
                    "with --clock-ppm X / --frac-delay D / --output-rate HZ the signal is resampled behind the channel (the noise too, as at a\n"
                    "receiver's ADC): HZ samples per second (default 2048000), every sample period X ppm longer, D of a sample late;\n"
                    "with --wideband D (1..8) the block goes onto a capture at D times the rate, --centre-offset-hz F above its centre, with up to 7\n"
                    "--neighbour blocks OFFSET_HZ from it and LEVEL_DB above it (the block's own stream, a fixed count of samples late);\n"
                    "with --tii (mode I, up to 4) the NULL period of every other frame carries those transmitters' identification\n", argv0);
}

static bool parse_args(int argc, char** argv, Args& args) {
    bool have_wide_option = false, have_wideband = false;
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
        else if (a == "--subchannel") { args.subchannels.push_back(parse_subchannel(value())); args.coded = true; }
        else if (a == "--fib-file") { args.fib_filename = value(); args.coded = true; }
        else if (a == "--payload-file") { args.payload_filename = value(); args.coded = true; }
        else if (a == "--seed") { args.seed = std::stoull(value()); args.coded = true; }
        else if (a == "--snr-db") { args.snr_db = std::stod(value()); args.have_snr = true; args.channel = true; }
        else if (a == "--cfo-hz") { args.cfo_hz = std::stod(value()); args.channel = true; }
        else if (a == "--timing-offset") { args.timing_offset = std::stoll(value()); args.channel = true; }
        else if (a == "--tap") { args.taps.push_back(parse_tap(value())); args.channel = true; }
        else if (a == "--noise-seed") { args.noise_seed = std::stoull(value()); args.channel = true; }
        else if (a == "--doppler-hz") { args.doppler_hz = std::stod(value()); args.have_doppler = true; args.channel = true; }
        else if (a == "--fading-seed") { args.fading_seed = std::stoull(value()); args.channel = true; }
        else if (a == "--profile") { args.profile = value(); args.channel = true; }
        else if (a == "--tap-kind") { args.tap_kinds.push_back(parse_tap_kind(value())); args.channel = true; }
        else if (a == "--tii") args.tii.push_back(parse_tii(value()));
        else if (a == "--interferer") { args.interferers.push_back(parse_interferer(value())); args.channel = true; }
        else if (a == "--interferer-gate") parse_interferer_gate(value(), args);
        else if (a == "--interferer-seed") args.interferer_seed = std::stoull(value());
        else if (a == "--clock-ppm") { args.clock_ppm = std::stod(value()); args.resample = true; }
        else if (a == "--frac-delay") { args.frac_delay = std::stod(value()); args.resample = true; }
        else if (a == "--output-rate") { args.output_rate = std::stod(value()); args.resample = true; }
        else if (a == "--wideband") { args.wideband = std::stoi(value()); have_wideband = true; }
        else if (a == "--centre-offset-hz") { args.centre_offset_hz = std::stod(value()); have_wide_option = true; }
        else if (a == "--iq-imbalance" || a == "--dc-offset") {
            const std::string v = value();
            const size_t colon = v.find(':');
            if (colon == std::string::npos) throw std::runtime_error(a + " expects two numbers, A:B: '" + v + "'");
            const double first = std::stod(v.substr(0, colon)), second = std::stod(v.substr(colon + 1));
            if (a == "--iq-imbalance") { args.iq_gain_db = first; args.iq_phase_deg = second; } else { args.dc_re = first; args.dc_im = second; }
            args.front_end = true; args.channel = true;
        }
        else if (a == "--neighbour") {
            const std::string v = value();
            const size_t colon = v.find(':');
            if (colon == std::string::npos) throw std::runtime_error("--neighbour expects OFFSET_HZ:LEVEL_DB: '" + v + "'");
            args.neighbours.push_back({std::stod(v.substr(0, colon)), std::stod(v.substr(colon + 1))});
            have_wide_option = true;
        }
        else if (a == "-h" || a == "--help") return false;
        else throw std::runtime_error("unknown argument: " + a);
    }
    if (have_wide_option && !have_wideband) throw std::runtime_error("--centre-offset-hz / --neighbour need --wideband D");
    if (have_wideband) {
        // the combiner stands behind the channel (and the resampler): without channel options that is the identity channel
        args.channel = true;
        if (args.wideband < 1 || args.wideband > DABGPU_CHANNELISER_MAX_DECIM) throw std::runtime_error("--wideband: 1 .. 8");
        if (args.neighbours.size() > DABGPU_CHANNELISER_MAX_CHANNELS - 1) throw std::runtime_error("--neighbour: at most 7");
        // the filter's edges are the block's (768 kHz) and its neighbour's (944 kHz) over the block rate: the stopband has to fit 0.5 x D
        if (!(944000.0 / args.output_rate <= 0.5 * args.wideband))
            throw std::runtime_error("--wideband: the capture's rate (D x --output-rate) does not hold a block and its neighbour's edge: at least 1888000 samples per second");
        const double half = 0.5 * args.output_rate * args.wideband;
        if (!(std::fabs(args.centre_offset_hz) <= half)) throw std::runtime_error("--centre-offset-hz: within half of the capture's rate either way");
        for (const auto& nb : args.neighbours) {
            if (!(std::fabs(args.centre_offset_hz + nb.offset_hz) <= half)) throw std::runtime_error("--neighbour: the block lies outside the capture");
            if (!(std::fabs(nb.level_db) <= 100.0)) throw std::runtime_error("--neighbour: level -100 .. 100 dB");
        }
    }
    if (args.resample) {
        // the resampler stands behind the channel: without channel options that is the identity channel, which returns its input bit for bit
        args.channel = true;
        if (!(args.frac_delay >= 0.0 && args.frac_delay < 1.0)) throw std::runtime_error("--frac-delay is a fraction of a sample: 0 <= D < 1");
        if (!(args.output_rate >= 1.024e6 && args.output_rate <= 4.096e6)) throw std::runtime_error("--output-rate: 1024000 .. 4096000");
        if (!(std::fabs(args.clock_ppm) <= 1000.0)) throw std::runtime_error("--clock-ppm: -1000 .. 1000");
    }
    if (args.front_end) {
        if (!(std::fabs(args.iq_gain_db) <= 20.0) || !(std::fabs(args.iq_phase_deg) <= 45.0)) throw std::runtime_error("--iq-imbalance: -20 .. 20 dB, -45 .. 45 degrees");
        if (!std::isfinite(args.dc_re) || !std::isfinite(args.dc_im)) throw std::runtime_error("--dc-offset: two finite numbers");
    }
    if (!args.profile.empty() && !args.taps.empty()) throw std::runtime_error("--profile is not available with --tap");
    if (args.interferers.size() > DABGPU_INTERFERER_MAX) throw std::runtime_error("--interferer: at most 4 sources");
    if (args.tii.size() > DABGPU_TII_MAX_TX) throw std::runtime_error("--tii: at most 4 transmitters");
    if (!args.tii.empty() && args.coded) throw std::runtime_error("--tii is not available with channel-coded frames");
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
        if (args.coded) {
            const int rc = run_coded(args, fp_out);
            if (fp_out != stdout) fclose(fp_out);
            else fflush(fp_out);
            return rc;
        }
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
        // with TII the transmission is two frames long: the payload twice, the comb in the first NULL period only
        const size_t n_tx = args.tii.empty() ? 1 : 2;
        if (n_tx == 2) frame_bytes_buf.insert(frame_bytes_buf.end(), frame_bytes_buf.begin(), frame_bytes_buf.begin() + (long)nb_frame_bytes);
        dabgpu_tii_tx tii_list[2 * DABGPU_TII_MAX_TX] = {};
        std::copy(args.tii.begin(), args.tii.end(), tii_list);
        const uint8_t tii_count[2] = {(uint8_t)args.tii.size(), 0};
        auto modulate = [&](void* out, int format) {
            if (n_tx == 2)
                return dabgpu_ofdm_modulate_frames_tii_host_sync(dabgpu_shared_context(), args.transmission_mode, frame_bytes_buf.data(),
                                                                 DABGPU_TX_PAYLOAD_REFERENCE, 2, reinterpret_cast<const float*>(prs_fft_ref.data()),
                                                                 frequency_norm, out, format, tii_list, tii_count);
            return dabgpu_ofdm_modulate_frames_host_sync(dabgpu_shared_context(), args.transmission_mode, frame_bytes_buf.data(),
                                                         DABGPU_TX_PAYLOAD_REFERENCE, 1, reinterpret_cast<const float*>(prs_fft_ref.data()),
                                                         frequency_norm, out, format);
        };
        auto quantised = std::vector<uint8_t>(2 * frame_size * n_tx);
        if (args.channel) {
            // the transmission once as complex float; the channel reads it as one that repeats
            auto frame = std::vector<std::complex<float>>(frame_size * n_tx);
            quantised.resize(2 * frame_size);
            const int st = modulate(frame.data(), DABGPU_IQ_RAW_F32L);
            if (st != DABGPU_OK) {
                fprintf(stderr, "Failed to create the OFDM frame: %s -- %s\n", dabgpu_strerror(st), dabgpu_last_error());
                return 1;
            }
            const dabgpu_channel_stream cp = channel_params(args, (int)params.nb_data_carriers);
            DAB_Channel_Model channel(cp);
            dabgpu_channel_fading_spec spec;
            if (fading_spec(args, cp, spec)) channel.SetFading(spec);
            const float u8_scale = (1.0f / (float)params.nb_data_carriers * 4.0f) * 127.5f;
            auto interferer = make_interferer(args, cp, (int)params.nb_data_carriers);
            auto resampler = make_resampler(args);
            auto wide = make_wideband(args, u8_scale, (int)params.nb_data_carriers);
            auto front = make_front_end(args);
            std::vector<std::complex<float>> impaired((resampler || wide || interferer || front) ? frame_size : 0), resampled;
            for (long long k = 0; args.frames < 0 || k < args.frames; k++) {
                if (wide) {
                    channel.Apply(impaired, frame, true);
                    if (interferer) interferer->Apply(impaired, impaired);
                    if (!write_wideband(*wide, resampler.get(), impaired, resampled, fp_out, front.get())) break;
                    continue;
                }
                if (resampler) {
                    channel.Apply(impaired, frame, true);
                    if (interferer) interferer->Apply(impaired, impaired);
                    if (!write_resampled(*resampler, impaired, u8_scale, quantised, fp_out, front.get(), &resampled)) break;
                    continue;
                }
                if (front) {
                    channel.Apply(impaired, frame, true);
                    if (interferer) interferer->Apply(impaired, impaired);
                    if (!front->Write(impaired, u8_scale, fp_out)) break;
                    continue;
                }
                if (interferer) {
                    channel.Apply(impaired, frame, true);
                    interferer->ApplyU8(quantised, impaired, u8_scale);
                } else
                channel.ApplyU8(quantised, frame, true, u8_scale);
                const size_t nb_write = fwrite(quantised.data(), 2, frame_size, fp_out);
                if (nb_write != frame_size) {
                    fprintf(stderr, "Failed to write out frame %zu/%zu\n", nb_write, frame_size);
                    break;
                }
            }
            if (fp_out != stdout) fclose(fp_out);
            else fflush(fp_out);
            return 0;
        }
        const int st = modulate(quantised.data(), DABGPU_IQ_RAW_U8);
        if (st != DABGPU_OK) {
            fprintf(stderr, "Failed to create the OFDM frame: %s -- %s\n", dabgpu_strerror(st), dabgpu_last_error());
            return 1;
        }
        for (long long k = 0; args.frames < 0 || k < args.frames; k++) {
            const size_t nb_write = fwrite(quantised.data() + 2 * frame_size * ((size_t)k % n_tx), 2, frame_size, fp_out);
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
