// clock_class_harness.cpp -- DAB_Clock_Tracker for tests/test_gpu_clock_class.py: one receiver, n frames in sequence, the state carried.
//   clock_class_harness <dir> <n_frames> <gain>
// Reads <dir>/dq.bin ([n][75][1536] complex float).  Frame n / 2 is followed by an all-zero frame (a fade: skipped, the state kept).
// Writes out.bin ([n][75][1536] complex float: the de-rotated frames), slope.bin ([n] int64), corr.bin ([n][2] float), valid.bin
// ([n] int32), ppm.bin ([n] double).  One line on stdout: frames=N
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ofdm/dab_clock_tracker.h"

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
    if (argc != 4) { std::fprintf(stderr, "usage: %s dir n_frames gain\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const size_t n = (size_t)std::atol(argv[2]);
    const float gain = std::strtof(argv[3], nullptr);
    const size_t frame = DAB_Clock_Tracker::NB_PRODUCTS;
    auto dq = load<std::complex<float>>(dir + "/dq.bin", n * frame);
    bool threw = false;
    try { DAB_Clock_Tracker bad(0.0f); } catch (const std::invalid_argument&) { threw = true; }
    DAB_Clock_Tracker trk;
    // what is refused changes nothing
    if (!threw || trk.SetGain(1.5f) || trk.SetGain(-1.0f) || trk.GetGain() != 1.0f || !trk.SetGain(gain) ||
        trk.Track(tcb::span<std::complex<float>>(dq.data(), frame - 1)) || trk.IsValid() || trk.GetSlope() != 0 || trk.GetPpm() != 0.0) {
        std::fprintf(stderr, "a wrong argument was accepted\n"); return 1;
    }
    std::ofstream f_o(dir + "/out.bin", std::ios::binary), f_s(dir + "/slope.bin", std::ios::binary), f_c(dir + "/corr.bin", std::ios::binary),
        f_v(dir + "/valid.bin", std::ios::binary), f_p(dir + "/ppm.bin", std::ios::binary);
    for (size_t i = 0; i < n; i++) {
        const bool ok = trk.Track(tcb::span<std::complex<float>>(dq.data() + i * frame, frame));
        if (ok != trk.IsValid()) { std::fprintf(stderr, "Track and IsValid disagree at frame %zu\n", i); return 1; }
        const int64_t s = trk.GetSlope();
        const int32_t v = ok ? 1 : 0;
        const double ppm = trk.GetPpm();
        put(f_o, dq.data() + i * frame, frame); put(f_s, &s, 1); put(f_c, trk.GetCorrelation().data(), 2); put(f_v, &v, 1); put(f_p, &ppm, 1);
        if (i == n / 2) {                                             // the signal fades: the state survives
            std::vector<std::complex<float>> zero(frame);
            if (trk.Track(zero) || trk.IsValid() || trk.GetSlope() != s) { std::fprintf(stderr, "an all-zero frame was not skipped\n"); return 1; }
        }
    }
    trk.Reset();
    if (trk.GetSlope() != 0 || trk.IsValid() || trk.GetGain() != gain) { std::fprintf(stderr, "Reset\n"); return 1; }
    std::printf("frames=%zu\n", n);
    return 0;
}
