// tx_mirror_harness.cpp -- drives the OFDM_Modulator mirror class (dab-radio_amd/host/ofdm/ofdm_modulator.h) for
// tests/test_gpu_ofdm_modulator.py, which compiles it against libdab_mirror.a + libdabgpu.so.
//   tx_mirror_harness MODE PAYLOAD_FILE PRS_FILE|- OUT_FILE
// PRS_FILE: nb_fft complex float (- = get_DAB_PRS_reference of the mode).  Writes ProcessBlock's frame to OUT_FILE (complex float),
// after checking that a payload one byte short and an output one sample short return false and leave the output untouched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <complex>
#include <string>
#include <vector>

#include "ofdm/dab_ofdm_params_ref.h"
#include "ofdm/dab_prs_ref.h"
#include "ofdm/ofdm_modulator.h"

static std::vector<uint8_t> read_file(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s MODE PAYLOAD PRS|- OUT\n", argv[0]); return 2; }
    const int mode = atoi(argv[1]);
    const OFDM_Params params = get_DAB_OFDM_params(mode);
    std::vector<std::complex<float>> prs(params.nb_fft);
    if (std::string(argv[3]) == "-") {
        get_DAB_PRS_reference(mode, prs);
    } else {
        const auto raw = read_file(argv[3]);
        if (raw.size() != prs.size() * sizeof(prs[0])) { fprintf(stderr, "PRS file: %zu bytes\n", raw.size()); return 2; }
        memcpy(static_cast<void*>(prs.data()), raw.data(), raw.size());
    }
    const auto payload = read_file(argv[2]);
    const size_t frame_size = params.nb_null_period + params.nb_symbol_period * params.nb_frame_symbols;
    OFDM_Modulator mod(params, prs);

    const std::complex<float> sentinel(12345.0f, -6789.0f);
    std::vector<std::complex<float>> out(frame_size + 1, sentinel);
    auto untouched = [&]() { for (const auto& v : out) if (v != sentinel) return false; return true; };
    if (payload.size() >= 1 && mod.ProcessBlock(tcb::span<std::complex<float>>(out.data(), frame_size),
                                                tcb::span<const uint8_t>(payload.data(), payload.size() - 1))) {
        fprintf(stderr, "payload one byte short accepted\n"); return 1;
    }
    if (!untouched()) { fprintf(stderr, "output written on a short payload\n"); return 1; }
    if (mod.ProcessBlock(tcb::span<std::complex<float>>(out.data(), frame_size - 1), payload)) {
        fprintf(stderr, "output one sample short accepted\n"); return 1;
    }
    if (!untouched()) { fprintf(stderr, "output written on a short output buffer\n"); return 1; }
    if (!mod.ProcessBlock(tcb::span<std::complex<float>>(out.data(), frame_size), payload)) {
        fprintf(stderr, "ProcessBlock refused a frame of the right sizes\n"); return 1;
    }
    if (out[frame_size] != sentinel) { fprintf(stderr, "ProcessBlock wrote past the frame\n"); return 1; }
    FILE* f = fopen(argv[4], "wb");
    if (!f || fwrite(out.data(), sizeof(out[0]), frame_size, f) != frame_size) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
    fclose(f);
    printf("ok mode %d: %zu samples\n", mode, frame_size);
    return 0;
}
