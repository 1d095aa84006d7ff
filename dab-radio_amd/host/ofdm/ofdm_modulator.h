// ofdm/ofdm_modulator.h -- OFDM_Modulator with the reference's public interface (src/ofdm/ofdm_modulator.h), re-implemented over the
// MI355X C ABI (include/dabgpu.h, dabgpu_ofdm_modulate_frames_host_sync): the DQPSK chain, the inverse transforms and the cyclic
// prefixes of a frame run on the device, in one call per ProcessBlock.
//   params        one of the four DAB geometries (get_DAB_OFDM_params); anything else has no device path and throws std::runtime_error
//   prs_fft_ref   the PRS spectrum (nb_fft bins) the frame starts from -- the caller's, as given
//   ProcessBlock  frame_out_buf = nb_null_period + nb_symbol_period * nb_frame_symbols samples, NULL first; data_in_buf =
//                 (nb_frame_symbols - 1) * nb_data_carriers / 4 bytes, 2 bits per carrier in natural carrier order.  Wrong sizes return
//                 false and write nothing (ofdm_modulator.cpp:54-63); a device failure throws std::runtime_error.
// Every ProcessBlock starts the chain from the PRS again (ofdm_modulator.cpp:73-76): the object keeps no state between frames.
//   SetTII        (not in the reference; mode I; include/dabgpu.h "TII") the transmitters whose comb fills the NULL period of every frame
//                 modulated from now on, at most DABGPU_TII_MAX_TX; an empty list (the default) keeps the zeros.  TII is sent in alternate
//                 frames: the caller sets and clears the list between ProcessBlock calls.  A list the library refuses (main id >= 70,
//                 sub id >= 24, an amplitude that is not finite, another mode) throws std::runtime_error and leaves the list as it was.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <complex>
#include <vector>
#include "utility/span.h"
#include "./ofdm_params.h"
#include "dabgpu.h"

class OFDM_Modulator
{
private:
    const OFDM_Params m_params;
    int m_mode = 0;
    const size_t m_frame_out_size;
    const size_t m_data_in_size;
    std::vector<std::complex<float>> m_prs_fft_ref;
    std::vector<dabgpu_tii_tx> m_tii;
public:
    OFDM_Modulator(
        const OFDM_Params& params,
        tcb::span<const std::complex<float>> prs_fft_ref);
    ~OFDM_Modulator();
    bool ProcessBlock(
        tcb::span<std::complex<float>> frame_out_buf,
        tcb::span<const uint8_t> data_in_buf);
    void SetTII(tcb::span<const dabgpu_tii_tx> transmitters);
};
