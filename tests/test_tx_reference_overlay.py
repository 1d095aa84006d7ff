"""CPU (build container only; skips where the reference tree is absent): the OFDM_Modulator mirror (dab-radio_amd/host/ofdm/
ofdm_modulator.{h,cpp}) laid over the reference's own files in a scratch copy of its src/ (INTEGRATION.md), and a translation unit doing what
examples/simulate_transmitter.cpp:145-165 does -- params, PRS and mapper from the reference's own ofdm/*_ref.cpp, its utility/span.h and
ofdm_params.h -- compiled there and linked against libdabgpu.so (link check only).  The example itself needs the empty argparse submodule."""
import os
import shutil

import pytest

import ref_overlay as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOD_FILES = ["ofdm/ofdm_modulator.h", "ofdm/ofdm_modulator.cpp"]

TU = r"""
#include <stdint.h>
#include <complex>
#include <vector>
#include "utility/span.h"
#include "ofdm/dab_mapper_ref.h"
#include "ofdm/dab_ofdm_params_ref.h"
#include "ofdm/dab_prs_ref.h"
#include "ofdm/ofdm_modulator.h"
#include "ofdm/ofdm_params.h"

int main(int argc, char**) {
    const int transmission_mode = argc;
    const auto params = get_DAB_OFDM_params(transmission_mode);
    auto prs_fft_ref = std::vector<std::complex<float>>(params.nb_fft);
    auto carrier_mapper = std::vector<int>(params.nb_data_carriers);
    get_DAB_PRS_reference(transmission_mode, prs_fft_ref);
    get_DAB_mapper_ref(carrier_mapper, params.nb_fft);
    const size_t frame_size = params.nb_null_period + params.nb_symbol_period*params.nb_frame_symbols;
    const size_t nb_frame_bits = (params.nb_frame_symbols-1)*params.nb_data_carriers*2;
    const size_t nb_frame_bytes = nb_frame_bits/8;
    auto frame_bytes_buf = std::vector<uint8_t>(nb_frame_bytes);
    auto ofdm_mod = OFDM_Modulator(params, prs_fft_ref);
    auto frame_out_buf = std::vector<std::complex<float>>(frame_size);
    auto res = ofdm_mod.ProcessBlock(frame_out_buf, frame_bytes_buf);
    return res ? 0 : 1;
}
"""


def test_simulate_transmitter_body_links_against_the_mirror_modulator(tmp_path):
    ok, why = RO.available()
    if not ok:
        pytest.skip(why)
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    ov = RO.Overlay(tmp_path / "ov")
    for f in MOD_FILES:
        shutil.copyfile(os.path.join(RO.HOST, f), os.path.join(ov.src, f))
    tu = tmp_path / "simulate_transmitter_body.cpp"
    tu.write_text(TU)
    objs = [ov.compile(f) for f in RO.REF_OFDM_SIDE]
    objs += [ov.compile(str(tu)), ov.compile("ofdm/ofdm_modulator.cpp"), ov.compile("dab/dabgpu_shared_context.cpp")]
    exe = ov.link(objs, "simulate_transmitter_body", backend="gpu")
    assert os.path.exists(exe)
