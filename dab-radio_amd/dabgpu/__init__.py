"""dabgpu -- thin ctypes binding over the C ABI in include/dabgpu.h (dab-radio_amd/libdabgpu.so).

This is plumbing for tests and bench.py: device memory comes from torch tensors (or any object with
`data_ptr()`), the compute is the hand-written HIP in dab-radio_amd/csrc.  There is NO CPU fallback:
if the shared library is missing or no gfx950 device is present, calls raise DabGpuError.
"""
import ctypes as C
import os

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG_DIR)
LIB_PATH = os.environ.get("DABGPU_LIB") or os.path.join(_ROOT, "libdabgpu.so")   # DABGPU_LIB: development A/B builds

NB_FRAME_SYMBOLS = 76
NB_SYMBOL_PERIOD = 2552
NB_NULL_PERIOD = 2656
NB_FFT = 2048
NB_CP = 504
NB_CARRIERS = 1536
NB_FRAME_SAMPLES = 196608
NB_SYM_BITS = 3072
NB_FRAME_BITS = 230400
NB_FIC_BITS = 9216
NB_FIB_GROUP_BITS = 2304
NB_CIF_BITS = 55296
ABI_VERSION = 4                          # DABGPU_ABI_VERSION of include/dabgpu.h
BITS_NATURAL, BITS_MSC_CLASSED = 0, 1     # dabgpu_ofdm_demod_frames_history / dabgpu_msc_decode_frames_layout


def classed_to_natural_index():
    """index array P with natural_frame_bits == classed_frame_bits[P]: FIC unchanged, inside each CIF row bit i sits at
    (i mod 16) * 3456 + i // 16 (DABGPU_BITS_MSC_CLASSED)"""
    import numpy as np
    i = np.arange(NB_CIF_BITS)
    row = (i % 16) * (NB_CIF_BITS // 16) + i // 16
    return np.concatenate([np.arange(NB_FIC_BITS)] + [NB_FIC_BITS + q * NB_CIF_BITS + row for q in range(4)])

# every symbol include/dabgpu.h declares (checked by tests/test_abi.py against the header text)
ABI_SYMBOLS = [
    "dabgpu_strerror", "dabgpu_last_error", "dabgpu_abi_version", "dabgpu_device_count",
    "dabgpu_create", "dabgpu_destroy", "dabgpu_synchronize", "dabgpu_host_pin", "dabgpu_host_unpin",
    "dabgpu_get_prs_fft_ref", "dabgpu_get_carrier_mapper", "dabgpu_get_fft_twiddles",
    "dabgpu_ofdm_demod_frames", "dabgpu_ofdm_phase_update", "dabgpu_ofdm_demod_frames_host_sync", "dabgpu_ofdm_demod_stream_frame_sync",
    "dabgpu_sync_cfg_default", "dabgpu_ofdm_sync", "dabgpu_ofdm_sync_host_sync",
    "dabgpu_viterbi_set_mapping", "dabgpu_ofdm_auto_symbols_per_block", "dabgpu_viterbi_decode_batch", "dabgpu_fic_decode_frames", "dabgpu_subchannel_plan", "dabgpu_subchannel_validate", "dabgpu_msc_decode_frames",
    "dabgpu_fic_decode_group_host_sync", "dabgpu_viterbi_decode_host_sync", "dabgpu_msc_stream_create",
    "dabgpu_msc_stream_destroy", "dabgpu_msc_stream_push_cif", "dabgpu_msc_stream_deinterleave_sync",
    "dabgpu_msc_stream_decode_sync",
    "dabgpu_iq_format_from_mode", "dabgpu_iq_format_sample_bytes", "dabgpu_wav_parse_header",
    "dabgpu_iq_convert", "dabgpu_iq_convert_host_sync", "dabgpu_ofdm_demod_frames_raw",
    "dabgpu_soft_bits_to_hard_bytes", "dabgpu_hard_bytes_to_soft_bits",
    "dabgpu_soft_bits_to_hard_bytes_host_sync", "dabgpu_hard_bytes_to_soft_bits_host_sync",
    "dabgpu_stream_cfg_default", "dabgpu_stream_bank_create", "dabgpu_stream_bank_create_mode", "dabgpu_stream_bank_destroy", "dabgpu_stream_bank_reset",
    "dabgpu_stream_bank_process", "dabgpu_stream_bank_process_raw", "dabgpu_stream_bank_status",
    "dabgpu_stream_bank_process_retained", "dabgpu_stream_bank_release",
    "dabgpu_dabplus_bank_create", "dabgpu_dabplus_bank_destroy", "dabgpu_dabplus_bank_reset", "dabgpu_dabplus_bank_process",
    "dabgpu_dabplus_process_frame_host_sync",
    "dabgpu_get_ofdm_params", "dabgpu_ofdm_demod_frames_mode", "dabgpu_ofdm_phase_update_mode",
    "dabgpu_ofdm_sync_mode", "dabgpu_ofdm_demod_stream_frame_sync_mode", "dabgpu_ofdm_sync_host_sync_mode",
    "dabgpu_stream_bank_process_ring", "dabgpu_fic_decode_ring", "dabgpu_msc_decode_ring", "dabgpu_dabplus_bank_process_masked",
    "dabgpu_ofdm_demod_frames_history", "dabgpu_msc_decode_frames_layout", "dabgpu_stream_bank_process_ring_layout",
    "dabgpu_msc_decode_ring_layout", "dabgpu_ofdm_demod_phase_frames", "dabgpu_decode_frames_layout", "dabgpu_decode_ring_layout",
    "dabgpu_frame_session_create", "dabgpu_frame_session_destroy", "dabgpu_frame_session_set_subchannels", "dabgpu_frame_session_push_frame",
    "dabgpu_frame_session_fetch_fib_group", "dabgpu_frame_session_fetch_cif",
    "dabgpu_viterbi_decode_depunctured_host_sync", "dabgpu_stream_bank_process_ring_retained",
    "dabgpu_ofdm_tune", "dabgpu_ofdm_tuned_symbols_per_block", "dabgpu_ofdm_sync_demod_frames",
    "dabgpu_multiplex_mapping",
    "dabgpu_receiver_create", "dabgpu_receiver_create_banked", "dabgpu_receiver_destroy", "dabgpu_receiver_session", "dabgpu_receiver_set_subchannels", "dabgpu_receiver_stage",
    "dabgpu_receiver_reset", "dabgpu_receiver_submit_sync", "dabgpu_receiver_wait_sync", "dabgpu_receiver_submit_frame", "dabgpu_receiver_wait_frame",
    "dabgpu_receiver_submit_demod", "dabgpu_receiver_submit_decode",
    "dabgpu_ingest_create", "dabgpu_ingest_destroy", "dabgpu_ingest_acquire", "dabgpu_ingest_submit", "dabgpu_ingest_wait", "dabgpu_ingest_consumed",
    "dabgpu_ofdm_modulate_frames", "dabgpu_ofdm_modulate_frames_host_sync",
    "dabgpu_tx_encode_plan", "dabgpu_tx_bank_create", "dabgpu_tx_bank_destroy", "dabgpu_tx_bank_reset", "dabgpu_tx_bank_encode_frames",
    "dabgpu_tx_bank_transmit_frames", "dabgpu_tx_bank_encode_frames_host_sync", "dabgpu_tx_bank_transmit_frames_host_sync",
    "dabgpu_dabplus_superframe_layout", "dabgpu_dabplus_tx_encode", "dabgpu_dabplus_tx_encode_host_sync",
    "dabgpu_packet_bank_create", "dabgpu_packet_bank_destroy", "dabgpu_packet_bank_reset", "dabgpu_packet_bank_process",
    "dabgpu_packet_bank_process_masked", "dabgpu_packet_fec_read_host_sync",
    "dabgpu_packet_tx_layout", "dabgpu_packet_tx_encode", "dabgpu_packet_tx_encode_host_sync",
    "dabgpu_channel_plan", "dabgpu_channel_freq_q64", "dabgpu_channel_freq_cycles", "dabgpu_channel_bank_create", "dabgpu_channel_bank_destroy",
    "dabgpu_channel_bank_set_params", "dabgpu_channel_bank_seek", "dabgpu_channel_bank_apply", "dabgpu_channel_bank_apply_host_sync",
    "dabgpu_channel_fading_plan", "dabgpu_channel_fading_gain_host", "dabgpu_channel_profile", "dabgpu_channel_bank_create_fading",
    "dabgpu_channel_bank_set_fading", "dabgpu_channel_plan_fading",
    "dabgpu_resample_design", "dabgpu_resample_plan", "dabgpu_resample_step_q62", "dabgpu_resample_step", "dabgpu_resample_input_needed",
    "dabgpu_resample_bank_create", "dabgpu_resample_bank_destroy", "dabgpu_resample_bank_set_params", "dabgpu_resample_bank_seek",
    "dabgpu_resample_bank_apply", "dabgpu_resample_bank_apply_host_sync",
    "dabgpu_channeliser_design", "dabgpu_channeliser_plan", "dabgpu_channeliser_freq_q64", "dabgpu_channeliser_input_needed",
    "dabgpu_channeliser_decim_for", "dabgpu_channeliser_bank_create", "dabgpu_channeliser_bank_destroy", "dabgpu_channeliser_bank_set_params",
    "dabgpu_channeliser_bank_seek", "dabgpu_channeliser_bank_split", "dabgpu_channeliser_bank_split_host_sync",
    "dabgpu_channeliser_bank_combine", "dabgpu_channeliser_bank_combine_host_sync",
    "dabgpu_tii_cfg_default", "dabgpu_tii_pattern", "dabgpu_tii_main_id", "dabgpu_tii_carriers", "dabgpu_tii_validate",
    "dabgpu_ofdm_modulate_frames_tii", "dabgpu_ofdm_modulate_frames_tii_host_sync",
    "dabgpu_tii_bank_create", "dabgpu_tii_bank_destroy", "dabgpu_tii_bank_reset", "dabgpu_tii_bank_process", "dabgpu_tii_bank_process_host_sync",
    "dabgpu_tii_bank_read",
    "dabgpu_ber_plan", "dabgpu_ber_frames_layout", "dabgpu_ber_ring_layout", "dabgpu_ber_fib_group_host_sync", "dabgpu_ber_codeword_host_sync",
    "dabgpu_soft_cfg_default", "dabgpu_soft_scale_host", "dabgpu_ofdm_demod_frames_soft", "dabgpu_ofdm_sync_demod_frames_soft",
    "dabgpu_receiver_set_soft", "dabgpu_stream_bank_set_soft", "dabgpu_stream_bank_get_soft",
    "dabgpu_stream_bank_set_products", "dabgpu_stream_bank_get_products",
    "dabgpu_diversity_plan", "dabgpu_diversity_combine_frames", "dabgpu_diversity_combine_host_sync", "dabgpu_diversity_scale_host",
    "dabgpu_ofdm_sync_demod_frames_branch", "dabgpu_receiver_frame_soft_scale",
    "dabgpu_noise_plan", "dabgpu_noise_estimate_frames", "dabgpu_noise_estimate_host_sync", "dabgpu_noise_unbias", "dabgpu_noise_floor_host",
    "dabgpu_noise_profile_plan", "dabgpu_noise_profile_frames", "dabgpu_noise_profile_host_sync", "dabgpu_noise_profile_bands_host",
    "dabgpu_noise_profile_exclude_tii", "dabgpu_diversity_plan_banded", "dabgpu_diversity_combine_frames_banded",
    "dabgpu_diversity_combine_banded_host_sync", "dabgpu_diversity_band_mean_host",
    "dabgpu_dd_profile_plan", "dabgpu_dd_profile_frames", "dabgpu_dd_profile_host_sync", "dabgpu_dd_profile_carriers_host",
    "dabgpu_sym_profile_plan", "dabgpu_sym_profile_frames", "dabgpu_sym_profile_host_sync", "dabgpu_sym_profile_rows_host",
    "dabgpu_diversity_plan_symbols", "dabgpu_diversity_combine_frames_symbols", "dabgpu_diversity_combine_symbols_host_sync",
    "dabgpu_clock_estimate_plan", "dabgpu_clock_derotate_plan", "dabgpu_clock_estimate_frames", "dabgpu_clock_derotate_frames",
    "dabgpu_clock_derotate_frames_split", "dabgpu_clock_track_host_sync", "dabgpu_clock_estimate_host", "dabgpu_clock_derotate_host",
    "dabgpu_clock_slope_q64", "dabgpu_clock_ppm",
    "dabgpu_interferer_design", "dabgpu_interferer_plan", "dabgpu_interferer_bank_create", "dabgpu_interferer_bank_destroy",
    "dabgpu_interferer_bank_set_params", "dabgpu_interferer_bank_seek", "dabgpu_interferer_bank_apply", "dabgpu_interferer_bank_apply_host_sync",
    "dabgpu_blanker_defaults", "dabgpu_blanker_mask_words", "dabgpu_blanker_plan", "dabgpu_blanker_input_needed", "dabgpu_blanker_bank_create",
    "dabgpu_blanker_bank_destroy", "dabgpu_blanker_bank_set_params", "dabgpu_blanker_bank_seek", "dabgpu_blanker_bank_apply",
    "dabgpu_blanker_bank_apply_host_sync",
    "dabgpu_iqbal_defaults", "dabgpu_iqbal_plan", "dabgpu_iqbal_impairment", "dabgpu_iqbal_forget", "dabgpu_iqbal_solve_host",
    "dabgpu_iqbal_bank_create", "dabgpu_iqbal_bank_destroy", "dabgpu_iqbal_bank_set_params", "dabgpu_iqbal_bank_seek", "dabgpu_iqbal_bank_reset",
    "dabgpu_iqbal_bank_apply", "dabgpu_iqbal_bank_apply_host_sync", "dabgpu_iqbal_bank_read_state_host_sync",
    "dabgpu_iqbal_bank_read_moments_host_sync",
]
NOISE_PROFILE_BANDS, NOISE_PROFILE_BAND_CARRIERS, NOISE_PROFILE_EXCLUDE_WORDS = 128, 12, 48      # noise profile (include/dabgpu.h)
SYM_PROFILE_SYMBOLS = 75                  # symbol noise profile: product rows of a mode I frame
CLOCK_LAG = 32                            # sampling-clock tracker (include/dabgpu.h): carriers between the two products of a lag product
CLOCK_MAX_SLOPE = 22986372498099012       # the slope word of 1000 ppm
SOFT_NORMALISED, SOFT_CSI = 0, 1          # dabgpu_soft_cfg.policy
DIVERSITY_MAX_BRANCHES = 8                # receive diversity (include/dabgpu.h)
NOISE_RECORD_DTYPE = [("noise_power", "<f4"), ("signal_power", "<f4"), ("weight", "<f4"), ("snr", "<f4"), ("valid", "<u4")]   # dabgpu_noise_record

# channel model (include/dabgpu.h)
CHANNEL_MAX_TAPS = 8
CHANNEL_MAX_DELAY = 2047
CHANNEL_BLOCK = 1024

# resampler (include/dabgpu.h)
RESAMPLE_PHASES = 256
RESAMPLE_TAPS = 48
RESAMPLE_BLOCK = 1024
RESAMPLE_DEFAULT_PASSBAND = 0.375

# channeliser (include/dabgpu.h)
CHANNELISER_TAPS_PER_PHASE = 72
CHANNELISER_MAX_DECIM = 8
CHANNELISER_MAX_CHANNELS = 8
CHANNELISER_SPLIT_TILE = 512
CHANNELISER_COMBINE_ROWS = 128
CHANNELISER_DEFAULT_PASSBAND = 0.375
CHANNELISER_DEFAULT_STOPBAND = 0.4609375
CHANNELISER_MAX_POSITION = 1 << 58
CHANNELISER_MAX_START = 1 << 61

# TII (include/dabgpu.h)
TII_MAX_TX = 4
TII_NB_MAIN = 70
TII_COMBS = 24
TII_GROUPS = 8
TII_DEFAULT_THRESHOLD = 2.16
TII_SETTLE_FRAMES = 1          # frames after an acquisition whose sync record is still up to half a carrier spacing off (dabgpu.h, "TII")
TII_TX_DTYPE = [("main_id", "u1"), ("sub_id", "u1"), ("pad", "<u2"), ("amp", "<f4")]                 # dabgpu_tii_tx
TII_RECORD_DTYPE = [("sub_id", "<i4"), ("main_id", "<i4"), ("mask", "<u4"), ("strength", "<f4")]   # dabgpu_tii_record

# OFDM transmitter payload layouts (include/dabgpu.h)
TX_PAYLOAD_REFERENCE = 0
TX_PAYLOAD_FRAME_BITS = 1

IQ_FORMATS = ["raw_u8", "raw_s8", "raw_s16l", "raw_s16b", "raw_u16l", "raw_u16b", "raw_s32l", "raw_s32b", "raw_u32l", "raw_u32b",
              "raw_f32l", "raw_f32b", "raw_f64l", "raw_f64b",
              "wav_pcm8", "wav_pcm16", "wav_pcm24", "wav_pcm32", "wav_f32", "wav_f64", "wav_alaw", "wav_mulaw"]


class WavHeader(C.Structure):
    """dabgpu_wav_header"""
    _fields_ = [("iq_format", C.c_int32), ("audio_format", C.c_uint16), ("total_channels", C.c_uint16),
                ("samples_per_second", C.c_uint32), ("average_bytes_per_second", C.c_uint32),
                ("data_block_align_bytes", C.c_uint16), ("bits_per_sample", C.c_uint16),
                ("data_chunk_size", C.c_uint32), ("data_chunk_offset", C.c_uint64)]


class Codeword(C.Structure):
    """dabgpu_codeword (include/dabgpu.h)"""
    _fields_ = [("d_src", C.c_uint64), ("d_out", C.c_uint64), ("n_steps", C.c_uint32),
                ("seg_pi", C.c_uint32 * 4), ("seg_steps", C.c_uint32 * 4), ("start_state", C.c_uint32),
                ("n_crc_blocks", C.c_uint32), ("n_slots", C.c_uint32), ("newest_slot", C.c_uint32),
                ("cifs_per_frame", C.c_uint32), ("frame_stride", C.c_uint32), ("cif_stride", C.c_uint32),
                ("end_state", C.c_uint32), ("flags", C.c_uint32)]


class CodewordResult(C.Structure):
    """dabgpu_codeword_result"""
    _fields_ = [("path_error", C.c_uint64), ("crc_ok_mask", C.c_uint32), ("n_out_bytes", C.c_uint32)]


class SubChannel(C.Structure):
    """dabgpu_subchannel"""
    _fields_ = [("start_address", C.c_int), ("length", C.c_int), ("is_uep", C.c_int),
                ("uep_prot_index", C.c_int), ("eep_prot_level", C.c_int), ("eep_type", C.c_int)]


class TxSubPlan(C.Structure):
    """dabgpu_tx_sub_plan"""
    _fields_ = [("start_address", C.c_uint32), ("length", C.c_uint32), ("in_offset", C.c_uint32), ("in_bytes", C.c_uint32),
                ("seg_pi", C.c_uint32 * 4), ("seg_blocks", C.c_uint32 * 4), ("n_words", C.c_uint32), ("kept_bits", C.c_uint32),
                ("sched_offset", C.c_uint32), ("ring_offset", C.c_uint32), ("ring_row_dwords", C.c_uint32)]


class BerGeometry(C.Structure):
    """dabgpu_ber_geometry"""
    _fields_ = [("n_sub", C.c_uint32), ("codewords_per_ensemble", C.c_uint32), ("cif_bytes", C.c_uint32), ("n_sched", C.c_uint32),
                ("sched_offset", C.c_uint32 * 65), ("max_kept_bits", C.c_uint32), ("lds_bytes", C.c_uint32), ("waves_per_block", C.c_uint32),
                ("block_threads", C.c_uint32), ("grid", C.c_uint32)]


class DiversityBranch(C.Structure):
    """dabgpu_diversity_branch: device addresses of one branch's products, scales, weights (0: weight 1) and sync records (0: none)"""
    _fields_ = [("d_dqpsk", C.c_void_p), ("d_scale", C.c_void_p), ("d_weight", C.c_void_p), ("d_sync", C.c_void_p)]


class DiversityGeometry(C.Structure):
    """dabgpu_diversity_geometry"""
    _fields_ = [("symbols_per_block", C.c_uint32), ("runs_per_frame", C.c_uint32), ("grid", C.c_uint32), ("threads", C.c_uint32),
                ("lds_bytes", C.c_uint32)]


class NoiseGeometry(C.Structure):
    """dabgpu_noise_geometry"""
    _fields_ = [("grid", C.c_uint32), ("threads", C.c_uint32), ("lds_bytes", C.c_uint32)]


class ChannelStream(C.Structure):
    """dabgpu_channel_stream"""
    _fields_ = [("freq_q64", C.c_uint64), ("phase0_q64", C.c_uint64), ("start", C.c_int64), ("seed", C.c_uint64),
                ("gain", C.c_float), ("noise_sigma", C.c_float), ("n_taps", C.c_int32), ("tap_delay", C.c_int32 * 8),
                ("tap_re", C.c_float * 8), ("tap_im", C.c_float * 8), ("reserved", C.c_int32)]


class ChannelFadingTap(C.Structure):
    """dabgpu_channel_fading_tap"""
    _fields_ = [("freq_q64", C.c_uint64 * 17), ("phase_q64", C.c_uint64 * 17), ("amp_diffuse", C.c_float), ("amp_los", C.c_float)]


class ChannelFadingStream(C.Structure):
    """dabgpu_channel_fading_stream"""
    _fields_ = [("kind", C.c_int32 * 8), ("tap", ChannelFadingTap * 8)]


class ChannelFadingSpec(C.Structure):
    """dabgpu_channel_fading_spec"""
    _fields_ = [("doppler_cycles", C.c_double), ("seed", C.c_uint64), ("kind", C.c_int32 * 8), ("rice_k", C.c_float * 8), ("los_cos", C.c_float * 8)]


TAP_STATIC, TAP_FADING = 0, 1
FADING_OSC, FADING_GRID, FADING_MAX_DOPPLER_CYCLES = 17, 64, 2.0 ** -11


class ChannelGeometry(C.Structure):
    """dabgpu_channel_geometry"""
    _fields_ = [("halo", C.c_uint32), ("block_samples", C.c_uint32), ("lds_bytes", C.c_uint32), ("staged", C.c_uint32)]


# interferer (include/dabgpu.h)
INTERFERER_MAX, INTERFERER_MAX_SHAPES, INTERFERER_TAPS, INTERFERER_MAX_INTERP, INTERFERER_BLOCK = 4, 4, 16, 64, 1024
INTERFERER_TRANSITION, INTERFERER_MIN_WIDTH, INTERFERER_MAX_POSITION = 0.25, 2.0 ** -8, 1 << 62
INTERFERER_OFF, INTERFERER_TONE, INTERFERER_BAND = 0, 1, 2


class InterfererSource(C.Structure):
    """dabgpu_interferer_source"""
    _fields_ = [("kind", C.c_int32), ("shape", C.c_int32), ("amp", C.c_float), ("reserved", C.c_int32), ("freq_q64", C.c_uint64),
                ("phase0_q64", C.c_uint64), ("gate_period", C.c_uint64), ("gate_on", C.c_uint64), ("gate_offset", C.c_int64)]


class InterfererStream(C.Structure):
    """dabgpu_interferer_stream"""
    _fields_ = [("seed", C.c_uint64), ("n_sources", C.c_int32), ("reserved", C.c_int32), ("source", InterfererSource * INTERFERER_MAX)]


class InterfererShape(C.Structure):
    """dabgpu_interferer_shape: the design record (its own figures) and the table of 16 x interp taps"""
    _fields_ = [("interp", C.c_int32), ("reserved", C.c_int32), ("width_cycles", C.c_double), ("cutoff_cycles", C.c_double), ("beta", C.c_double),
                ("width_3db_cycles", C.c_double), ("inband_share", C.c_double), ("stopband_level", C.c_double), ("phase_ripple", C.c_double),
                ("taps", C.c_float * (INTERFERER_TAPS * INTERFERER_MAX_INTERP))]


class InterfererGeometry(C.Structure):
    """dabgpu_interferer_geometry"""
    _fields_ = [("block_samples", C.c_uint32), ("band_slots", C.c_uint32), ("slot_bytes", C.c_uint32), ("lds_bytes", C.c_uint32)]


# impulse blanker (include/dabgpu.h)
BLANKER_POWER_BLOCK, BLANKER_BLOCK, BLANKER_MAX_WINDOW, BLANKER_MAX_GAP, BLANKER_MAX_GUARD, BLANKER_MAX_POSITION = 32, 1024, 32, 32, 4, 1 << 62


class BlankerStream(C.Structure):
    """dabgpu_blanker_stream"""
    _fields_ = [("start", C.c_int64), ("threshold", C.c_float), ("gap", C.c_int32), ("window", C.c_int32), ("guard", C.c_int32),
                ("enabled", C.c_int32), ("reserved", C.c_int32)]


class BlankerGeometry(C.Structure):
    """dabgpu_blanker_geometry"""
    _fields_ = [("reach_blocks", C.c_uint32), ("block_samples", C.c_uint32), ("lds_bytes", C.c_uint32), ("reserved", C.c_uint32)]


# IQ balance (include/dabgpu.h)
IQBAL_TILE, IQBAL_OFF, IQBAL_FIXED, IQBAL_TRACK, IQBAL_MEASURE, IQBAL_APPLY, IQBAL_MAX_POSITION = 1024, 0, 1, 2, 1, 2, 1 << 62


class IqBalanceStream(C.Structure):
    """dabgpu_iqbal_stream"""
    _fields_ = [("mode", C.c_int32), ("reserved", C.c_int32), ("a_re", C.c_float), ("a_im", C.c_float), ("b_re", C.c_float), ("b_im", C.c_float),
                ("c_re", C.c_float), ("c_im", C.c_float), ("forget", C.c_float), ("min_weight", C.c_float)]


class IqBalanceGeometry(C.Structure):
    """dabgpu_iqbal_geometry"""
    _fields_ = [("tile_samples", C.c_uint32), ("tiles_per_call", C.c_uint32), ("scratch_bytes", C.c_uint64)]


# dabgpu_iqbal_record
IQBAL_RECORD_DTYPE = [("N", "<f4"), ("S", "<f4", (5,)), ("d_re", "<f4"), ("d_im", "<f4"), ("P", "<f4"), ("C_re", "<f4"), ("C_im", "<f4"),
                      ("w_re", "<f4"), ("w_im", "<f4"), ("a_re", "<f4"), ("a_im", "<f4"), ("b_re", "<f4"), ("b_im", "<f4"), ("c_re", "<f4"),
                      ("c_im", "<f4"), ("valid", "<u4"), ("tiles_used", "<u8"), ("tiles_skipped", "<u8"), ("calls_refused", "<u4"),
                      ("reserved", "<u4")]


class ResampleStream(C.Structure):
    """dabgpu_resample_stream"""
    _fields_ = [("step_q62", C.c_uint64), ("offset_samples", C.c_int64), ("offset_frac_q62", C.c_uint64), ("gain", C.c_float), ("reserved", C.c_int32)]


class ResampleFilter(C.Structure):
    """dabgpu_resample_filter: the design record (its error figures) and the (L + 1) x taps table"""
    _fields_ = [("max_step", C.c_double), ("passband_cycles", C.c_double), ("beta", C.c_double),
                ("passband_error", C.c_double), ("alias_leakage", C.c_double), ("error", C.c_double),
                ("table", C.c_float * ((RESAMPLE_PHASES + 1) * RESAMPLE_TAPS))]


class ResampleGeometry(C.Structure):
    """dabgpu_resample_geometry"""
    _fields_ = [("block_samples", C.c_uint32), ("window_samples", C.c_uint32), ("table_rows", C.c_uint32), ("lds_bytes", C.c_uint32)]


class ChanneliserChannel(C.Structure):
    """dabgpu_channeliser_channel"""
    _fields_ = [("freq_q64", C.c_uint64), ("phase0_q64", C.c_uint64), ("gain", C.c_float), ("stream", C.c_uint32)]


class ChanneliserFilter(C.Structure):
    """dabgpu_channeliser_filter: the design record (its error figures) and the table of 72 x decim taps"""
    _fields_ = [("decim", C.c_int32), ("taps", C.c_int32), ("passband_cycles", C.c_double), ("stopband_cycles", C.c_double),
                ("cutoff_cycles", C.c_double), ("beta", C.c_double), ("passband_error", C.c_double), ("stopband_level", C.c_double),
                ("error", C.c_double), ("table", C.c_float * (CHANNELISER_TAPS_PER_PHASE * CHANNELISER_MAX_DECIM))]


class ChanneliserGeometry(C.Structure):
    """dabgpu_channeliser_geometry"""
    _fields_ = [(name, C.c_uint32) for name in ("decim", "taps", "split_tile", "split_window", "split_lds_bytes", "combine_tile", "combine_window",
                                                "combine_lds_bytes")]


class SyncCfg(C.Structure):
    """dabgpu_sync_cfg"""
    _fields_ = [("fine_freq_update_beta", C.c_float), ("is_coarse_freq_correction", C.c_int),
                ("max_coarse_freq_correction_norm", C.c_float), ("coarse_freq_slow_beta", C.c_float),
                ("impulse_peak_threshold_db", C.c_float), ("impulse_peak_distance_probability", C.c_float)]


class SoftCfg(C.Structure):
    """dabgpu_soft_cfg: the soft-decision policy of the mode I demodulator (SOFT_NORMALISED / SOFT_CSI) and the level of SOFT_CSI"""
    _fields_ = [("policy", C.c_int), ("level", C.c_float)]

    def __init__(self, policy=SOFT_NORMALISED, level=64.0):
        super().__init__(int(policy), float(level))


class SyncState(C.Structure):
    """dabgpu_sync_state"""
    _fields_ = [("freq_coarse", C.c_float), ("freq_fine", C.c_float), ("is_found_coarse", C.c_int),
                ("fine_time_offset", C.c_int), ("sync_valid", C.c_int), ("reserved", C.c_int)]


class StreamCfg(C.Structure):
    """dabgpu_stream_cfg"""
    _fields_ = [("signal_l1_update_beta", C.c_float), ("signal_l1_nb_samples", C.c_int), ("signal_l1_nb_decimate", C.c_int),
                ("thresh_null_start", C.c_float), ("thresh_null_end", C.c_float), ("sync", SyncCfg)]


STREAM_STATUS_DTYPE = [("state", "<i4"), ("signal_l1_average", "<f4"), ("freq_coarse", "<f4"), ("freq_fine", "<f4"),
                       ("is_found_coarse", "<i4"), ("fine_time_offset", "<i4"), ("total_frames_read", "<i4"),
                       ("total_frames_desync", "<i4")]
SUPERFRAME_RESULT_DTYPE = [("rs_failed_index", "<i4"), ("rs_corrected", "<i4"), ("firecode_ok", "<i4"), ("header_valid", "<i4"),
                           ("descriptor", "<i4"), ("num_aus", "<i4"), ("au_start", "<i4", (8,)), ("au_walk_stopped_at", "<i4"),
                           ("au_crc_ok_mask", "<u4"), ("frame_index", "<i4"), ("firecode_rx_calc", "<u4"),
                           ("au_crc_calc", "<u2", (6,)), ("reserved", "<u2", (2,))]
# MSC packet mode (include/dabgpu.h): dabgpu_packet_record, dabgpu_packet_fec_frame, dabgpu_packet_tx_entry
PACKET_RECORD_DTYPE = [("offset", "<u4"), ("length", "<u2"), ("address", "<u2"), ("continuity_index", "u1"), ("first_last", "u1"), ("command", "u1"),
                       ("useful_length", "u1"), ("is_corrected", "u1"), ("crc_ok", "u1"), ("reserved", "u1", (2,))]
PACKET_FEC_FRAME_DTYPE = [("frame_index", "<i4"), ("first_record", "<i4"), ("rs_count", "i1", (12,))]
PACKET_TX_ENTRY_DTYPE = [("group", "<i4"), ("offset", "<u4"), ("position", "<u4"), ("length", "u1"), ("useful", "u1"), ("flags", "u1"),
                         ("continuity_index", "u1")]
PACKET_RING_BYTES = 2472
PACKET_APP_BYTES = 2256
PACKET_MAX_FRAME_PACKETS = 94
SYNC_STATE_DTYPE = [("freq_coarse", "<f4"), ("freq_fine", "<f4"), ("is_found_coarse", "<i4"),
                    ("fine_time_offset", "<i4"), ("sync_valid", "<i4"), ("reserved", "<i4")]
RESULT_DTYPE = [("path_error", "<u8"), ("crc_ok_mask", "<u4"), ("n_out_bytes", "<u4")]
BER_RESULT_DTYPE = [("n_bits", "<u4"), ("n_errors", "<u4"), ("error_weight", "<u4"), ("total_weight", "<u4")]      # dabgpu_ber_result


class DabGpuError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libdabgpu.so; loud failure when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DabGpuError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C dab-radio_amd/csrc` (no CPU fallback exists)")
        # torch bundles its own libamdhip64.so.7; when torch is in the process it must be the one HIP runtime
        # (same SONAME as /opt/rocm's): import it first so libdabgpu.so binds to the already-loaded copy and
        # tensors, streams and our kernels share one runtime.  Stand-alone C/C++ users link /opt/rocm's.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        if L.dabgpu_abi_version() != ABI_VERSION:
            raise DabGpuError(f"{LIB_PATH} implements ABI version {L.dabgpu_abi_version()}, this binding was written for {ABI_VERSION}: rebuild it")
        L.dabgpu_strerror.restype = C.c_char_p
        L.dabgpu_strerror.argtypes = [C.c_int]
        L.dabgpu_last_error.restype = C.c_char_p
        L.dabgpu_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
        L.dabgpu_destroy.argtypes = [C.c_void_p]
        L.dabgpu_synchronize.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_get_prs_fft_ref.argtypes = [C.c_int, C.c_void_p]
        L.dabgpu_get_carrier_mapper.argtypes = [C.c_int, C.c_void_p]
        L.dabgpu_get_fft_twiddles.argtypes = [C.c_void_p]
        L.dabgpu_ofdm_demod_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        L.dabgpu_ofdm_demod_frames_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        L.dabgpu_ofdm_demod_frames_history.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_int, C.c_size_t, C.c_int, C.c_void_p]
        L.dabgpu_ofdm_demod_phase_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_int, C.c_size_t, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_msc_decode_frames_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                                      C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabgpu_decode_frames_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabgpu_decode_ring_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabgpu_ofdm_demod_stream_frame_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float,
                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_ofdm_phase_update.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
        L.dabgpu_ofdm_demod_frames_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_sync_cfg_default.argtypes = [C.c_void_p]
        L.dabgpu_ofdm_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
        L.dabgpu_ofdm_sync_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_viterbi_set_mapping.argtypes = [C.c_void_p, C.c_int]
        L.dabgpu_ofdm_auto_symbols_per_block.argtypes = [C.c_void_p, C.c_size_t]
        L.dabgpu_ofdm_tune.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.dabgpu_ofdm_tuned_symbols_per_block.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int]
        L.dabgpu_ofdm_sync_demod_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
        L.dabgpu_soft_cfg_default.argtypes = [C.c_void_p]
        L.dabgpu_soft_cfg_default.restype = None
        L.dabgpu_soft_scale_host.argtypes = [C.c_void_p, C.c_float]
        L.dabgpu_soft_scale_host.restype = C.c_float
        L.dabgpu_ofdm_demod_frames_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_ofdm_sync_demod_frames_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p]
        L.dabgpu_receiver_set_soft.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_receiver_frame_soft_scale.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.dabgpu_diversity_plan.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        L.dabgpu_diversity_combine_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_diversity_combine_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                         C.c_void_p, C.c_void_p]
        L.dabgpu_diversity_scale_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_diversity_scale_host.restype = C.c_float
        L.dabgpu_noise_plan.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t] + [C.c_void_p] * 9
        L.dabgpu_noise_estimate_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t] + [C.c_void_p] * 9
        L.dabgpu_noise_estimate_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int, C.c_void_p]
        L.dabgpu_noise_unbias.argtypes = []
        L.dabgpu_noise_unbias.restype = C.c_float
        L.dabgpu_noise_floor_host.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
        L.dabgpu_noise_profile_plan.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t] + [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 6
        L.dabgpu_noise_profile_frames.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t] + [C.c_void_p] * 4 + [C.c_float] +
                                                  [C.c_void_p] * 6)
        L.dabgpu_noise_profile_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                                     C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_noise_profile_bands_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_noise_profile_exclude_tii.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_dd_profile_plan.argtypes = [C.c_int, C.c_void_p, C.c_size_t] + [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 7
        L.dabgpu_dd_profile_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 7
        L.dabgpu_dd_profile_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 5
        L.dabgpu_dd_profile_carriers_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_diversity_plan_banded.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.dabgpu_diversity_combine_frames_banded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_diversity_combine_banded_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_diversity_band_mean_host.argtypes = [C.c_void_p]
        L.dabgpu_diversity_band_mean_host.restype = C.c_float
        L.dabgpu_sym_profile_plan.argtypes = [C.c_int, C.c_void_p, C.c_size_t] + [C.c_void_p] * 6
        L.dabgpu_sym_profile_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 6
        L.dabgpu_sym_profile_host_sync.argtypes = [C.c_void_p] * 6
        L.dabgpu_sym_profile_rows_host.argtypes = [C.c_void_p] * 4
        L.dabgpu_clock_estimate_plan.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 5
        L.dabgpu_clock_derotate_plan.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_clock_estimate_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 5
        L.dabgpu_clock_derotate_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_clock_derotate_frames_split.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_clock_track_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.dabgpu_clock_estimate_host.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]
        L.dabgpu_clock_derotate_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.dabgpu_clock_slope_q64.restype = C.c_int64
        L.dabgpu_clock_slope_q64.argtypes = [C.c_double]
        L.dabgpu_clock_ppm.restype = C.c_double
        L.dabgpu_clock_ppm.argtypes = [C.c_int64]
        L.dabgpu_diversity_plan_symbols.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]
        L.dabgpu_diversity_combine_frames_symbols.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_diversity_combine_symbols_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_ofdm_sync_demod_frames_branch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_void_p]
        L.dabgpu_viterbi_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
        L.dabgpu_fic_decode_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_void_p]
        L.dabgpu_subchannel_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_msc_decode_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_iq_format_from_mode.argtypes = [C.c_char_p]
        L.dabgpu_iq_format_sample_bytes.restype = C.c_size_t
        L.dabgpu_iq_format_sample_bytes.argtypes = [C.c_int]
        L.dabgpu_wav_parse_header.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.dabgpu_iq_convert.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dabgpu_iq_convert_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        L.dabgpu_soft_bits_to_hard_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dabgpu_hard_bytes_to_soft_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dabgpu_soft_bits_to_hard_bytes_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dabgpu_hard_bytes_to_soft_bits_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dabgpu_stream_cfg_default.argtypes = [C.c_void_p]
        L.dabgpu_stream_bank_create.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]
        L.dabgpu_stream_bank_create_mode.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]
        L.dabgpu_stream_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_stream_bank_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_stream_bank_process.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                 C.c_void_p, C.c_void_p]
        L.dabgpu_stream_bank_process_retained.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                          C.c_void_p, C.c_void_p]
        L.dabgpu_stream_bank_release.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        L.dabgpu_stream_bank_process_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                     C.c_void_p, C.c_void_p]
        L.dabgpu_stream_bank_process_ring.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_void_p]
        L.dabgpu_stream_bank_process_ring_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int,
                                                             C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_stream_bank_process_ring_retained.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                                               C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_msc_decode_ring_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                    C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabgpu_fic_decode_ring.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p]
        L.dabgpu_msc_decode_ring.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_dabplus_bank_process_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                                         C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_stream_bank_status.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_stream_bank_set_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.dabgpu_stream_bank_get_soft.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_stream_bank_set_products.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.dabgpu_stream_bank_get_products.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_dabplus_bank_create.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.dabgpu_dabplus_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_dabplus_bank_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_dabplus_bank_process.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                                  C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.dabgpu_dabplus_process_frame_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_void_p, C.c_void_p]
        L.dabgpu_ofdm_sync_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
        L.dabgpu_ofdm_sync_host_sync_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_get_ofdm_params.argtypes = [C.c_int, C.c_void_p]
        L.dabgpu_ofdm_demod_frames_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_ofdm_phase_update_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]
        L.dabgpu_ingest_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
        L.dabgpu_ingest_destroy.argtypes = [C.c_void_p]
        L.dabgpu_ingest_acquire.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.dabgpu_ingest_submit.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.dabgpu_ingest_wait.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_ingest_consumed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_ofdm_modulate_frames.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_float,
                                                  C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_ofdm_modulate_frames_host_sync.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_float,
                                                            C.c_void_p, C.c_int]
        L.dabgpu_tx_encode_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dabgpu_tx_bank_create.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.dabgpu_tx_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_tx_bank_destroy.restype = None
        L.dabgpu_tx_bank_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_tx_bank_encode_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dabgpu_tx_bank_transmit_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_tx_bank_encode_frames_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dabgpu_tx_bank_transmit_frames_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_int]
        L.dabgpu_dabplus_superframe_layout.argtypes = [C.c_uint32, C.c_uint8, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_dabplus_tx_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dabgpu_dabplus_tx_encode_host_sync.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                         C.c_void_p]
        L.dabgpu_packet_bank_create.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.dabgpu_packet_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_packet_bank_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_packet_bank_process.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                                 C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.dabgpu_packet_bank_process_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                                        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_packet_fec_read_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                       C.c_void_p]
        L.dabgpu_packet_tx_layout.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p,
                                              C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_packet_tx_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dabgpu_packet_tx_encode_host_sync.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                        C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        L.dabgpu_channel_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.dabgpu_channel_freq_q64.argtypes = [C.c_double]
        L.dabgpu_channel_freq_q64.restype = C.c_uint64
        L.dabgpu_channel_freq_cycles.argtypes = [C.c_uint64]
        L.dabgpu_channel_freq_cycles.restype = C.c_double
        L.dabgpu_channel_bank_create.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]
        L.dabgpu_channel_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_channel_bank_destroy.restype = None
        L.dabgpu_channel_bank_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_channel_bank_seek.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.dabgpu_channel_bank_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t,
                                                C.c_float, C.c_void_p]
        L.dabgpu_channel_plan_fading.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.dabgpu_channel_fading_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dabgpu_channel_fading_gain_host.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_size_t, C.c_void_p]
        L.dabgpu_channel_profile.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
        L.dabgpu_channel_bank_create_fading.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.dabgpu_channel_bank_set_fading.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_resample_design.argtypes = [C.c_double, C.c_double, C.c_void_p]
        L.dabgpu_resample_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dabgpu_resample_step_q62.argtypes = [C.c_double, C.c_double, C.c_double]
        L.dabgpu_resample_step_q62.restype = C.c_uint64
        L.dabgpu_resample_step.argtypes = [C.c_uint64]
        L.dabgpu_resample_step.restype = C.c_double
        L.dabgpu_resample_input_needed.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
        L.dabgpu_channeliser_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_void_p]
        L.dabgpu_channeliser_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p]
        L.dabgpu_channeliser_freq_q64.argtypes = [C.c_double, C.c_double]
        L.dabgpu_channeliser_freq_q64.restype = C.c_uint64
        L.dabgpu_channeliser_input_needed.argtypes = [C.c_int, C.c_uint64, C.c_int64, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
        L.dabgpu_channeliser_decim_for.argtypes = [C.c_double]
        L.dabgpu_channeliser_bank_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)]
        L.dabgpu_channeliser_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_channeliser_bank_destroy.restype = None
        L.dabgpu_channeliser_bank_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_void_p]
        L.dabgpu_channeliser_bank_seek.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.dabgpu_channeliser_bank_split.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dabgpu_channeliser_bank_split_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t]
        L.dabgpu_channeliser_bank_combine.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t,
                                                      C.c_float, C.c_void_p]
        L.dabgpu_channeliser_bank_combine_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_int,
                                                                C.c_size_t, C.c_float]
        L.dabgpu_resample_bank_create.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.dabgpu_resample_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_resample_bank_destroy.restype = None
        L.dabgpu_resample_bank_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_resample_bank_seek.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.dabgpu_resample_bank_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t,
                                                 C.c_float, C.c_void_p]
        L.dabgpu_resample_bank_apply_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_int,
                                                           C.c_size_t, C.c_float]
        L.dabgpu_channel_bank_apply_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_int,
                                                          C.c_size_t, C.c_float]
        L.dabgpu_tii_cfg_default.argtypes = [C.c_void_p]
        L.dabgpu_tii_cfg_default.restype = None
        L.dabgpu_tii_pattern.argtypes = [C.c_int]
        L.dabgpu_tii_main_id.argtypes = [C.c_uint32]
        L.dabgpu_tii_carriers.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.dabgpu_tii_validate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.dabgpu_ofdm_modulate_frames_tii.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_float,
                                                      C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_ofdm_modulate_frames_tii_host_sync.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_float,
                                                                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.dabgpu_tii_bank_create.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]
        L.dabgpu_tii_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_tii_bank_destroy.restype = None
        L.dabgpu_tii_bank_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_tii_bank_process.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
        L.dabgpu_tii_bank_process_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int, C.c_int, C.c_void_p,
                                                        C.c_void_p]
        L.dabgpu_tii_bank_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_ber_plan.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
        L.dabgpu_ber_frames_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_ber_ring_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_ber_fib_group_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_ber_codeword_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_interferer_design.argtypes = [C.c_double, C.c_void_p]
        L.dabgpu_interferer_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        L.dabgpu_interferer_bank_create.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.dabgpu_interferer_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_interferer_bank_destroy.restype = None
        L.dabgpu_interferer_bank_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_interferer_bank_seek.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.dabgpu_interferer_bank_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_void_p]
        L.dabgpu_interferer_bank_apply_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t, C.c_float]
        L.dabgpu_blanker_defaults.argtypes, L.dabgpu_blanker_defaults.restype = [], BlankerStream
        L.dabgpu_blanker_mask_words.argtypes, L.dabgpu_blanker_mask_words.restype = [C.c_size_t], C.c_size_t
        L.dabgpu_blanker_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.dabgpu_blanker_input_needed.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
        L.dabgpu_blanker_bank_create.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]
        L.dabgpu_blanker_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_blanker_bank_destroy.restype = None
        L.dabgpu_blanker_bank_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_blanker_bank_seek.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.dabgpu_blanker_bank_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                C.c_void_p]
        L.dabgpu_blanker_bank_apply_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                          C.c_size_t]
        L.dabgpu_iqbal_defaults.argtypes, L.dabgpu_iqbal_defaults.restype = [], IqBalanceStream
        L.dabgpu_iqbal_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
        L.dabgpu_iqbal_impairment.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]
        L.dabgpu_iqbal_forget.argtypes, L.dabgpu_iqbal_forget.restype = [C.c_double], C.c_float
        L.dabgpu_iqbal_solve_host.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_iqbal_bank_create.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.dabgpu_iqbal_bank_destroy.argtypes = [C.c_void_p]
        L.dabgpu_iqbal_bank_destroy.restype = None
        L.dabgpu_iqbal_bank_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dabgpu_iqbal_bank_seek.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.dabgpu_iqbal_bank_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_iqbal_bank_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_uint32,
                                              C.c_void_p]
        L.dabgpu_iqbal_bank_apply_host_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t, C.c_float,
                                                        C.c_uint32]
        L.dabgpu_iqbal_bank_read_state_host_sync.argtypes = [C.c_void_p, C.c_void_p]
        L.dabgpu_iqbal_bank_read_moments_host_sync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        _lib = L
    return _lib


def check(status, what=""):
    if status != 0:
        L = lib()
        raise DabGpuError(f"{what}: {L.dabgpu_strerror(status).decode()} -- {L.dabgpu_last_error().decode()}")


def _ptr(x):
    """device/host pointer of a torch tensor, numpy array, int or None"""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    if hasattr(x, "ctypes"):
        return C.c_void_p(x.ctypes.data)
    raise TypeError(f"cannot take a pointer of {type(x)}")


def device_count():
    return lib().dabgpu_device_count()


def host_tables():
    """(prs_fft_ref complex64[2048], carrier_mapper int32[1536], twiddles complex64[2048]) from the product's host code"""
    import numpy as np
    prs = np.zeros(NB_FFT, dtype=np.complex64)
    mapper = np.zeros(NB_CARRIERS, dtype=np.int32)
    tw = np.zeros(NB_FFT, dtype=np.complex64)
    check(lib().dabgpu_get_prs_fft_ref(1, _ptr(prs)), "get_prs_fft_ref")
    check(lib().dabgpu_get_carrier_mapper(1, _ptr(mapper)), "get_carrier_mapper")
    check(lib().dabgpu_get_fft_twiddles(_ptr(tw)), "get_fft_twiddles")
    return prs, mapper, tw


class _Handle:
    """owns one handle of the library, `_h`; `_destroy` names the function that releases it"""
    _destroy = None

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_form(call, h_in, rows, n_out, fmt):
    """a *_host_sync call into `rows` padded output rows: call(x, n_in, out, stride); -> [rows][n_out] complex64, or [rows][n_out][2] uint8"""
    import numpy as np
    x = np.ascontiguousarray(h_in, dtype=np.complex64)
    sb = 8 if fmt == IQ_FORMATS.index("raw_f32l") else 2
    stride = (n_out * sb + 15) & ~15
    out = np.zeros((rows, stride), np.uint8)
    call(x, x.shape[-1], out, stride)
    out = out[:, :n_out * sb]
    return out.copy().view(np.complex64) if sb == 8 else out.reshape(rows, n_out, 2).copy()


class Context:
    """One device + constant tables (dabgpu_create / dabgpu_destroy)."""

    def __init__(self, device=0, prs_fft_ref=None, carrier_mapper=None):
        import numpy as np
        self._h = C.c_void_p()
        prs = None if prs_fft_ref is None else np.ascontiguousarray(prs_fft_ref, dtype=np.complex64)
        mp = None if carrier_mapper is None else np.ascontiguousarray(carrier_mapper, dtype=np.int32)
        check(lib().dabgpu_create(C.byref(self._h), device, _ptr(prs), _ptr(mp)), "dabgpu_create")
        self.device = device

    def close(self):
        if self._h:
            lib().dabgpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stream(stream):
        if stream is None:
            try:
                import torch
                if torch.cuda.is_available():
                    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
            except Exception:
                pass
            return None
        return C.c_void_p(int(stream))

    def synchronize(self, stream=None):
        check(lib().dabgpu_synchronize(self._h, self._stream(stream)), "dabgpu_synchronize")

    def ofdm_demod_frames(self, iq, bits, freq_offset=None, cp_corr=None, fft=None, symbols_per_block=0,
                          n_frames=None, stream=None, dqpsk=None, bits_frame_stride=0):
        """Launch the fused PLL+CP-phase+FFT+DQPSK+demap kernel on device buffers (asynchronous)."""
        if n_frames is None:
            n_frames = iq.numel() // NB_FRAME_SAMPLES if hasattr(iq, "numel") else None
        check(lib().dabgpu_ofdm_demod_frames(self._h, _ptr(iq), n_frames, _ptr(freq_offset), _ptr(bits),
                                             _ptr(cp_corr), _ptr(fft), _ptr(dqpsk), symbols_per_block, bits_frame_stride, self._stream(stream)),
              "dabgpu_ofdm_demod_frames")

    def ofdm_demod_frames_raw(self, raw, fmt, n_frames, bits, freq_offset=None, cp_corr=None, fft=None, symbols_per_block=0,
                              stream=None, dqpsk=None, bits_frame_stride=0):
        """The same from frames still in capture format number `fmt` (u8 / s8 / s16l are read by the kernel itself)."""
        check(lib().dabgpu_ofdm_demod_frames_raw(self._h, _ptr(raw), int(fmt), n_frames, _ptr(freq_offset), _ptr(bits),
                                                 _ptr(cp_corr), _ptr(fft), _ptr(dqpsk), symbols_per_block, bits_frame_stride,
                                                 self._stream(stream)), "dabgpu_ofdm_demod_frames_raw")

    def ofdm_demod_frames_history(self, raw, fmt, n_frames, bits, freq_offset=None, cp_corr=None, symbols_per_block=0,
                                  bits_frame_stride=0, bits_layout=BITS_NATURAL, stream=None):
        """Soft bits straight into the decoder's frame-history ring; bits_layout = BITS_MSC_CLASSED stores the MSC part in
        time-interleaver class order (read it with msc_decode_frames(..., bits_layout=BITS_MSC_CLASSED))."""
        check(lib().dabgpu_ofdm_demod_frames_history(self._h, _ptr(raw), int(fmt), n_frames, _ptr(freq_offset), _ptr(bits), _ptr(cp_corr),
                                                     symbols_per_block, bits_frame_stride, int(bits_layout), self._stream(stream)),
              "dabgpu_ofdm_demod_frames_history")

    def ofdm_demod_phase_frames(self, raw, fmt, n_frames, bits, freq_offset=None, cp_corr=None, symbols_per_block=0, bits_frame_stride=0,
                                bits_layout=BITS_NATURAL, beta=0.0, total_phase=None, fine_freq=None, stream=None):
        """demodulation + phase tail (ofdm_phase_update) as one call; one launch when a workgroup walks a whole frame"""
        check(lib().dabgpu_ofdm_demod_phase_frames(self._h, _ptr(raw), int(fmt), n_frames, _ptr(freq_offset), _ptr(bits), _ptr(cp_corr),
                                                   symbols_per_block, bits_frame_stride, int(bits_layout), float(beta), _ptr(total_phase),
                                                   _ptr(fine_freq), self._stream(stream)), "dabgpu_ofdm_demod_phase_frames")

    def ofdm_demod_frames_mode(self, mode, iq, n_frames, bits, freq_offset=None, cp_corr=None, fft=None, symbols_per_block=0, stream=None):
        """frame-aligned frames of transmission mode 1..4 through the size-generic kernel"""
        check(lib().dabgpu_ofdm_demod_frames_mode(self._h, int(mode), _ptr(iq), n_frames, _ptr(freq_offset), _ptr(bits), _ptr(cp_corr),
                                                  _ptr(fft), symbols_per_block, self._stream(stream)), "dabgpu_ofdm_demod_frames_mode")

    def ofdm_sync_host_mode(self, mode, prs_sym, state, cfg=None):
        """numpy convenience over dabgpu_ofdm_sync_host_sync_mode: returns (impulse_db[nb_fft], freq_response_db[nb_fft])"""
        import numpy as np
        n = ofdm_params(mode)["nb_fft"]
        cfg = cfg or sync_cfg_default()
        sym = np.ascontiguousarray(prs_sym, dtype=np.complex64).reshape(-1)
        assert sym.size == n
        imp = np.empty(n, dtype=np.float32)
        frq = np.empty(n, dtype=np.float32)
        check(lib().dabgpu_ofdm_sync_host_sync_mode(self._h, int(mode), _ptr(sym), C.byref(cfg), C.byref(state), _ptr(imp), _ptr(frq)),
              "dabgpu_ofdm_sync_host_sync_mode")
        return imp, frq

    def ofdm_phase_update_mode(self, mode, cp_corr, n_frames, total_phase=None, fine_freq=None, beta=0.9, stream=None):
        check(lib().dabgpu_ofdm_phase_update_mode(self._h, int(mode), _ptr(cp_corr), n_frames, beta, _ptr(total_phase), _ptr(fine_freq),
                                                  self._stream(stream)), "dabgpu_ofdm_phase_update_mode")

    def ofdm_phase_update(self, cp_corr, n_frames, total_phase=None, fine_freq=None, beta=0.9, stream=None):
        check(lib().dabgpu_ofdm_phase_update(self._h, _ptr(cp_corr), n_frames, beta, _ptr(total_phase),
                                             _ptr(fine_freq), self._stream(stream)), "dabgpu_ofdm_phase_update")

    def ofdm_demod_frames_host(self, iq, freq_offset=None, want_fft=False):
        """numpy in / numpy out convenience over dabgpu_ofdm_demod_frames_host_sync"""
        import numpy as np
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        n = iq.size // NB_FRAME_SAMPLES
        assert n * NB_FRAME_SAMPLES == iq.size
        f = None if freq_offset is None else np.ascontiguousarray(freq_offset, dtype=np.float32).reshape(-1)
        bits = np.empty((n, NB_FRAME_BITS), dtype=np.int8)
        total = np.empty(n, dtype=np.float32)
        fft = np.empty((n, 77, NB_FFT), dtype=np.complex64) if want_fft else None
        check(lib().dabgpu_ofdm_demod_frames_host_sync(self._h, _ptr(iq), n, _ptr(f), _ptr(bits), _ptr(total),
                                                       _ptr(fft)), "dabgpu_ofdm_demod_frames_host_sync")
        return bits, total, fft

    # ---- sync ----
    def ofdm_sync(self, prs_syms, n_streams, stride_samples, states, cfg=None, impulse=None, freq_response=None, stream=None):
        cfg = cfg or sync_cfg_default()
        check(lib().dabgpu_ofdm_sync(self._h, _ptr(prs_syms), n_streams, stride_samples, C.byref(cfg), _ptr(states),
                                     _ptr(impulse), _ptr(freq_response), self._stream(stream)), "dabgpu_ofdm_sync")

    def ofdm_sync_host(self, prs_sym, state, cfg=None):
        """numpy convenience: returns (state, impulse_response, freq_response)"""
        import numpy as np
        cfg = cfg or sync_cfg_default()
        x = np.ascontiguousarray(prs_sym, dtype=np.complex64)[:NB_FFT].copy()
        imp = np.empty(NB_FFT, dtype=np.float32)
        frq = np.empty(NB_FFT, dtype=np.float32)
        check(lib().dabgpu_ofdm_sync_host_sync(self._h, _ptr(x), C.byref(cfg), C.byref(state), _ptr(imp), _ptr(frq)),
              "dabgpu_ofdm_sync_host_sync")
        return state, imp, frq

    def ofdm_sync_demod_frames(self, iq, n_streams, stream_stride_samples, prs_offset_samples, states, bits, cfg=None, cp_corr=None,
                               symbols_per_block=0, bits_frame_stride=0, bits_layout=BITS_NATURAL, total_phase=None, stream=None):
        """PRS synchronisation -> demodulation at the position / with the offset it found -> fine-frequency update, one call (device
        buffers, asynchronous); `states` = [n_streams] dabgpu_sync_state records on the device, in/out"""
        cfg = cfg or sync_cfg_default()
        check(lib().dabgpu_ofdm_sync_demod_frames(self._h, _ptr(iq), n_streams, stream_stride_samples, prs_offset_samples, C.byref(cfg),
                                                  _ptr(states), _ptr(bits), _ptr(cp_corr), symbols_per_block, bits_frame_stride,
                                                  int(bits_layout), _ptr(total_phase), self._stream(stream)), "dabgpu_ofdm_sync_demod_frames")

    def ofdm_demod_frames_soft(self, raw, fmt, n_frames, bits, soft, freq_offset=None, cp_corr=None, fft=None, dqpsk=None, symbols_per_block=0,
                               bits_frame_stride=0, bits_layout=BITS_NATURAL, soft_scale=None, stream=None):
        """ofdm_demod_frames_raw / _history with a soft-decision policy (`soft` = a SoftCfg); soft_scale [n_frames] float32 on the
        device receives the scale of every frame under SOFT_CSI"""
        check(lib().dabgpu_ofdm_demod_frames_soft(self._h, _ptr(raw), int(fmt), n_frames, _ptr(freq_offset), _ptr(bits), _ptr(cp_corr), _ptr(fft),
                                                  _ptr(dqpsk), symbols_per_block, bits_frame_stride, int(bits_layout), C.byref(soft),
                                                  _ptr(soft_scale), self._stream(stream)), "dabgpu_ofdm_demod_frames_soft")

    def ofdm_sync_demod_frames_soft(self, iq, n_streams, stream_stride_samples, prs_offset_samples, states, bits, soft, cfg=None, cp_corr=None,
                                    symbols_per_block=0, bits_frame_stride=0, bits_layout=BITS_NATURAL, total_phase=None, soft_scale=None,
                                    stream=None):
        """ofdm_sync_demod_frames with a soft-decision policy (`soft` = a SoftCfg)"""
        cfg = cfg or sync_cfg_default()
        check(lib().dabgpu_ofdm_sync_demod_frames_soft(self._h, _ptr(iq), n_streams, stream_stride_samples, prs_offset_samples, C.byref(cfg),
                                                       _ptr(states), _ptr(bits), _ptr(cp_corr), symbols_per_block, bits_frame_stride,
                                                       int(bits_layout), _ptr(total_phase), C.byref(soft), _ptr(soft_scale),
                                                       self._stream(stream)), "dabgpu_ofdm_sync_demod_frames_soft")

    def ofdm_sync_demod_frames_branch(self, iq, n_streams, stream_stride_samples, prs_offset_samples, states, bits, soft, dqpsk, cfg=None,
                                      cp_corr=None, symbols_per_block=0, bits_frame_stride=0, total_phase=None, soft_scale=None, stream=None):
        """a synchronised diversity branch: ofdm_sync_demod_frames_soft (natural layout) that also writes the receivers' DQPSK products,
        dqpsk [n_streams][75][1536] complex float on the device"""
        cfg = cfg or sync_cfg_default()
        check(lib().dabgpu_ofdm_sync_demod_frames_branch(self._h, _ptr(iq), n_streams, stream_stride_samples, prs_offset_samples, C.byref(cfg),
                                                         _ptr(states), _ptr(bits), _ptr(cp_corr), symbols_per_block, bits_frame_stride,
                                                         _ptr(total_phase), C.byref(soft), _ptr(soft_scale), _ptr(dqpsk),
                                                         self._stream(stream)), "dabgpu_ofdm_sync_demod_frames_branch")

    def diversity_combine(self, branches, n_frames, bits, bits_frame_stride=0, bits_layout=BITS_NATURAL, symbols_per_block=0, soft_scale=None,
                          live_mask=None, stream=None, band_weights=None, symbol_weights=None):
        """receive diversity: `branches` = up to 8 of (dqpsk, scale[, weight[, sync]]) device buffers (or DiversityBranch records) of the same
        n_frames frames -> their combined soft bits in `bits`; soft_scale [n_frames] float32 and live_mask [n_frames] uint32 on the device
        receive the scale used and the live branches.  One kernel launch, no copy: capturable.  band_weights = one entry per branch, a
        device buffer [n_frames][128] of band weights (Context.noise_profile's) or None: dabgpu_diversity_combine_frames_banded.
        symbol_weights = one entry per branch, a device buffer [n_frames][75] of symbol weights (Context.sym_profile's) or None:
        dabgpu_diversity_combine_frames_symbols"""
        table = diversity_table(branches)
        args = [self._h, table, len(table), n_frames, _ptr(bits), bits_frame_stride, int(bits_layout), int(symbols_per_block), _ptr(soft_scale),
                _ptr(live_mask)]
        # the entry point follows the arguments given, not what they hold (the library itself goes by that)
        name = "dabgpu_diversity_combine_frames"
        if symbol_weights is not None:
            name += "_symbols"
            args.append(None if band_weights is None else band_weight_table(band_weights, len(table)))
            args.append(band_weight_table(symbol_weights, len(table), "symbol_weights"))
        elif band_weights is not None:
            name += "_banded"
            args.append(band_weight_table(band_weights, len(table)))
        check(getattr(lib(), name)(*args, self._stream(stream)), name)

    def diversity_combine_host(self, dqpsk, scales, weights=None, valid=None, bits_layout=BITS_NATURAL, band_weights=None, symbol_weights=None):
        """numpy convenience over dabgpu_diversity_combine_host_sync: one frame; dqpsk = a list of [75][1536] complex64 arrays (None where the
        branch is not live); returns (bits [230400] int8, scale, live mask).  band_weights = one [128] float32 array or None per branch:
        dabgpu_diversity_combine_banded_host_sync; symbol_weights = one [75] float32 array or None per branch:
        dabgpu_diversity_combine_symbols_host_sync"""
        import numpy as np
        n = len(dqpsk)
        # the entry point follows the arguments given; its tables ride behind the common arguments
        name, tables = "dabgpu_diversity_combine_host_sync", []
        if symbol_weights is not None:
            if len(symbol_weights) != n or (band_weights is not None and len(band_weights) != n):
                raise ValueError("diversity_combine_host: one band_weights and one symbol_weights entry per branch")
            name, tables = "dabgpu_diversity_combine_symbols_host_sync", [(band_weights, NOISE_PROFILE_BANDS), (symbol_weights, SYM_PROFILE_SYMBOLS)]
        elif band_weights is not None:
            if len(band_weights) != n:
                raise ValueError("diversity_combine_host: one band_weights entry per branch")
            name, tables = "dabgpu_diversity_combine_banded_host_sync", [(band_weights, NOISE_PROFILE_BANDS)]

        def rows(arrays, dtype, size):
            """(the addresses of the rows, null for a row that is None; what keeps them alive), or (None, None) for no array at all"""
            if arrays is None:
                return None, None
            keep = [None if x is None else np.ascontiguousarray(x, dtype=dtype).reshape(size) for x in arrays]
            return (C.c_void_p * n)(*[None if x is None else x.ctypes.data for x in keep]), keep

        ptrs, keep = rows(dqpsk, np.complex64, -1)
        k = np.ascontiguousarray(scales, dtype=np.float32).reshape(n)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32).reshape(n)
        v = None if valid is None else np.ascontiguousarray(valid, dtype=np.int32).reshape(n)
        extra = [rows(t, np.float32, size) for t, size in tables]
        bits = np.empty(NB_FRAME_BITS, np.int8)
        out_k, out_m = C.c_float(0.0), C.c_uint32(0)
        check(getattr(lib(), name)(self._h, ptrs, _ptr(k), _ptr(w), _ptr(v), n, int(bits_layout), _ptr(bits), C.byref(out_k), C.byref(out_m),
                                   *[e[0] for e in extra]), name)
        return bits, out_k.value, out_m.value

    def noise_estimate(self, iq, n_frames, stream_stride_samples, null_offset_samples, states=None, freq_offset=None, noise_power=None,
                       signal_power=None, weight=None, snr=None, group_energy=None, valid=None, stream=None):
        """the noise estimate of n_frames frames (include/dabgpu.h, "Noise estimate"): every output an optional device buffer, [n_frames]
        float32 each (group_energy [n_frames][192], valid uint32); `weight` can be a diversity branch's weight array as it is.  One kernel
        launch, no copy: capturable"""
        check(lib().dabgpu_noise_estimate_frames(self._h, _ptr(iq), n_frames, stream_stride_samples, null_offset_samples, _ptr(states),
                                                 _ptr(freq_offset), _ptr(noise_power), _ptr(signal_power), _ptr(weight), _ptr(snr),
                                                 _ptr(group_energy), _ptr(valid), self._stream(stream)), "dabgpu_noise_estimate_frames")

    def noise_profile(self, iq, n_frames, stream_stride_samples, null_offset_samples, states=None, freq_offset=None, exclude=None,
                      profile_in=None, alpha=1.0, profile_out=None, band_weight=None, mean_noise=None, carrier_power=None, valid=None, stream=None):
        """the noise profile of n_frames frames (include/dabgpu.h, "Noise profile"): exclude = 48 uint32 words on the device
        (noise_profile_exclude), profile_in / profile_out [n_frames][128] float32 the smoothing state (may be one buffer), band_weight
        [n_frames][128] (an entry of diversity_combine's band_weights as it is), mean_noise [n_frames], carrier_power [n_frames][1536],
        valid [n_frames] uint32; every output optional.  One kernel launch, no copy: capturable"""
        check(lib().dabgpu_noise_profile_frames(self._h, _ptr(iq), n_frames, stream_stride_samples, null_offset_samples, _ptr(states),
                                                _ptr(freq_offset), _ptr(exclude), _ptr(profile_in), float(alpha), _ptr(profile_out),
                                                _ptr(band_weight), _ptr(mean_noise), _ptr(carrier_power), _ptr(valid), self._stream(stream)),
              "dabgpu_noise_profile_frames")

    def noise_profile_host(self, samples, null_offset_samples, freq_offset=0.0, fine_time_offset=0, exclude=None, profile=None, alpha=1.0,
                           carrier_power=False):
        """numpy convenience over dabgpu_noise_profile_host_sync: one frame's NULL out of complex64 samples -> (band weights [128], mean
        noise, valid[, carrier powers [1536]]); profile = a [128] float32 array, the state, updated in place"""
        import numpy as np
        x = np.ascontiguousarray(samples, dtype=np.complex64).reshape(-1)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint32).reshape(NOISE_PROFILE_EXCLUDE_WORDS)
        if profile is not None and (profile.dtype != np.float32 or profile.size != NOISE_PROFILE_BANDS or not profile.flags.c_contiguous):
            raise ValueError("noise_profile_host: profile must be a contiguous float32 array of 128")
        bw, cp = np.zeros(NOISE_PROFILE_BANDS, np.float32), (np.zeros(NB_CARRIERS, np.float32) if carrier_power else None)
        mean, ok = C.c_float(0.0), C.c_uint32(0)
        check(lib().dabgpu_noise_profile_host_sync(self._h, _ptr(x), x.size, null_offset_samples, float(freq_offset), int(fine_time_offset), _ptr(ex),
                                                   _ptr(profile), float(alpha), _ptr(bw), C.byref(mean), _ptr(cp), C.byref(ok)),
              "dabgpu_noise_profile_host_sync")
        return (bw, mean.value, ok.value) + ((cp,) if carrier_power else ())

    def dd_profile(self, dqpsk, n_frames, sync=None, exclude=None, profile_in=None, alpha=1.0, profile_out=None, band_weight=None,
                   mean_noise=None, carrier_noise=None, carrier_amplitude=None, valid=None, stream=None):
        """the decision-directed noise profile of n_frames frames (include/dabgpu.h, "Decision-directed noise profile"): dqpsk
        [n_frames][75][1536] complex64 and sync the records of ofdm_sync_demod_frames_branch, exclude = 48 uint32 words on the device,
        profile_in / profile_out [n_frames][128] float32 the smoothing state (may be one buffer), band_weight [n_frames][128] (an entry
        of diversity_combine's band_weights as it is), mean_noise [n_frames], carrier_noise / carrier_amplitude [n_frames][1536], valid
        [n_frames] uint32; every output optional.  One kernel launch, no copy: capturable"""
        check(lib().dabgpu_dd_profile_frames(self._h, _ptr(dqpsk), n_frames, _ptr(sync), _ptr(exclude), _ptr(profile_in), float(alpha),
                                             _ptr(profile_out), _ptr(band_weight), _ptr(mean_noise), _ptr(carrier_noise), _ptr(carrier_amplitude),
                                             _ptr(valid), self._stream(stream)), "dabgpu_dd_profile_frames")

    def dd_profile_host(self, dqpsk, exclude=None, profile=None, alpha=1.0, carriers=False):
        """numpy convenience over dabgpu_dd_profile_host_sync: one frame's products [75][1536] complex64 -> (band weights [128], mean
        noise, valid[, carrier noise [1536], carrier amplitude [1536]]); profile = a [128] float32 array, the state, updated in place"""
        import numpy as np
        x = np.ascontiguousarray(dqpsk, dtype=np.complex64).reshape(75 * NB_CARRIERS)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint32).reshape(NOISE_PROFILE_EXCLUDE_WORDS)
        if profile is not None and (profile.dtype != np.float32 or profile.size != NOISE_PROFILE_BANDS or not profile.flags.c_contiguous):
            raise ValueError("dd_profile_host: profile must be a contiguous float32 array of 128")
        bw = np.zeros(NOISE_PROFILE_BANDS, np.float32)
        q, a = (np.zeros(NB_CARRIERS, np.float32), np.zeros(NB_CARRIERS, np.float32)) if carriers else (None, None)
        mean, ok = C.c_float(0.0), C.c_uint32(0)
        check(lib().dabgpu_dd_profile_host_sync(self._h, _ptr(x), _ptr(ex), _ptr(profile), float(alpha), _ptr(bw), C.byref(mean), _ptr(q), _ptr(a),
                                                C.byref(ok)), "dabgpu_dd_profile_host_sync")
        return (bw, mean.value, ok.value) + ((q, a) if carriers else ())

    def sym_profile(self, dqpsk, n_frames, sync=None, symbol_weight=None, symbol_noise=None, ref_noise=None, valid=None, stream=None):
        """the symbol noise profile of n_frames frames (include/dabgpu.h, "Symbol noise profile"): dqpsk [n_frames][75][1536] complex64 and
        sync the records of ofdm_sync_demod_frames_branch; symbol_weight [n_frames][75] float32 (an entry of diversity_combine's
        symbol_weights as it is), symbol_noise [n_frames][75], ref_noise [n_frames], valid [n_frames] uint32; every output optional.  One
        kernel launch, no copy: capturable"""
        check(lib().dabgpu_sym_profile_frames(self._h, _ptr(dqpsk), n_frames, _ptr(sync), _ptr(symbol_weight), _ptr(symbol_noise), _ptr(ref_noise),
                                              _ptr(valid), self._stream(stream)), "dabgpu_sym_profile_frames")

    def sym_profile_host(self, dqpsk):
        """numpy convenience over dabgpu_sym_profile_host_sync: one frame's products [75][1536] complex64 -> (symbol weights [75], symbol
        noise [75], reference noise, valid)"""
        import numpy as np
        x = np.ascontiguousarray(dqpsk, dtype=np.complex64).reshape(SYM_PROFILE_SYMBOLS * NB_CARRIERS)
        v, q = np.zeros(SYM_PROFILE_SYMBOLS, np.float32), np.zeros(SYM_PROFILE_SYMBOLS, np.float32)
        ref, ok = C.c_float(0.0), C.c_uint32(0)
        check(lib().dabgpu_sym_profile_host_sync(self._h, _ptr(x), _ptr(v), _ptr(q), C.byref(ref), C.byref(ok)), "dabgpu_sym_profile_host_sync")
        return v, q, ref.value, ok.value

    def clock_estimate(self, dqpsk, n_frames, sync=None, slope_in=None, gain=1.0, slope_out=None, residual=None, corr=None, valid=None,
                       stream=None):
        """the sampling-clock estimator over n_frames frames (include/dabgpu.h, "Sampling-clock tracker"): dqpsk [n_frames][75][1536]
        complex64 and sync the records of ofdm_sync_demod_frames_branch; slope_in [n_frames] int64 (None: zero), slope_out [n_frames]
        int64 (may be slope_in itself: the state), residual [n_frames] int64, corr [n_frames][2] float32, valid [n_frames] uint32; every
        output optional.  One kernel launch, no copy: capturable"""
        check(lib().dabgpu_clock_estimate_frames(self._h, _ptr(dqpsk), n_frames, _ptr(sync), _ptr(slope_in), float(gain), _ptr(slope_out),
                                                 _ptr(residual), _ptr(corr), _ptr(valid), self._stream(stream)), "dabgpu_clock_estimate_frames")

    def clock_derotate(self, dqpsk_in, dqpsk_out, n_frames, slope, sync=None, symbols_per_block=0, stream=None):
        """the products of n_frames frames with the ramp of slope [n_frames] int64 taken out; dqpsk_out may be dqpsk_in.  A frame of slope 0
        is a copy (in place: untouched), a frame whose record in sync is not valid is neither read nor written.  symbols_per_block: the
        rows a workgroup walks (0: the planner's choice; the bytes do not depend on it).  One kernel launch: capturable"""
        check(lib().dabgpu_clock_derotate_frames_split(self._h, _ptr(dqpsk_in), _ptr(dqpsk_out), n_frames, _ptr(sync), _ptr(slope),
                                                       int(symbols_per_block), self._stream(stream)), "dabgpu_clock_derotate_frames")

    def clock_track_host(self, dqpsk, slope=0, gain=1.0, derotate=True):
        """numpy convenience over dabgpu_clock_track_host_sync: one frame's products [75][1536] complex64 through the estimator and the
        de-rotator -> (de-rotated products or None, new slope word, corr [2], valid)"""
        import numpy as np
        x = np.ascontiguousarray(dqpsk, dtype=np.complex64).reshape(75 * NB_CARRIERS)
        out = np.zeros_like(x) if derotate else None
        s, corr, ok = C.c_int64(int(slope)), np.zeros(2, np.float32), C.c_uint32(0)
        check(lib().dabgpu_clock_track_host_sync(self._h, _ptr(x), _ptr(out), C.byref(s), float(gain), _ptr(corr), C.byref(ok)),
              "dabgpu_clock_track_host_sync")
        return (None if out is None else out.reshape(75, NB_CARRIERS)), s.value, corr, ok.value

    def noise_estimate_host(self, samples, null_offset_samples, freq_offset=0.0, fine_time_offset=0):
        """numpy convenience over dabgpu_noise_estimate_host_sync: one frame's NULL and phase reference symbol out of complex64 samples ->
        a NOISE_RECORD_DTYPE record"""
        import numpy as np
        x = np.ascontiguousarray(samples, dtype=np.complex64).reshape(-1)
        rec = np.zeros(1, np.dtype(NOISE_RECORD_DTYPE))
        check(lib().dabgpu_noise_estimate_host_sync(self._h, _ptr(x), x.size, null_offset_samples, float(freq_offset), int(fine_time_offset),
                                                    _ptr(rec)), "dabgpu_noise_estimate_host_sync")
        return rec[0]

    def ofdm_tune(self, raw, fmt, n_frames, bits, bits_frame_stride=0, bits_layout=BITS_NATURAL, with_phase_tail=False, stream=None):
        """explicit (blocking) calibration of symbols_per_block = 0 for this call shape; returns the run length recorded"""
        chosen = C.c_int(0)
        check(lib().dabgpu_ofdm_tune(self._h, _ptr(raw), int(fmt), n_frames, _ptr(bits), bits_frame_stride, int(bits_layout),
                                     int(bool(with_phase_tail)), self._stream(stream), C.byref(chosen)), "dabgpu_ofdm_tune")
        return chosen.value

    def ofdm_tuned_symbols_per_block(self, fmt, n_frames, bits_layout=BITS_NATURAL, with_phase_tail=False):
        """what symbols_per_block = 0 resolves to for that call shape right now"""
        return int(lib().dabgpu_ofdm_tuned_symbols_per_block(self._h, int(fmt), int(n_frames), int(bits_layout), int(bool(with_phase_tail))))

    # ---- channel decode ----
    def ofdm_auto_symbols_per_block(self, n_frames):
        """the run length dabgpu_ofdm_tune last recorded for the size bucket of n_frames (0 = nothing recorded)"""
        return int(lib().dabgpu_ofdm_auto_symbols_per_block(self._h, int(n_frames)))

    def viterbi_set_mapping(self, mapping):
        """0 = auto, 1 = one wavefront per codeword, 2 = one lane per codeword, 3 = eight lanes per codeword (include/dabgpu.h DABGPU_VIT_MAP_*)."""
        check(lib().dabgpu_viterbi_set_mapping(self._h, int(mapping)), "dabgpu_viterbi_set_mapping")

    def multiplex_mapping(self, n_ensembles, subchannels):
        """(mapping the MSC decode of this multiplex takes: 1 wave / 2 lane / 3 octet, modelled microseconds of the three)"""
        n = len(subchannels)
        arr = (SubChannel * n)(*subchannels)
        m, us = C.c_int(0), (C.c_double * 3)()
        lib().dabgpu_multiplex_mapping.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        check(lib().dabgpu_multiplex_mapping(self._h, n_ensembles, arr, n, C.byref(m), us), "dabgpu_multiplex_mapping")
        return m.value, {"wave": us[0], "lane": us[1], "octet": us[2]}

    def viterbi_decode_batch(self, codewords, results, tie_rule=0, stream=None):
        """codewords: list/ctypes array of Codeword (host); results: device buffer of n CodewordResult"""
        n = len(codewords)
        arr = (Codeword * n)(*codewords) if not isinstance(codewords, C.Array) else codewords
        check(lib().dabgpu_viterbi_decode_batch(self._h, arr, n, tie_rule, _ptr(results), self._stream(stream)),
              "dabgpu_viterbi_decode_batch")

    def fic_decode_frames(self, bits, n_frames, fib_bytes, results, frame_stride=NB_FRAME_BITS, tie_rule=0, stream=None):
        check(lib().dabgpu_fic_decode_frames(self._h, _ptr(bits), n_frames, frame_stride, _ptr(fib_bytes), _ptr(results),
                                             tie_rule, self._stream(stream)), "dabgpu_fic_decode_frames")

    def fic_decode_ring(self, history, n_ensembles, ensemble_stride, newest_slot, fib_bytes, results, tie_rule=0, stream=None):
        check(lib().dabgpu_fic_decode_ring(self._h, _ptr(history), n_ensembles, ensemble_stride, _ptr(newest_slot), _ptr(fib_bytes),
                                           _ptr(results), tie_rule, self._stream(stream)), "dabgpu_fic_decode_ring")

    def msc_decode_ring(self, history, n_ensembles, ensemble_stride, history_frames, newest_slot, subchannels, out, out_ensemble_stride,
                        results, tie_rule=0, stream=None, bits_layout=BITS_NATURAL):
        n = len(subchannels)
        arr = (SubChannel * n)(*subchannels)
        if bits_layout != BITS_NATURAL:
            check(lib().dabgpu_msc_decode_ring_layout(self._h, _ptr(history), n_ensembles, ensemble_stride, history_frames, _ptr(newest_slot),
                                                      arr, n, _ptr(out), out_ensemble_stride, _ptr(results), tie_rule, int(bits_layout),
                                                      self._stream(stream)), "dabgpu_msc_decode_ring_layout")
            return
        check(lib().dabgpu_msc_decode_ring(self._h, _ptr(history), n_ensembles, ensemble_stride, history_frames, _ptr(newest_slot), arr, n,
                                           _ptr(out), out_ensemble_stride, _ptr(results), tie_rule, self._stream(stream)),
              "dabgpu_msc_decode_ring")

    def decode_frames(self, history, n_ensembles, ensemble_stride, history_frames, newest_frame_slot, subchannels, fib_bytes, fic_results,
                      out, out_ensemble_stride, results, tie_rule=0, stream=None, bits_layout=BITS_NATURAL):
        """FIC (ring slot newest_frame_slot) + MSC of one transmission frame of every ensemble in one call (dabgpu_decode_frames_layout)"""
        n = len(subchannels)
        arr = (SubChannel * n)(*subchannels) if n else None
        check(lib().dabgpu_decode_frames_layout(self._h, _ptr(history), n_ensembles, ensemble_stride, history_frames, newest_frame_slot, arr, n,
                                                _ptr(fib_bytes), _ptr(fic_results), _ptr(out), out_ensemble_stride, _ptr(results), tie_rule,
                                                int(bits_layout), self._stream(stream)), "dabgpu_decode_frames_layout")

    def decode_ring(self, history, n_ensembles, ensemble_stride, history_frames, newest_slot, subchannels, fib_bytes, fic_results,
                    out, out_ensemble_stride, results, tie_rule=0, stream=None, bits_layout=BITS_NATURAL):
        n = len(subchannels)
        arr = (SubChannel * n)(*subchannels) if n else None
        check(lib().dabgpu_decode_ring_layout(self._h, _ptr(history), n_ensembles, ensemble_stride, history_frames, _ptr(newest_slot), arr, n,
                                              _ptr(fib_bytes), _ptr(fic_results), _ptr(out), out_ensemble_stride, _ptr(results), tie_rule,
                                              int(bits_layout), self._stream(stream)), "dabgpu_decode_ring_layout")

    def msc_decode_frames(self, history, n_ensembles, ensemble_stride, history_frames, newest_frame_slot, subchannels,
                          out, out_ensemble_stride, results, tie_rule=0, stream=None, bits_layout=BITS_NATURAL):
        n = len(subchannels)
        arr = (SubChannel * n)(*subchannels)
        if bits_layout != BITS_NATURAL:
            check(lib().dabgpu_msc_decode_frames_layout(self._h, _ptr(history), n_ensembles, ensemble_stride, history_frames,
                                                        newest_frame_slot, arr, n, _ptr(out), out_ensemble_stride, _ptr(results),
                                                        tie_rule, int(bits_layout), self._stream(stream)), "dabgpu_msc_decode_frames_layout")
            return
        check(lib().dabgpu_msc_decode_frames(self._h, _ptr(history), n_ensembles, ensemble_stride, history_frames,
                                             newest_frame_slot, arr, n, _ptr(out), out_ensemble_stride, _ptr(results),
                                             tie_rule, self._stream(stream)), "dabgpu_msc_decode_frames")

    def ber_frames(self, history, n_ensembles, ensemble_stride, history_frames, newest_frame_slot, subchannels, fib_bytes, msc_out,
                   out_ensemble_stride, fic_ber, msc_ber, stream=None, bits_layout=BITS_NATURAL):
        """channel BER of the code words decode_frames decoded (dabgpu_ber_frames_layout): fib_bytes / msc_out as that call left them,
        fic_ber [n][4] and msc_ber [n][4][n_sub] device buffers of BER_RESULT_DTYPE; a half whose bytes or records are None is skipped"""
        n = len(subchannels)
        arr = (SubChannel * n)(*subchannels) if n else None
        check(lib().dabgpu_ber_frames_layout(self._h, _ptr(history), n_ensembles, ensemble_stride, history_frames, newest_frame_slot, arr, n,
                                             _ptr(fib_bytes), _ptr(msc_out), out_ensemble_stride, _ptr(fic_ber), _ptr(msc_ber), int(bits_layout),
                                             self._stream(stream)), "dabgpu_ber_frames_layout")

    def ber_ring(self, history, n_ensembles, ensemble_stride, history_frames, newest_slot, subchannels, fib_bytes, msc_out, out_ensemble_stride,
                 fic_ber, msc_ber, stream=None, bits_layout=BITS_NATURAL):
        """ber_frames for rings: newest_slot = device int32 [n], a negative slot yields all-zero records (dabgpu_ber_ring_layout)"""
        n = len(subchannels)
        arr = (SubChannel * n)(*subchannels) if n else None
        check(lib().dabgpu_ber_ring_layout(self._h, _ptr(history), n_ensembles, ensemble_stride, history_frames, _ptr(newest_slot), arr, n,
                                           _ptr(fib_bytes), _ptr(msc_out), out_ensemble_stride, _ptr(fic_ber), _ptr(msc_ber), int(bits_layout),
                                           self._stream(stream)), "dabgpu_ber_ring_layout")

    def ber_fib_group(self, bits, fib_bytes):
        """one FIB group from host memory: 2304 soft bits, 96 decoded bytes -> record of BER_RESULT_DTYPE (dabgpu_ber_fib_group_host_sync)"""
        import numpy as np
        b = np.ascontiguousarray(bits, dtype=np.int8)
        d = np.ascontiguousarray(fib_bytes, dtype=np.uint8)
        assert b.size == NB_FIB_GROUP_BITS and d.size == 96
        res = np.zeros(1, np.dtype(BER_RESULT_DTYPE))
        check(lib().dabgpu_ber_fib_group_host_sync(self._h, _ptr(b), _ptr(d), _ptr(res)), "dabgpu_ber_fib_group_host_sync")
        return res[0]

    def ber_codeword(self, subchannel, deinterleaved_bits, decoded_bytes):
        """one sub-channel code word from host memory: its de-interleaved CIF and decoded bytes (dabgpu_ber_codeword_host_sync)"""
        import numpy as np
        b = np.ascontiguousarray(deinterleaved_bits, dtype=np.int8)
        d = np.ascontiguousarray(decoded_bytes, dtype=np.uint8)
        _, _, nb = subchannel_plan(subchannel)
        assert b.size == subchannel.length * 64 and d.size == nb
        res = np.zeros(1, np.dtype(BER_RESULT_DTYPE))
        check(lib().dabgpu_ber_codeword_host_sync(self._h, C.byref(subchannel), _ptr(b), _ptr(d), _ptr(res)), "dabgpu_ber_codeword_host_sync")
        return res[0]

    def iq_convert(self, raw, fmt, n_samples, iq, stream=None):
        """device raw samples in format number `fmt` -> device interleaved float IQ (asynchronous)"""
        check(lib().dabgpu_iq_convert(self._h, _ptr(raw), int(fmt), n_samples, _ptr(iq), self._stream(stream)), "dabgpu_iq_convert")

    def iq_convert_host(self, raw, fmt):
        import numpy as np
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        sb = iq_format_sample_bytes(fmt)
        if sb == 0:
            raise DabGpuError(f"unknown IQ format number {fmt}")
        n = raw.size // sb
        out = np.empty(2 * n, np.float32)
        check(lib().dabgpu_iq_convert_host_sync(self._h, _ptr(raw), int(fmt), n, _ptr(out)), "dabgpu_iq_convert_host_sync")
        return out

    def ofdm_modulate_frames(self, mode, payload, n_frames, out, layout=TX_PAYLOAD_REFERENCE, out_format=None, prs_fft_ref=None,
                             freq_norm=0.0, stream=None):
        """OFDM transmitter (asynchronous): n_frames payloads on the device -> NULL-first frames in `out` (device, 16-byte aligned);
        out_format = IQ_FORMATS.index("raw_f32l") (default) or IQ_FORMATS.index("raw_u8"); prs_fft_ref = device spectrum or None"""
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        check(lib().dabgpu_ofdm_modulate_frames(self._h, int(mode), _ptr(payload), int(layout), n_frames, _ptr(prs_fft_ref), float(freq_norm),
                                                _ptr(out), fmt, self._stream(stream)), "dabgpu_ofdm_modulate_frames")

    def ofdm_modulate_frames_host(self, mode, payload, n_frames, layout=TX_PAYLOAD_REFERENCE, out_format=None, prs_fft_ref=None, freq_norm=0.0):
        """numpy form: returns [n_frames][samples per frame] complex64 (raw_f32l) or [n_frames][2 * samples] uint8 (raw_u8)"""
        import numpy as np
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        n_samp = ofdm_params(mode)["nb_frame_samples"]
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        prs = None if prs_fft_ref is None else np.ascontiguousarray(prs_fft_ref, dtype=np.complex64)
        out = np.empty((n_frames, n_samp), np.complex64) if fmt == IQ_FORMATS.index("raw_f32l") else np.empty((n_frames, 2 * n_samp), np.uint8)
        check(lib().dabgpu_ofdm_modulate_frames_host_sync(self._h, int(mode), _ptr(payload), int(layout), n_frames, _ptr(prs), float(freq_norm),
                                                          _ptr(out), fmt), "dabgpu_ofdm_modulate_frames_host_sync")
        return out

    def ofdm_modulate_frames_tii(self, mode, payload, n_frames, out, tii, tii_count, layout=TX_PAYLOAD_REFERENCE, out_format=None,
                                 prs_fft_ref=None, freq_norm=0.0, stream=None):
        """ofdm_modulate_frames with the TII symbol in the NULL period: tii = device [n_frames][4] TII_TX_DTYPE, tii_count = device
        [n_frames] uint8 (either None: no TII)"""
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        check(lib().dabgpu_ofdm_modulate_frames_tii(self._h, int(mode), _ptr(payload), int(layout), n_frames, _ptr(prs_fft_ref), float(freq_norm),
                                                    _ptr(out), fmt, self._stream(stream), _ptr(tii), _ptr(tii_count)),
              "dabgpu_ofdm_modulate_frames_tii")

    def ofdm_modulate_frames_tii_host(self, mode, payload, n_frames, tii, layout=TX_PAYLOAD_REFERENCE, out_format=None, prs_fft_ref=None,
                                      freq_norm=0.0):
        """numpy form: tii = per frame a list of (main_id, sub_id, amp), at most TII_MAX_TX each (tii_lists packs them)"""
        import numpy as np
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        n_samp = ofdm_params(mode)["nb_frame_samples"]
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        prs = None if prs_fft_ref is None else np.ascontiguousarray(prs_fft_ref, dtype=np.complex64)
        lists, counts = tii_lists(tii, n_frames)
        out = np.empty((n_frames, n_samp), np.complex64) if fmt == IQ_FORMATS.index("raw_f32l") else np.empty((n_frames, 2 * n_samp), np.uint8)
        check(lib().dabgpu_ofdm_modulate_frames_tii_host_sync(self._h, int(mode), _ptr(payload), int(layout), n_frames, _ptr(prs), float(freq_norm),
                                                              _ptr(out), fmt, _ptr(lists), _ptr(counts)), "dabgpu_ofdm_modulate_frames_tii_host_sync")
        return out

    def soft_bits_to_hard_bytes(self, bits, n_bytes, out, stream=None):
        check(lib().dabgpu_soft_bits_to_hard_bytes(self._h, _ptr(bits), n_bytes, _ptr(out), self._stream(stream)),
              "dabgpu_soft_bits_to_hard_bytes")

    def hard_bytes_to_soft_bits(self, data, n_bytes, out, stream=None):
        check(lib().dabgpu_hard_bytes_to_soft_bits(self._h, _ptr(data), n_bytes, _ptr(out), self._stream(stream)),
              "dabgpu_hard_bytes_to_soft_bits")

    def soft_bits_to_hard_bytes_host(self, bits):
        import numpy as np
        bits = np.ascontiguousarray(bits, dtype=np.int8)
        out = np.empty(bits.size // 8, np.uint8)
        check(lib().dabgpu_soft_bits_to_hard_bytes_host_sync(self._h, _ptr(bits), out.size, _ptr(out)), "soft_bits_to_hard_bytes_host_sync")
        return out

    def hard_bytes_to_soft_bits_host(self, data):
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        out = np.empty(data.size * 8, np.int8)
        check(lib().dabgpu_hard_bytes_to_soft_bits_host_sync(self._h, _ptr(data), data.size, _ptr(out)), "hard_bytes_to_soft_bits_host_sync")
        return out


class StreamBank(_Handle):
    """dabgpu_stream_bank: n unsynchronised receivers resident on the device (one OFDM_Demod each)"""
    _destroy = "dabgpu_stream_bank_destroy"

    def __init__(self, ctx, n_streams, cfg=None, mode=1):
        self._ctx = ctx
        self.n = n_streams
        self.mode = mode
        self._h = C.c_void_p()
        check(lib().dabgpu_stream_bank_create_mode(ctx._h, int(mode), n_streams, C.byref(cfg) if cfg is not None else None, C.byref(self._h)),
              "dabgpu_stream_bank_create_mode")

    def reset(self, stream=None):
        check(lib().dabgpu_stream_bank_reset(self._h, Context._stream(stream)), "dabgpu_stream_bank_reset")

    def process(self, iq, stream_stride_samples, n_samples, bits, max_frames, n_frames=None, stream=None):
        check(lib().dabgpu_stream_bank_process(self._h, _ptr(iq), stream_stride_samples, n_samples, _ptr(bits), max_frames,
                                               _ptr(n_frames), Context._stream(stream)), "dabgpu_stream_bank_process")

    def process_raw(self, raw, fmt, stream_stride_samples, n_samples, bits, max_frames, n_frames=None, stream=None):
        check(lib().dabgpu_stream_bank_process_raw(self._h, _ptr(raw), int(fmt), stream_stride_samples, n_samples, _ptr(bits), max_frames,
                                                   _ptr(n_frames), Context._stream(stream)), "dabgpu_stream_bank_process_raw")

    def process_retained(self, raw, fmt, stream_stride_samples, n_samples, prev_raw, bits, max_frames, n_frames=None, stream=None):
        """process_raw for callers that keep `raw` valid and unchanged until the NEXT call has returned: no carry-over copy at the end of
        the block; prev_raw = the block of the previous retained call (None at the first)"""
        check(lib().dabgpu_stream_bank_process_retained(self._h, _ptr(raw), int(fmt), stream_stride_samples, n_samples, _ptr(prev_raw), _ptr(bits),
                                                        max_frames, _ptr(n_frames), Context._stream(stream)), "dabgpu_stream_bank_process_retained")

    def release(self, prev_raw, fmt, stream_stride_samples, stream=None):
        check(lib().dabgpu_stream_bank_release(self._h, _ptr(prev_raw), int(fmt), stream_stride_samples, Context._stream(stream)),
              "dabgpu_stream_bank_release")

    def process_ring(self, raw, fmt, stream_stride_samples, n_samples, hist, hist_frames, newest_slot, stream=None, bits_layout=BITS_NATURAL):
        if bits_layout != BITS_NATURAL:
            check(lib().dabgpu_stream_bank_process_ring_layout(self._h, _ptr(raw), int(fmt), stream_stride_samples, n_samples, _ptr(hist),
                                                               hist_frames, _ptr(newest_slot), int(bits_layout), Context._stream(stream)),
                  "dabgpu_stream_bank_process_ring_layout")
            return
        check(lib().dabgpu_stream_bank_process_ring(self._h, _ptr(raw), int(fmt), stream_stride_samples, n_samples, _ptr(hist), hist_frames,
                                                    _ptr(newest_slot), Context._stream(stream)), "dabgpu_stream_bank_process_ring")

    def process_ring_retained(self, raw, fmt, stream_stride_samples, n_samples, prev_raw, hist, hist_frames, newest_slot, stream=None, bits_layout=BITS_NATURAL):
        """process_ring for callers that keep `raw` valid and unchanged until the NEXT call has returned (no carry-over copy);
        prev_raw = the block of the previous retained call (None at the first)"""
        check(lib().dabgpu_stream_bank_process_ring_retained(self._h, _ptr(raw), int(fmt), stream_stride_samples, n_samples, _ptr(prev_raw), _ptr(hist),
                                                             hist_frames, _ptr(newest_slot), int(bits_layout), Context._stream(stream)),
              "dabgpu_stream_bank_process_ring_retained")

    def set_soft(self, soft, soft_scale=None):
        """the soft-decision policy (`soft` = a SoftCfg) of every frame demodulated from the next process call on; soft_scale = a float32
        tensor on the device that receives the scale of the frame in bits slot j of stream s at [s * max_frames + j] (ring forms:
        [s * hist_frames + ring slot]).  The bank keeps the address: keep the tensor alive while the policy is set
        (dabgpu_stream_bank_set_soft)"""
        check(lib().dabgpu_stream_bank_set_soft(self._h, C.byref(soft), _ptr(soft_scale), 0 if soft_scale is None else int(soft_scale.numel())),
              "dabgpu_stream_bank_set_soft")
        self._soft_scale = soft_scale

    def get_soft(self):
        soft = SoftCfg()
        check(lib().dabgpu_stream_bank_get_soft(self._h, C.byref(soft)), "dabgpu_stream_bank_get_soft")
        return soft

    def set_products(self, dqpsk, records):
        """the DQPSK products and sync records of every frame the frames forms complete from the next call on, by bits slot: dqpsk = a
        device tensor of [capacity][75][1536] complex64 (or [...][2] float32), records = a device tensor of capacity SYNC_STATE_DTYPE
        records (24 bytes each; any dtype).  With set_soft's soft_scale they are a diversity branch (dqpsk, soft_scale, None, records)
        and the (dqpsk, sync) pair of dd_profile, sym_profile, clock_estimate and clock_derotate as they stand.  Both None switches the
        feature off.  The bank keeps the addresses: the tensors are kept alive here (dabgpu_stream_bank_set_products)"""
        cap = 0
        if dqpsk is not None and records is not None:
            cap = min(int(dqpsk.numel()) * int(dqpsk.element_size()) // (75 * NB_CARRIERS * 8), int(records.numel()) * int(records.element_size()) // 24)
        check(lib().dabgpu_stream_bank_set_products(self._h, _ptr(dqpsk), _ptr(records), cap), "dabgpu_stream_bank_set_products")
        self._products = (dqpsk, records)

    def get_products(self):
        """(dqpsk, records, capacity in frames): the tensors set_products was given (None, None, 0 when the feature is off); the addresses
        and the capacity are read back from the bank (dabgpu_stream_bank_get_products)"""
        d, r, cap = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        check(lib().dabgpu_stream_bank_get_products(self._h, C.byref(d), C.byref(r), C.byref(cap)), "dabgpu_stream_bank_get_products")
        if not d.value:
            return None, None, 0
        dq, rec = getattr(self, "_products", (None, None))
        if dq is None or dq.data_ptr() != d.value or rec.data_ptr() != r.value:          # (set through the C ABI directly)
            return d.value, r.value, cap.value
        return dq, rec, cap.value

    def status(self, stream=None):
        import numpy as np
        out = np.zeros(self.n, dtype=np.dtype(STREAM_STATUS_DTYPE))
        check(lib().dabgpu_stream_bank_status(self._h, _ptr(out), Context._stream(stream)), "dabgpu_stream_bank_status")
        return out


class TxBank(_Handle):
    """dabgpu_tx_bank: the channel encoder of n ensembles sharing one multiplex (FIB bodies + sub-channel bytes -> frame bits -> IQ)"""
    _destroy = "dabgpu_tx_bank_destroy"

    def __init__(self, ctx, n_ensembles, subchannels):
        self._ctx = ctx
        self.n = n_ensembles
        self.plan = tx_encode_plan(subchannels)
        self.cif_in_bytes = self.plan["cif_in_bytes"]
        n = len(subchannels)
        arr = (SubChannel * n)(*subchannels) if n else None
        self._h = C.c_void_p()
        check(lib().dabgpu_tx_bank_create(ctx._h, n_ensembles, arr, n, C.byref(self._h)), "dabgpu_tx_bank_create")

    def reset(self, stream=None):
        check(lib().dabgpu_tx_bank_reset(self._h, Context._stream(stream)), "dabgpu_tx_bank_reset")

    def encode_frames(self, fib_data, payload, n_frames, frame_bits, frame_stride=0, stream=None):
        """fib_data [n][F][4][3][30], payload [n][F][4][cif_in_bytes] -> frame_bits [n][F] frames of 28800 bytes (device, asynchronous)"""
        check(lib().dabgpu_tx_bank_encode_frames(self._h, _ptr(fib_data), _ptr(payload), n_frames, _ptr(frame_bits), frame_stride,
                                                 Context._stream(stream)), "dabgpu_tx_bank_encode_frames")

    def transmit_frames(self, fib_data, payload, n_frames, out, freq_norm=0.0, out_format=None, stream=None):
        """the same on to NULL-first IQ frames: out [n][F][196608] complex float (default) or u8 pairs"""
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        check(lib().dabgpu_tx_bank_transmit_frames(self._h, _ptr(fib_data), _ptr(payload), n_frames, float(freq_norm), _ptr(out), fmt,
                                                   Context._stream(stream)), "dabgpu_tx_bank_transmit_frames")

    def encode_frames_host(self, fib_data, payload, n_frames):
        import numpy as np
        fib = np.ascontiguousarray(fib_data, dtype=np.uint8)
        pay = None if payload is None else np.ascontiguousarray(payload, dtype=np.uint8)
        out = np.empty((self.n, n_frames, NB_FRAME_BITS // 8), np.uint8)
        check(lib().dabgpu_tx_bank_encode_frames_host_sync(self._h, _ptr(fib), _ptr(pay), n_frames, _ptr(out)), "dabgpu_tx_bank_encode_frames_host_sync")
        return out

    def transmit_frames_host(self, fib_data, payload, n_frames, freq_norm=0.0, out_format=None):
        import numpy as np
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        fib = np.ascontiguousarray(fib_data, dtype=np.uint8)
        pay = None if payload is None else np.ascontiguousarray(payload, dtype=np.uint8)
        out = np.empty((self.n, n_frames, NB_FRAME_SAMPLES), np.complex64) if fmt == IQ_FORMATS.index("raw_f32l") else \
            np.empty((self.n, n_frames, 2 * NB_FRAME_SAMPLES), np.uint8)
        check(lib().dabgpu_tx_bank_transmit_frames_host_sync(self._h, _ptr(fib), _ptr(pay), n_frames, float(freq_norm), _ptr(out), fmt),
              "dabgpu_tx_bank_transmit_frames_host_sync")
        return out


def channel_stream(taps=((0, 1.0, 0.0),), cycles_per_sample=0.0, phase0_cycles=0.0, start=0, seed=0, gain=1.0, noise_sigma=0.0,
                   freq_q64=None, phase0_q64=None):
    """a ChannelStream from taps [(delay, re, im), ...] and a carrier offset in cycles per sample (Hz / 2.048e6 for DAB)"""
    P = ChannelStream()
    P.freq_q64 = lib().dabgpu_channel_freq_q64(float(cycles_per_sample)) if freq_q64 is None else int(freq_q64)
    P.phase0_q64 = lib().dabgpu_channel_freq_q64(float(phase0_cycles)) if phase0_q64 is None else int(phase0_q64)
    P.start, P.seed, P.gain, P.noise_sigma, P.n_taps = int(start), int(seed), float(gain), float(noise_sigma), len(taps)
    for k, (d, re, im) in enumerate(taps[:8]):
        P.tap_delay[k], P.tap_re[k], P.tap_im[k] = int(d), float(re), float(im)
    return P


def channel_plan(streams, fading=False):
    """dabgpu_channel_plan (host only): {"halo", "block_samples", "lds_bytes", "staged"} of a list of ChannelStream; raises DabGpuError.
    fading: the geometry of a fading bank (dabgpu_channel_plan_fading: always staged, the grid gains in LDS)"""
    n = len(streams)
    arr = (ChannelStream * n)(*streams) if n else None
    g = ChannelGeometry()
    if fading:
        check(lib().dabgpu_channel_plan_fading(arr, n, C.byref(g)), "dabgpu_channel_plan_fading")
    else:
        check(lib().dabgpu_channel_plan(arr, n, C.byref(g)), "dabgpu_channel_plan")
    return {"halo": g.halo, "block_samples": g.block_samples, "lds_bytes": g.lds_bytes, "staged": g.staged}


def channel_fading_spec(doppler_cycles=0.0, seed=0, kinds=(), rice_k=(), los_cos=()):
    """a ChannelFadingSpec: doppler_cycles = f_D / sample rate (Hz / 2.048e6 for DAB), kinds TAP_STATIC / TAP_FADING per tap, rice_k linear"""
    S = ChannelFadingSpec()
    S.doppler_cycles, S.seed = float(doppler_cycles), int(seed)
    for k, v in enumerate(kinds):
        S.kind[k] = int(v)
    for k, v in enumerate(rice_k):
        S.rice_k[k] = float(v)
    for k, v in enumerate(los_cos):
        S.los_cos[k] = float(v)
    return S


def channel_fading_plan(streams, specs):
    """dabgpu_channel_fading_plan (host only): the fading tables (a ctypes array of ChannelFadingStream) of ChannelStream and
    ChannelFadingSpec lists of one length; raises DabGpuError"""
    n = len(streams)
    assert len(specs) == n
    arr = (ChannelStream * n)(*streams) if n else None
    sp = (ChannelFadingSpec * n)(*specs) if n else None
    out = (ChannelFadingStream * max(n, 1))()
    check(lib().dabgpu_channel_fading_plan(arr, sp, n, out), "dabgpu_channel_fading_plan")
    return out


def channel_fading_gain(table, tap, m0, count):
    """dabgpu_channel_fading_gain_host: g(m) of one tap of a ChannelFadingStream for m0 .. m0 + count - 1, complex64"""
    import numpy as np
    out = np.zeros(count, np.complex64)
    check(lib().dabgpu_channel_fading_gain_host(C.byref(table), int(tap), int(m0), count, _ptr(out)), "dabgpu_channel_fading_gain_host")
    return out


def channel_profile(name):
    """dabgpu_channel_profile: {"taps": [(delay, re, im), ...], "kinds", "rice_k", "los_cos"} of "tu6", "ra6" or "sfn2" (as recalled from
    COST 207, delays in samples at 2.048 MHz); the lists feed channel_stream(taps=...) and channel_fading_spec(...)"""
    P, S = ChannelStream(), ChannelFadingSpec()
    check(lib().dabgpu_channel_profile(name.encode(), C.byref(P), C.byref(S)), "dabgpu_channel_profile")
    n = P.n_taps
    return {"taps": [(P.tap_delay[k], P.tap_re[k], P.tap_im[k]) for k in range(n)], "kinds": list(S.kind[:n]), "rice_k": list(S.rice_k[:n]),
            "los_cos": list(S.los_cos[:n])}


class Channel(_Handle):
    """dabgpu_channel_bank: multipath, carrier offset, timing offset and noise for n streams; the stream position lives on the device.
    fading = the tables of channel_fading_plan: a fading bank (Rayleigh / Rice taps with Doppler)"""
    _destroy = "dabgpu_channel_bank_destroy"

    def __init__(self, ctx, streams, fading=None):
        self._ctx = ctx
        self.n = len(streams)
        self.fading = fading is not None
        self.plan = channel_plan(streams, fading=self.fading)
        arr = (ChannelStream * self.n)(*streams)
        self._h = C.c_void_p()
        if self.fading:
            tab = self._tables(fading)
            check(lib().dabgpu_channel_bank_create_fading(ctx._h, self.n, arr, tab, C.byref(self._h)), "dabgpu_channel_bank_create_fading")
        else:
            check(lib().dabgpu_channel_bank_create(ctx._h, self.n, arr, C.byref(self._h)), "dabgpu_channel_bank_create")

    def _tables(self, fading):
        assert len(fading) >= self.n
        return fading if isinstance(fading, C.Array) else (ChannelFadingStream * self.n)(*fading)

    def set_fading(self, fading, stream=None):
        check(lib().dabgpu_channel_bank_set_fading(self._h, self._tables(fading), Context._stream(stream)), "dabgpu_channel_bank_set_fading")

    def set_params(self, streams, stream=None):
        assert len(streams) == self.n
        arr = (ChannelStream * self.n)(*streams)
        check(lib().dabgpu_channel_bank_set_params(self._h, arr, Context._stream(stream)), "dabgpu_channel_bank_set_params")

    def seek(self, position, stream=None):
        check(lib().dabgpu_channel_bank_seek(self._h, int(position), Context._stream(stream)), "dabgpu_channel_bank_seek")

    def apply(self, d_in, n_in, n_out, d_out, in_stride_samples=0, wrap=False, out_format=None, out_stride_bytes=0, u8_scale=1.0, stream=None):
        """d_in complex float (device) -> d_out rows of n_out samples, complex float (default) or u8 pairs; asynchronous"""
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        check(lib().dabgpu_channel_bank_apply(self._h, _ptr(d_in), in_stride_samples, n_in, int(bool(wrap)), n_out, _ptr(d_out), fmt, out_stride_bytes,
                                              float(u8_scale), Context._stream(stream)), "dabgpu_channel_bank_apply")

    def apply_host(self, h_in, n_out, in_stride_samples=0, wrap=False, out_format=None, u8_scale=1.0):
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        return _host_form(lambda x, n_in, out, stride: check(lib().dabgpu_channel_bank_apply_host_sync(
            self._h, _ptr(x), in_stride_samples, n_in, int(bool(wrap)), n_out, _ptr(out), fmt, stride, float(u8_scale)),
            "dabgpu_channel_bank_apply_host_sync"), h_in, self.n, n_out, fmt)


def interferer_source(kind=INTERFERER_OFF, amp=0.0, cycles_per_sample=0.0, phase0_cycles=0.0, shape=-1, gate_period=0, gate_on=0, gate_offset=0,
                      freq_q64=None, phase0_q64=None):
    """an InterfererSource: a tone at, or a band centred on, cycles_per_sample (Hz / 2.048e6 for DAB); shape = index of a bank's shape, -1 = white;
    the gate in samples (gate_period = 0: always on)"""
    S = InterfererSource()
    S.kind, S.shape, S.amp = int(kind), int(shape), float(amp)
    S.freq_q64 = lib().dabgpu_channel_freq_q64(float(cycles_per_sample)) if freq_q64 is None else int(freq_q64)
    S.phase0_q64 = lib().dabgpu_channel_freq_q64(float(phase0_cycles)) if phase0_q64 is None else int(phase0_q64)
    S.gate_period, S.gate_on, S.gate_offset = int(gate_period), int(gate_on), int(gate_offset)
    return S


def interferer_stream(sources=(), seed=0):
    """an InterfererStream from up to INTERFERER_MAX InterfererSource, in list order"""
    P = InterfererStream()
    P.seed, P.n_sources = int(seed), len(sources)
    for k, S in enumerate(sources[:INTERFERER_MAX]):
        P.source[k] = S
    return P


def interferer_design(width_cycles):
    """dabgpu_interferer_design (host only): the InterfererShape of a flat band width_cycles wide (two-sided, a fraction of the sample rate:
    Hz / 2.048e6 for DAB) with its own figures; raises DabGpuError"""
    H = InterfererShape()
    check(lib().dabgpu_interferer_design(float(width_cycles), C.byref(H)), "dabgpu_interferer_design")
    return H


def interferer_plan(streams, shapes=()):
    """dabgpu_interferer_plan (host only): {"block_samples", "band_slots", "slot_bytes", "lds_bytes"} of a list of InterfererStream against a
    list of InterfererShape; raises DabGpuError"""
    n, ns = len(streams), len(shapes)
    arr = (InterfererStream * n)(*streams) if n else None
    sh = (InterfererShape * ns)(*shapes) if ns else None
    g = InterfererGeometry()
    check(lib().dabgpu_interferer_plan(arr, n, sh, ns, C.byref(g)), "dabgpu_interferer_plan")
    return {"block_samples": g.block_samples, "band_slots": g.band_slots, "slot_bytes": g.slot_bytes, "lds_bytes": g.lds_bytes}


class Interferer(_Handle):
    """dabgpu_interferer_bank: tones, band-limited noise and gated bursts added to n streams; the stream position lives on the device"""
    _destroy = "dabgpu_interferer_bank_destroy"

    def __init__(self, ctx, streams, shapes=()):
        self._ctx = ctx
        self.n = len(streams)
        self.plan = interferer_plan(streams, shapes)
        arr = (InterfererStream * self.n)(*streams)
        sh = (InterfererShape * len(shapes))(*shapes) if len(shapes) else None
        self._h = C.c_void_p()
        check(lib().dabgpu_interferer_bank_create(ctx._h, self.n, arr, sh, len(shapes), C.byref(self._h)), "dabgpu_interferer_bank_create")

    def set_params(self, streams, stream=None):
        assert len(streams) == self.n
        arr = (InterfererStream * self.n)(*streams)
        check(lib().dabgpu_interferer_bank_set_params(self._h, arr, Context._stream(stream)), "dabgpu_interferer_bank_set_params")

    def seek(self, position, stream=None):
        check(lib().dabgpu_interferer_bank_seek(self._h, int(position), Context._stream(stream)), "dabgpu_interferer_bank_seek")

    def apply(self, d_in, n_out, d_out, in_stride_samples=0, out_format=None, out_stride_bytes=0, u8_scale=1.0, stream=None):
        """d_in complex float (device, or None: the interferer alone) -> d_out rows of n_out samples, complex float (default) or u8 pairs;
        d_out may be d_in; asynchronous"""
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        check(lib().dabgpu_interferer_bank_apply(self._h, _ptr(d_in), in_stride_samples, n_out, _ptr(d_out), fmt, out_stride_bytes, float(u8_scale),
                                                 Context._stream(stream)), "dabgpu_interferer_bank_apply")

    def apply_host(self, h_in, n_out, in_stride_samples=0, out_format=None, u8_scale=1.0):
        """h_in [n][>= n_out] complex64 (or [>= n_out] shared with in_stride_samples = 0, or None) -> [n][n_out] complex64 / [n][n_out][2] uint8"""
        import numpy as np
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        if h_in is None:
            sb = 8 if fmt == IQ_FORMATS.index("raw_f32l") else 2
            stride = (n_out * sb + 15) & ~15
            out = np.zeros((self.n, stride), np.uint8)
            check(lib().dabgpu_interferer_bank_apply_host_sync(self._h, None, 0, n_out, _ptr(out), fmt, stride, float(u8_scale)),
                  "dabgpu_interferer_bank_apply_host_sync")
            out = out[:, :n_out * sb]
            return out.copy().view(np.complex64) if sb == 8 else out.reshape(self.n, n_out, 2).copy()
        return _host_form(lambda x, n_in, out, stride: check(lib().dabgpu_interferer_bank_apply_host_sync(
            self._h, _ptr(x), in_stride_samples, n_out, _ptr(out), fmt, stride, float(u8_scale)),
            "dabgpu_interferer_bank_apply_host_sync"), h_in, self.n, n_out, fmt)


def blanker_stream(threshold=None, gap=None, window=None, guard=None, start=0, enabled=True):
    """a BlankerStream: dabgpu_blanker_defaults (threshold 3, gap 8, window 16, guard 1) with the given fields replaced; gap, window and guard
    in blocks of 32 samples"""
    P = lib().dabgpu_blanker_defaults()
    if threshold is not None:
        P.threshold = float(threshold)
    if gap is not None:
        P.gap = int(gap)
    if window is not None:
        P.window = int(window)
    if guard is not None:
        P.guard = int(guard)
    P.start, P.enabled = int(start), int(bool(enabled))
    return P


def blanker_mask_words(n_out):
    """dabgpu_blanker_mask_words: the mask words per stream that a call of n_out samples writes"""
    return int(lib().dabgpu_blanker_mask_words(int(n_out)))


def blanker_plan(streams):
    """dabgpu_blanker_plan (host only): {"reach_blocks", "block_samples", "lds_bytes"} of a list of BlankerStream; raises DabGpuError"""
    n = len(streams)
    arr = (BlankerStream * n)(*streams) if n else None
    g = BlankerGeometry()
    check(lib().dabgpu_blanker_plan(arr, n, C.byref(g)), "dabgpu_blanker_plan")
    return {"reach_blocks": g.reach_blocks, "block_samples": g.block_samples, "lds_bytes": g.lds_bytes}


def blanker_input_needed(stream_params, position, n_out):
    """dabgpu_blanker_input_needed (host only): (first, count), the input indices a call of n_out samples at `position` reads"""
    first, count = C.c_int64(), C.c_uint64()
    check(lib().dabgpu_blanker_input_needed(C.byref(stream_params) if stream_params is not None else None, int(position), int(n_out), C.byref(first),
                                            C.byref(count)), "dabgpu_blanker_input_needed")
    return first.value, count.value


class Blanker(_Handle):
    """dabgpu_blanker_bank: zeroes bursts in n streams ahead of the demodulator; the stream position lives on the device"""
    _destroy = "dabgpu_blanker_bank_destroy"

    def __init__(self, ctx, streams):
        self._ctx = ctx
        self.n = len(streams)
        self.plan = blanker_plan(streams)
        arr = (BlankerStream * self.n)(*streams)
        self._h = C.c_void_p()
        check(lib().dabgpu_blanker_bank_create(ctx._h, self.n, arr, C.byref(self._h)), "dabgpu_blanker_bank_create")

    def set_params(self, streams, stream=None):
        assert len(streams) == self.n
        arr = (BlankerStream * self.n)(*streams)
        check(lib().dabgpu_blanker_bank_set_params(self._h, arr, Context._stream(stream)), "dabgpu_blanker_bank_set_params")

    def seek(self, position, stream=None):
        check(lib().dabgpu_blanker_bank_seek(self._h, int(position), Context._stream(stream)), "dabgpu_blanker_bank_seek")

    def apply(self, d_in, n_in, n_out, d_out, in_stride_samples=0, out_stride_bytes=0, d_mask=None, mask_stride_words=0, stream=None):
        """d_in complex float (device) -> d_out rows of n_out complex float; d_mask (optional): rows of blanker_mask_words(n_out) uint32;
        d_out must not be d_in; asynchronous"""
        check(lib().dabgpu_blanker_bank_apply(self._h, _ptr(d_in), in_stride_samples, n_in, n_out, _ptr(d_out), out_stride_bytes, _ptr(d_mask),
                                              mask_stride_words, Context._stream(stream)), "dabgpu_blanker_bank_apply")

    def apply_host(self, h_in, n_out, in_stride_samples=0, mask=False):
        """h_in [n][n_in] complex64 (or [n_in] shared with in_stride_samples = 0) -> [n][n_out] complex64; mask = True: (that, the mask words
        [n][blanker_mask_words(n_out)] uint32)"""
        import numpy as np
        words = blanker_mask_words(n_out)
        m = np.zeros((self.n, words), np.uint32) if mask else None
        y = _host_form(lambda x, n_in, out, stride: check(lib().dabgpu_blanker_bank_apply_host_sync(
            self._h, _ptr(x), in_stride_samples, n_in, n_out, _ptr(out), stride, _ptr(m), words), "dabgpu_blanker_bank_apply_host_sync"),
            h_in, self.n, n_out, IQ_FORMATS.index("raw_f32l"))
        return (y, m) if mask else y


def iqbal_stream(mode=None, a=None, b=None, c=None, forget=None, min_weight=None):
    """an IqBalanceStream: dabgpu_iqbal_defaults (TRACK, identity, a memory of 16 mode-I frames, min_weight 65536) with the given fields
    replaced; a, b, c complex"""
    P = lib().dabgpu_iqbal_defaults()
    if mode is not None:
        P.mode = int(mode)
    for name, v in (("a", a), ("b", b), ("c", c)):
        if v is not None:
            setattr(P, name + "_re", complex(v).real)
            setattr(P, name + "_im", complex(v).imag)
    if forget is not None:
        P.forget = float(forget)
    if min_weight is not None:
        P.min_weight = float(min_weight)
    return P


def iqbal_plan(streams, max_samples_per_call):
    """dabgpu_iqbal_plan (host only): {"tile_samples", "tiles_per_call", "scratch_bytes"} of a list of IqBalanceStream; raises DabGpuError"""
    n = len(streams)
    arr = (IqBalanceStream * n)(*streams) if n else None
    g = IqBalanceGeometry()
    check(lib().dabgpu_iqbal_plan(arr, n, int(max_samples_per_call), C.byref(g)), "dabgpu_iqbal_plan")
    return {"tile_samples": g.tile_samples, "tiles_per_call": g.tiles_per_call, "scratch_bytes": g.scratch_bytes}


def iqbal_impairment(gain_db, phase_deg, dc=0j):
    """dabgpu_iqbal_impairment: the FIXED IqBalanceStream of a front end with these errors (a = K1, b = K2, c = DC)"""
    P = IqBalanceStream()
    check(lib().dabgpu_iqbal_impairment(float(gain_db), float(phase_deg), complex(dc).real, complex(dc).imag, C.byref(P)), "dabgpu_iqbal_impairment")
    return P


def iqbal_forget(time_constant_samples):
    """dabgpu_iqbal_forget: forget per tile of 1024 samples for a time constant in samples (0.0: not at least one tile)"""
    return float(lib().dabgpu_iqbal_forget(float(time_constant_samples)))


def iqbal_solve_host(stream_params, N, S):
    """dabgpu_iqbal_solve_host: the record (a numpy scalar of IQBAL_RECORD_DTYPE) solved from the state N, S[5]"""
    import numpy as np
    rec = np.zeros(1, np.dtype(IQBAL_RECORD_DTYPE))
    rec["N"], rec["S"] = N, np.asarray(S, np.float32)
    check(lib().dabgpu_iqbal_solve_host(C.byref(stream_params) if stream_params is not None else None, _ptr(rec)), "dabgpu_iqbal_solve_host")
    return rec[0]


class IqBalance(_Handle):
    """dabgpu_iqbal_bank: DC offset and mirror image made (FIXED) or removed blindly (TRACK) in n streams; position and records live on the
    device"""
    _destroy = "dabgpu_iqbal_bank_destroy"

    def __init__(self, ctx, streams, max_samples_per_call):
        self._ctx = ctx
        self.n = len(streams)
        self.plan = iqbal_plan(streams, max_samples_per_call)
        arr = (IqBalanceStream * self.n)(*streams)
        self._h = C.c_void_p()
        check(lib().dabgpu_iqbal_bank_create(ctx._h, self.n, arr, int(max_samples_per_call), C.byref(self._h)), "dabgpu_iqbal_bank_create")

    def set_params(self, streams, stream=None):
        assert len(streams) == self.n
        arr = (IqBalanceStream * self.n)(*streams)
        check(lib().dabgpu_iqbal_bank_set_params(self._h, arr, Context._stream(stream)), "dabgpu_iqbal_bank_set_params")

    def seek(self, position, stream=None):
        check(lib().dabgpu_iqbal_bank_seek(self._h, int(position), Context._stream(stream)), "dabgpu_iqbal_bank_seek")

    def reset(self, stream=None):
        check(lib().dabgpu_iqbal_bank_reset(self._h, Context._stream(stream)), "dabgpu_iqbal_bank_reset")

    def apply(self, d_in, n, d_out=None, flags=IQBAL_APPLY, in_stride_samples=0, out_format=None, out_stride_bytes=0, u8_scale=1.0, stream=None):
        """d_in complex float (device) -> d_out rows of n samples, complex float (default) or u8 pairs (flags with IQBAL_APPLY; d_out may be
        d_in), and / or the call's tiles folded into the records (IQBAL_MEASURE); asynchronous"""
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        check(lib().dabgpu_iqbal_bank_apply(self._h, _ptr(d_in), in_stride_samples, n, _ptr(d_out), fmt, out_stride_bytes, float(u8_scale), int(flags),
                                            Context._stream(stream)), "dabgpu_iqbal_bank_apply")

    def apply_host(self, h_in, n, flags=IQBAL_APPLY, in_stride_samples=0, out_format=None, u8_scale=1.0):
        """h_in [n_streams][>= n] complex64 (or [>= n] shared with in_stride_samples = 0) -> [n_streams][n] complex64 / [n_streams][n][2] uint8;
        None for a MEASURE-only call"""
        import numpy as np
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        if not flags & IQBAL_APPLY:
            x = np.ascontiguousarray(h_in, dtype=np.complex64)
            check(lib().dabgpu_iqbal_bank_apply_host_sync(self._h, _ptr(x), in_stride_samples, n, None, fmt, 0, 1.0, int(flags)),
                  "dabgpu_iqbal_bank_apply_host_sync")
            return None
        return _host_form(lambda x, n_in, out, stride: check(lib().dabgpu_iqbal_bank_apply_host_sync(
            self._h, _ptr(x), in_stride_samples, n, _ptr(out), fmt, stride, float(u8_scale), int(flags)), "dabgpu_iqbal_bank_apply_host_sync"),
            h_in, self.n, n, fmt)

    def read_state(self):
        """the n records as a numpy array of IQBAL_RECORD_DTYPE (waits for the context's stream)"""
        import numpy as np
        rec = np.zeros(self.n, np.dtype(IQBAL_RECORD_DTYPE))
        check(lib().dabgpu_iqbal_bank_read_state_host_sync(self._h, _ptr(rec)), "dabgpu_iqbal_bank_read_state_host_sync")
        return rec

    def read_moments(self, n_tiles):
        """the five sums of the last MEASURE call's first n_tiles tiles, [n_streams][n_tiles][5] float32 (waits for the context's stream)"""
        import numpy as np
        m = np.zeros((self.n, n_tiles, 8), np.float32)
        check(lib().dabgpu_iqbal_bank_read_moments_host_sync(self._h, int(n_tiles), _ptr(m)), "dabgpu_iqbal_bank_read_moments_host_sync")
        return np.ascontiguousarray(m[:, :, :5])


def resample_step(in_rate_hz=2048000.0, out_rate_hz=2048000.0, ppm=0.0):
    """dabgpu_resample_step_q62: in / out * (1 + ppm * 1e-6) as the nearest Q2.62 word (input samples per output sample); 0: not representable"""
    return int(lib().dabgpu_resample_step_q62(float(in_rate_hz), float(out_rate_hz), float(ppm)))


def resample_stream(step_q62=1 << 62, offset=0.0, offset_samples=0, offset_frac_q62=None, gain=1.0):
    """a ResampleStream: step_q62 from resample_step; the offset as offset_samples + a fraction (`offset`, a float in input samples, is split
    into floor and fraction) or as the exact word offset_frac_q62"""
    import math
    P = ResampleStream()
    whole = math.floor(offset)
    P.step_q62 = int(step_q62)
    P.offset_samples = int(offset_samples) + whole
    P.offset_frac_q62 = min(int(round((offset - whole) * 2.0 ** 62)), (1 << 62) - 1) if offset_frac_q62 is None else int(offset_frac_q62)
    P.gain = gain
    return P


def resample_design(max_step=1.0, passband_cycles=0.0):
    """dabgpu_resample_design (host only): a ResampleFilter -- the table for steps up to max_step and the error figures it was found to have"""
    D = ResampleFilter()
    check(lib().dabgpu_resample_design(float(max_step), float(passband_cycles), C.byref(D)), "dabgpu_resample_design")
    return D


def resample_plan(streams, design):
    """dabgpu_resample_plan (host only): {"block_samples", "window_samples", "table_rows", "lds_bytes"}; raises DabGpuError"""
    n = len(streams)
    arr = (ResampleStream * n)(*streams) if n else None
    g = ResampleGeometry()
    check(lib().dabgpu_resample_plan(arr, n, C.byref(design) if design is not None else None, C.byref(g)), "dabgpu_resample_plan")
    return {"block_samples": g.block_samples, "window_samples": g.window_samples, "table_rows": g.table_rows, "lds_bytes": g.lds_bytes}


def resample_input_needed(stream, position, n_out):
    """dabgpu_resample_input_needed: (first, count) of the input indices a call of n_out samples at `position` reads for one stream"""
    first, count = C.c_int64(), C.c_uint64()
    check(lib().dabgpu_resample_input_needed(C.byref(stream), int(position), int(n_out), C.byref(first), C.byref(count)), "dabgpu_resample_input_needed")
    return first.value, count.value


class Resampler(_Handle):
    """dabgpu_resample_bank: arbitrary-ratio, fractional-delay resampling of n streams (a sampling-clock error, a capture rate); the stream
    position lives on the device.  design = None: a table for the largest step of `params` (at least 1), default passband"""
    _destroy = "dabgpu_resample_bank_destroy"

    def __init__(self, ctx, params, design=None):
        self._ctx = ctx
        self.n = len(params)
        if design is None:
            import math
            widest = max([1.0] + [p.step_q62 * 2.0 ** -62 for p in params])               # (a double holds 53 of the word's bits: round up)
            design = resample_design(min(math.nextafter(widest, 4.0), 2.0) if widest > 1.0 else 1.0)
        self.design = design
        self.plan = resample_plan(params, design)
        arr = (ResampleStream * self.n)(*params)
        self._h = C.c_void_p()
        check(lib().dabgpu_resample_bank_create(ctx._h, self.n, arr, C.byref(design), C.byref(self._h)), "dabgpu_resample_bank_create")

    def set_params(self, params, stream=None):
        assert len(params) == self.n
        arr = (ResampleStream * self.n)(*params)
        check(lib().dabgpu_resample_bank_set_params(self._h, arr, Context._stream(stream)), "dabgpu_resample_bank_set_params")

    def seek(self, position, stream=None):
        check(lib().dabgpu_resample_bank_seek(self._h, int(position), Context._stream(stream)), "dabgpu_resample_bank_seek")

    def apply(self, d_in, n_in, n_out, d_out, in_stride_samples=0, wrap=False, out_format=None, out_stride_bytes=0, u8_scale=1.0, stream=None):
        """d_in complex float (device) -> d_out rows of n_out samples, complex float (default) or u8 pairs; asynchronous"""
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        check(lib().dabgpu_resample_bank_apply(self._h, _ptr(d_in), in_stride_samples, n_in, int(bool(wrap)), n_out, _ptr(d_out), fmt, out_stride_bytes,
                                               float(u8_scale), Context._stream(stream)), "dabgpu_resample_bank_apply")

    def apply_host(self, h_in, n_out, in_stride_samples=0, wrap=False, out_format=None, u8_scale=1.0):
        """dabgpu_resample_bank_apply_host_sync: h_in complex64 [n_in] (shared, in_stride_samples = 0) or [n][n_in] with in_stride_samples =
        n_in, on the host -> [n][n_out] complex64, or [n][n_out][2] uint8 for the u8 format; returns when the output is there"""
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        return _host_form(lambda x, n_in, out, stride: check(lib().dabgpu_resample_bank_apply_host_sync(
            self._h, _ptr(x), in_stride_samples, n_in, int(bool(wrap)), n_out, _ptr(out), fmt, stride, float(u8_scale)),
            "dabgpu_resample_bank_apply_host_sync"), h_in, self.n, n_out, fmt)


def channeliser_freq(offset_hz, rate_hz):
    """dabgpu_channeliser_freq_q64: offset / rate (cycles per wideband sample) as the nearest Q64 word; 0 for NaN or outside +- half the rate"""
    return int(lib().dabgpu_channeliser_freq_q64(float(offset_hz), float(rate_hz)))


def channeliser_decim_for(rate_hz):
    """dabgpu_channeliser_decim_for: the largest D <= 8 with rate / D >= 2.048 MHz; 0: none"""
    return int(lib().dabgpu_channeliser_decim_for(float(rate_hz)))


def channeliser_channel(freq_q64=0, phase0_q64=0, gain=1.0, stream=0):
    """a ChanneliserChannel: freq_q64 from channeliser_freq"""
    ch = ChanneliserChannel()
    ch.freq_q64, ch.phase0_q64, ch.gain, ch.stream = int(freq_q64) & ((1 << 64) - 1), int(phase0_q64) & ((1 << 64) - 1), gain, int(stream)
    return ch


def channeliser_design(decim, passband_cycles=0.0, stopband_cycles=0.0):
    """dabgpu_channeliser_design (host only): a ChanneliserFilter -- 72 x decim taps and the error figures the table was found to have"""
    D = ChanneliserFilter()
    check(lib().dabgpu_channeliser_design(int(decim), float(passband_cycles), float(stopband_cycles), C.byref(D)), "dabgpu_channeliser_design")
    return D


def channeliser_plan(channels, n_streams, design, start=0):
    """dabgpu_channeliser_plan (host only): the geometry as a dict; raises DabGpuError"""
    n = len(channels)
    arr = (ChanneliserChannel * n)(*channels) if n else None
    g = ChanneliserGeometry()
    check(lib().dabgpu_channeliser_plan(arr, n, int(n_streams), int(start), C.byref(design) if design is not None else None, C.byref(g)),
          "dabgpu_channeliser_plan")
    return {name: getattr(g, name) for name, _ in ChanneliserGeometry._fields_}


def channeliser_input_needed(decim, position, start, n_out):
    """dabgpu_channeliser_input_needed: (first, count) of the wideband indices a split of n_out samples at `position` reads"""
    first, count = C.c_int64(), C.c_uint64()
    check(lib().dabgpu_channeliser_input_needed(int(decim), int(position), int(start), int(n_out), C.byref(first), C.byref(count)),
          "dabgpu_channeliser_input_needed")
    return first.value, count.value


class Channeliser(_Handle):
    """dabgpu_channeliser_bank: split (wideband streams -> block streams, one row per channel of the list) and combine (block streams -> wideband
    streams); the list is sorted by stream, at most 8 channels per stream; the position lives on the device.  design: a ChanneliserFilter, or
    the decimation (default edges)"""
    _destroy = "dabgpu_channeliser_bank_destroy"

    def __init__(self, ctx, channels, n_streams, design, start=0):
        self._ctx = ctx
        self._h = C.c_void_p()
        self.n_channels, self.n_streams = len(channels), int(n_streams)
        if not isinstance(design, ChanneliserFilter):
            design = channeliser_design(design)
        self.design, self.decim = design, design.decim
        self.plan = channeliser_plan(channels, n_streams, design, start)
        self.start = int(start)
        arr = (ChanneliserChannel * self.n_channels)(*channels)
        check(lib().dabgpu_channeliser_bank_create(ctx._h, arr, self.n_channels, self.n_streams, int(start), C.byref(design), C.byref(self._h)),
              "dabgpu_channeliser_bank_create")

    def set_params(self, channels, start=None, stream=None):
        """replaces the channel list; start = None keeps the bank's `start` (the one of its creation or of the last set_params)"""
        start = self.start if start is None else int(start)
        n = len(channels)
        arr = (ChanneliserChannel * n)(*channels) if n else None
        check(lib().dabgpu_channeliser_bank_set_params(self._h, arr, n, int(start), Context._stream(stream)), "dabgpu_channeliser_bank_set_params")
        self.n_channels, self.start = n, start

    def seek(self, position, stream=None):
        check(lib().dabgpu_channeliser_bank_seek(self._h, int(position), Context._stream(stream)), "dabgpu_channeliser_bank_seek")

    def split(self, d_in, n_in, n_out, d_out, in_stride_samples=0, wrap=False, out_stride_bytes=0, stream=None):
        """d_in wideband complex float (device) -> d_out [n_channels] rows of n_out block samples; asynchronous"""
        check(lib().dabgpu_channeliser_bank_split(self._h, _ptr(d_in), in_stride_samples, n_in, int(bool(wrap)), n_out, _ptr(d_out), out_stride_bytes,
                                                  Context._stream(stream)), "dabgpu_channeliser_bank_split")

    def combine(self, d_in, n_in, n_out, d_out, in_stride_samples=0, wrap=False, out_format=None, out_stride_bytes=0, u8_scale=1.0, stream=None):
        """d_in [n_channels] block rows (device) -> d_out [n_streams] rows of n_out wideband samples, complex float or u8 pairs; asynchronous"""
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        check(lib().dabgpu_channeliser_bank_combine(self._h, _ptr(d_in), in_stride_samples, n_in, int(bool(wrap)), n_out, _ptr(d_out), fmt,
                                                    out_stride_bytes, float(u8_scale), Context._stream(stream)), "dabgpu_channeliser_bank_combine")

    def _host(self, split, h_in, n_out, in_stride_samples, wrap, fmt, u8_scale):
        def call(x, n_in, out, stride):
            if split:
                check(lib().dabgpu_channeliser_bank_split_host_sync(self._h, _ptr(x), in_stride_samples, n_in, int(bool(wrap)), n_out, _ptr(out), stride),
                      "dabgpu_channeliser_bank_split_host_sync")
            else:
                check(lib().dabgpu_channeliser_bank_combine_host_sync(self._h, _ptr(x), in_stride_samples, n_in, int(bool(wrap)), n_out, _ptr(out), fmt, stride,
                                                                      float(u8_scale)), "dabgpu_channeliser_bank_combine_host_sync")
        return _host_form(call, h_in, self.n_channels if split else self.n_streams, n_out, fmt)

    def split_host(self, h_in, n_out, in_stride_samples=0, wrap=False):
        """h_in complex64 [n_in] (shared) or [n_streams][n_in] with in_stride_samples = n_in -> [n_channels][n_out] complex64; returns when done"""
        return self._host(True, h_in, n_out, in_stride_samples, wrap, IQ_FORMATS.index("raw_f32l"), 1.0)

    def combine_host(self, h_in, n_out, in_stride_samples=0, wrap=False, out_format=None, u8_scale=1.0):
        """h_in complex64 [n_channels][n_in] with in_stride_samples = n_in (or one shared row) -> [n_streams][n_out] complex64 / [..][n_out][2] uint8"""
        fmt = IQ_FORMATS.index("raw_f32l") if out_format is None else int(out_format)
        return self._host(False, h_in, n_out, in_stride_samples, wrap, fmt, u8_scale)


def tii_pattern(main_id):
    """T[main_id]: the byte whose bit 7 - b says whether group b carries the transmitter; -1 outside 0..69"""
    return lib().dabgpu_tii_pattern(int(main_id))


def tii_carriers(main_id, sub_id):
    """the 32 carriers (-768 .. 768) of a transmitter, in adjacent pairs"""
    import numpy as np
    out = np.zeros(32, np.int32)
    check(lib().dabgpu_tii_carriers(int(main_id), int(sub_id), _ptr(out)), "dabgpu_tii_carriers")
    return out


def tii_lists(per_frame, n_frames=None):
    """per frame a list of (main_id, sub_id, amp) -> ([n_frames][4] TII_TX_DTYPE, [n_frames] uint8) as the modulator reads them; a list
    longer than TII_MAX_TX keeps its count (and is refused by the library), its first four entries are packed"""
    import numpy as np
    n = len(per_frame) if n_frames is None else n_frames
    lists = np.zeros((n, TII_MAX_TX), np.dtype(TII_TX_DTYPE))
    counts = np.zeros(n, np.uint8)
    for f, txs in enumerate(per_frame):
        counts[f] = len(txs)
        for i, (p, c, amp) in enumerate(txs[:TII_MAX_TX]):
            lists[f, i] = (p, c, 0, amp)
    return lists, counts


def tii_validate(lists, counts):
    check(lib().dabgpu_tii_validate(_ptr(lists), _ptr(counts), len(counts)), "dabgpu_tii_validate")


class TiiBank(_Handle):
    """dabgpu_tii_bank: the TII detector of n receivers; accumulators and frame counts live on the device"""
    _destroy = "dabgpu_tii_bank_destroy"

    def __init__(self, ctx, n, threshold=None):
        self._ctx = ctx
        self.n = int(n)
        cfg = (C.c_float * 2)()
        lib().dabgpu_tii_cfg_default(cfg)
        if threshold is not None:
            cfg[0] = float(threshold)
        self.threshold = cfg[0]
        self._h = C.c_void_p()
        check(lib().dabgpu_tii_bank_create(ctx._h, self.n, cfg, C.byref(self._h)), "dabgpu_tii_bank_create")

    def reset(self, stream=None):
        check(lib().dabgpu_tii_bank_reset(self._h, Context._stream(stream)), "dabgpu_tii_bank_reset")

    def process(self, d_iq, stream_stride_samples, null_offset_samples, states=None, freq_offset=None, decide=False, results=None, counts=None,
                stream=None):
        """one frame of every receiver (asynchronous): results = device [n][24] TII_RECORD_DTYPE, counts = device [n] uint32"""
        check(lib().dabgpu_tii_bank_process(self._h, _ptr(d_iq), stream_stride_samples, null_offset_samples, _ptr(states), _ptr(freq_offset),
                                            int(bool(decide)), _ptr(results), _ptr(counts), Context._stream(stream)), "dabgpu_tii_bank_process")

    def process_host(self, h_iq, null_offset_samples, freq_offset=0.0, fine_time_offset=0, decide=True):
        """one receiver from host memory; returns the records of the decision (None without one)"""
        import numpy as np
        x = np.ascontiguousarray(h_iq, dtype=np.complex64)
        rec = np.zeros(TII_COMBS, np.dtype(TII_RECORD_DTYPE))
        cnt = np.zeros(1, np.uint32)
        check(lib().dabgpu_tii_bank_process_host_sync(self._h, _ptr(x), x.size, null_offset_samples, float(freq_offset), int(fine_time_offset),
                                                      int(bool(decide)), _ptr(rec), _ptr(cnt)), "dabgpu_tii_bank_process_host_sync")
        return rec[:int(cnt[0])] if decide else None

    def read(self, stream=None):
        """(accumulators [n][24][8] float32, frame counts [n]) behind everything queued on the stream"""
        import numpy as np
        acc = np.zeros((self.n, TII_COMBS, TII_GROUPS), np.float32)
        frames = np.zeros(self.n, np.uint32)
        check(lib().dabgpu_tii_bank_read(self._h, _ptr(acc), _ptr(frames), Context._stream(stream)), "dabgpu_tii_bank_read")
        return acc, frames


class DabPlusTx:
    """the DAB+ super-frame encoder (dabgpu_dabplus_tx_*): access units -> the logical frames of DAB+ sub-channels; stateless"""

    def __init__(self, ctx):
        self._ctx = ctx

    @staticmethod
    def layout(frame_bytes, descriptor, au_len):
        """dabgpu_dabplus_superframe_layout (host only) -> (status, au_start[7] or None, num_aus, n_rs)"""
        import numpy as np
        lens = np.zeros(6, np.uint16)
        au_len = np.asarray(au_len, np.uint16).ravel()[:6]
        lens[:au_len.size] = au_len
        start = np.zeros(7, np.uint16)
        na, n_rs = C.c_int(0), C.c_uint32(0)
        st = lib().dabgpu_dabplus_superframe_layout(int(frame_bytes), int(descriptor) & 0xFF, _ptr(lens), _ptr(start), C.byref(na), C.byref(n_rs))
        return st, (start if st == 0 else None), na.value, n_rs.value

    def encode(self, n_streams, n_superframes, au_bytes, au_offsets, au_len, descriptor, frame_bytes, frames, stream_offsets, frame_stride,
               status, stream=None):
        """device buffers: au_offsets uint64 [S][K], au_len uint16 [S][K][6], descriptor uint8 [S][K], frame_bytes uint32 [S], stream_offsets
        uint64 [S], status int32 [S][K]; logical frame 5 k + j of stream s -> frames + stream_offsets[s] + (5 k + j) frame_stride (asynchronous)"""
        check(lib().dabgpu_dabplus_tx_encode(self._ctx._h, n_streams, n_superframes, _ptr(au_bytes), _ptr(au_offsets), _ptr(au_len), _ptr(descriptor),
                                             _ptr(frame_bytes), _ptr(frames), _ptr(stream_offsets), frame_stride, _ptr(status),
                                             Context._stream(stream)), "dabgpu_dabplus_tx_encode")

    def encode_host(self, frame_bytes, superframes):
        """one stream: superframes = [(descriptor, [access-unit payloads]), ...] -> (uint8 [5 K][frame_bytes], int32 status [K])"""
        import numpy as np
        K = len(superframes)
        offs, lens, desc = np.zeros(K, np.uint64), np.zeros((K, 6), np.uint16), np.zeros(K, np.uint8)
        blob, off = [np.zeros(0, np.uint8)], 0
        for k, (d, aus) in enumerate(superframes):
            desc[k], offs[k] = d, off
            for a, p in enumerate(aus[:6]):
                p = np.ascontiguousarray(p, dtype=np.uint8)
                lens[k, a] = p.size
                blob.append(p)
                off += p.size
        au = np.concatenate(blob + [np.zeros(1, np.uint8)])
        frames = np.full((5 * K, int(frame_bytes)), 0xA5, np.uint8)
        status = np.full(K, -1, np.int32)
        check(lib().dabgpu_dabplus_tx_encode_host_sync(self._ctx._h, K, _ptr(au), _ptr(offs), _ptr(lens), _ptr(desc), int(frame_bytes), _ptr(frames),
                                                       _ptr(status)), "dabgpu_dabplus_tx_encode_host_sync")
        return frames, status


def dabplus_tx_offsets(tx_bank, subchannel_indices, n_frames=5):
    """where DabPlusTx.encode writes into a TxBank payload [n][n_frames][4][cif_in_bytes] so that the bank reads the sub-channels' logical frames:
    (stream_offsets uint64 [n * len(subchannel_indices)], ensemble major, frame_stride, frame_bytes uint32 of the same shape).  4 n_frames is a
    multiple of 5 when whole super frames fill the payload (n_frames = 5, n_superframes = 4)."""
    import numpy as np
    cif = tx_bank.cif_in_bytes
    offs = [e * 4 * n_frames * cif + tx_bank.plan["subs"][i].in_offset for e in range(tx_bank.n) for i in subchannel_indices]
    sizes = [tx_bank.plan["subs"][i].in_bytes for _ in range(tx_bank.n) for i in subchannel_indices]
    return np.array(offs, np.uint64), cif, np.array(sizes, np.uint32)


class IngestPipe(_Handle):
    """dabgpu_ingest: ring of pinned host buffers + device twins + a copy stream (include/dabgpu.h)"""
    _destroy = "dabgpu_ingest_destroy"

    def __init__(self, ctx, buffer_bytes, depth=2):
        self._ctx = ctx
        self.bytes = buffer_bytes
        self._h = C.c_void_p()
        check(lib().dabgpu_ingest_create(ctx._h, buffer_bytes, depth, C.byref(self._h)), "dabgpu_ingest_create")

    def acquire(self):
        """-> numpy uint8 view of the next pinned buffer"""
        import numpy as np
        p = C.c_void_p()
        check(lib().dabgpu_ingest_acquire(self._h, C.byref(p)), "dabgpu_ingest_acquire")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(self.bytes,))

    def submit(self, n_bytes):
        """starts the copy of the acquired buffer -> device pointer (int) of its twin"""
        d = C.c_void_p()
        check(lib().dabgpu_ingest_submit(self._h, n_bytes, C.byref(d)), "dabgpu_ingest_submit")
        return d.value

    def wait(self, d_buffer, stream=None):
        check(lib().dabgpu_ingest_wait(self._h, C.c_void_p(d_buffer), Context._stream(stream)), "dabgpu_ingest_wait")

    def consumed(self, d_buffer, stream=None):
        check(lib().dabgpu_ingest_consumed(self._h, C.c_void_p(d_buffer), Context._stream(stream)), "dabgpu_ingest_consumed")


class FrameSession:
    """dabgpu_frame_session: one receiver's frames decoded one batched device call each (FIC + every registered sub-channel), results
    fetched by (generation, FIB group / sub-channel, CIF) -- what the mirror classes use through dabgpu_frame_batcher"""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        L = lib()
        L.dabgpu_frame_session_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.dabgpu_frame_session_destroy.argtypes = [C.c_void_p]
        L.dabgpu_frame_session_destroy.restype = None
        L.dabgpu_frame_session_set_subchannels.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.dabgpu_frame_session_push_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.dabgpu_frame_session_fetch_fib_group.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.dabgpu_frame_session_fetch_cif.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                                     C.POINTER(C.c_uint64)]
        check(L.dabgpu_frame_session_create(C.byref(self._h), device), "dabgpu_frame_session_create")

    def close(self):
        if self._h:
            lib().dabgpu_frame_session_destroy(self._h)
            self._h = C.c_void_p()

    def set_subchannels(self, subchannels):
        n = len(subchannels)
        arr = (SubChannel * n)(*subchannels) if n else None
        check(lib().dabgpu_frame_session_set_subchannels(self._h, arr, n), "dabgpu_frame_session_set_subchannels")

    def push_frame(self, bits, decode_fic=True, tie_rule=0):
        """bits: numpy int8[230400] (host) -> generation number of the frame"""
        import numpy as np
        b = np.ascontiguousarray(bits, dtype=np.int8)
        assert b.size == NB_FRAME_BITS
        gen = C.c_uint64()
        check(lib().dabgpu_frame_session_push_frame(self._h, _ptr(b), int(bool(decode_fic)), tie_rule, C.byref(gen)), "dabgpu_frame_session_push_frame")
        return gen.value

    def fetch_fib_group(self, generation, group):
        """-> (bytes uint8[96], crc_ok_mask, path_error), or None when that generation is gone / was pushed without the FIC"""
        import numpy as np
        out = np.empty(96, dtype=np.uint8)
        m, e = C.c_uint32(), C.c_uint64()
        st = lib().dabgpu_frame_session_fetch_fib_group(self._h, generation, group, _ptr(out), C.byref(m), C.byref(e))
        if st == 4:                                   # DABGPU_ERR_NOT_READY
            return None
        check(st, "dabgpu_frame_session_fetch_fib_group")
        return out, m.value, e.value

    def fetch_cif(self, generation, subchannel, cif, capacity=8192):
        """-> (bytes uint8[n], path_error), or None (generation gone / sub-channel not registered when that frame was pushed)"""
        import numpy as np
        out = np.empty(capacity, dtype=np.uint8)
        n, e = C.c_size_t(), C.c_uint64()
        st = lib().dabgpu_frame_session_fetch_cif(self._h, generation, C.byref(subchannel), cif, _ptr(out), capacity, C.byref(n), C.byref(e))
        if st == 4:
            return None
        check(st, "dabgpu_frame_session_fetch_cif")
        return out[:n.value].copy(), e.value


class DabPlusBank(_Handle):
    """dabgpu_dabplus_bank: n AAC_Frame_Processor states resident on the device"""
    _destroy = "dabgpu_dabplus_bank_destroy"

    def __init__(self, ctx, n_streams):
        self._ctx = ctx
        self.n = n_streams
        self._h = C.c_void_p()
        check(lib().dabgpu_dabplus_bank_create(ctx._h, n_streams, C.byref(self._h)), "dabgpu_dabplus_bank_create")

    def reset(self, stream=None):
        check(lib().dabgpu_dabplus_bank_reset(self._h, Context._stream(stream)), "dabgpu_dabplus_bank_reset")

    def process(self, frames, stream_offsets, frame_stride, frame_bytes, n_frames, superframes, superframe_stride, results,
                max_superframes, counts, stream=None):
        check(lib().dabgpu_dabplus_bank_process(self._h, _ptr(frames), _ptr(stream_offsets), frame_stride, _ptr(frame_bytes),
                                                n_frames, _ptr(superframes), superframe_stride, _ptr(results), max_superframes,
                                                _ptr(counts), Context._stream(stream)), "dabgpu_dabplus_bank_process")

    def process_masked(self, frames, stream_offsets, frame_stride, frame_bytes, n_frames, superframes, superframe_stride, results,
                       max_superframes, counts, active, streams_per_flag, stream=None):
        check(lib().dabgpu_dabplus_bank_process_masked(self._h, _ptr(frames), _ptr(stream_offsets), frame_stride, _ptr(frame_bytes),
                                                       n_frames, _ptr(superframes), superframe_stride, _ptr(results), max_superframes,
                                                       _ptr(counts), _ptr(active), streams_per_flag, Context._stream(stream)),
              "dabgpu_dabplus_bank_process_masked")

    def process_frame_host(self, frame):
        """one-stream bank: -> (superframe_done, firecode_wait_failed, result record, super frame bytes or None)"""
        import numpy as np
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        done, wait = C.c_int(0), C.c_int(0)
        res = np.zeros(1, dtype=np.dtype(SUPERFRAME_RESULT_DTYPE))
        res["rs_failed_index"] = -1                      # the record is only written when a super frame was attempted
        res["au_walk_stopped_at"] = -1
        sf = np.zeros(5 * frame.size, np.uint8)
        check(lib().dabgpu_dabplus_process_frame_host_sync(self._h, _ptr(frame), frame.size, C.byref(done), C.byref(wait), None, _ptr(res),
                                                           _ptr(sf)), "dabgpu_dabplus_process_frame_host_sync")
        return done.value, wait.value, res[0], (sf if done.value else None)


class PacketBank(_Handle):
    """dabgpu_packet_bank: n MSC_Reed_Solomon_Data_Packet_Processor states (packet mode with FEC) resident on the device"""
    _destroy = "dabgpu_packet_bank_destroy"

    def __init__(self, ctx, n_streams):
        self._ctx = ctx
        self.n = n_streams
        self._h = C.c_void_p()
        check(lib().dabgpu_packet_bank_create(ctx._h, n_streams, C.byref(self._h)), "dabgpu_packet_bank_create")

    def reset(self, stream=None):
        check(lib().dabgpu_packet_bank_reset(self._h, Context._stream(stream)), "dabgpu_packet_bank_reset")

    def process(self, frames, stream_offsets, frame_stride, frame_bytes, n_frames, packets, packet_stride, records, max_records, fec_frames,
                max_fec_frames, counts, stream=None):
        """device buffers: stream_offsets uint64 [S], frame_bytes uint32 [S], packets uint8 [S][packet_stride], records PACKET_RECORD_DTYPE
        [S][max_records], fec_frames PACKET_FEC_FRAME_DTYPE [S][max_fec_frames], counts int32 [S][4] (asynchronous)"""
        check(lib().dabgpu_packet_bank_process(self._h, _ptr(frames), _ptr(stream_offsets), frame_stride, _ptr(frame_bytes), n_frames,
                                               _ptr(packets), packet_stride, _ptr(records), max_records, _ptr(fec_frames), max_fec_frames,
                                               _ptr(counts), Context._stream(stream)), "dabgpu_packet_bank_process")

    def process_masked(self, frames, stream_offsets, frame_stride, frame_bytes, n_frames, packets, packet_stride, records, max_records,
                       fec_frames, max_fec_frames, counts, active, streams_per_flag, stream=None):
        check(lib().dabgpu_packet_bank_process_masked(self._h, _ptr(frames), _ptr(stream_offsets), frame_stride, _ptr(frame_bytes), n_frames,
                                                      _ptr(packets), packet_stride, _ptr(records), max_records, _ptr(fec_frames),
                                                      max_fec_frames, _ptr(counts), _ptr(active), streams_per_flag, Context._stream(stream)),
              "dabgpu_packet_bank_process_masked")

    def read_host(self, buf):
        """one-stream bank, one buffer (a logical frame) -> (packets uint8, records, FEC frame records, counts int32 [4])"""
        import numpy as np
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        cap = PACKET_RING_BYTES + buf.size
        max_rec, max_fec = cap // 24 + 1, buf.size // 24 // 9 + 2
        packets = np.zeros(cap, np.uint8)
        rec = np.zeros(max_rec, np.dtype(PACKET_RECORD_DTYPE))
        fec = np.zeros(max_fec, np.dtype(PACKET_FEC_FRAME_DTYPE))
        counts = np.zeros(4, np.int32)
        check(lib().dabgpu_packet_fec_read_host_sync(self._h, _ptr(buf), buf.size, _ptr(packets), _ptr(rec), max_rec, _ptr(fec), max_fec,
                                                     _ptr(counts)), "dabgpu_packet_fec_read_host_sync")
        return packets[:max(int(counts[1]), 0)], rec[:int(counts[0])], fec[:int(counts[2])], counts


def packet_tx_layout(group_len, address, packet_length, frame_bytes, start_byte=0, continuity_index=0, n_fec_frames=1):
    """dabgpu_packet_tx_layout (host only) -> (status, table PACKET_TX_ENTRY_DTYPE [n], frame_first uint32 [n_fec_frames + 1], groups consumed,
    end start_byte, end continuity index); table and frame_first are None when the call is refused"""
    import numpy as np
    lens = np.ascontiguousarray(group_len, dtype=np.uint32).ravel()
    K = max(int(n_fec_frames), 0)
    table = np.zeros(max(PACKET_MAX_FRAME_PACKETS * K, 1), np.dtype(PACKET_TX_ENTRY_DTYPE))
    first = np.zeros(K + 1, np.uint32)
    consumed, end_start, end_ci = C.c_size_t(0), C.c_uint64(int(start_byte)), C.c_uint32(int(continuity_index))
    st = lib().dabgpu_packet_tx_layout(_ptr(lens) if lens.size else None, lens.size, int(address), int(packet_length), int(frame_bytes),
                                       int(start_byte), int(continuity_index), int(n_fec_frames), _ptr(table), PACKET_MAX_FRAME_PACKETS * K,
                                       _ptr(first), C.byref(consumed), C.byref(end_start), C.byref(end_ci))
    if st != 0:
        return st, None, None, 0, int(start_byte), int(continuity_index)
    return 0, table[:int(first[K])], first, consumed.value, end_start.value, end_ci.value


class PacketTx:
    """the packet-mode encoder with FEC (dabgpu_packet_tx_*): data groups -> the logical frames of packet-mode sub-channels; stateless"""

    def __init__(self, ctx):
        self._ctx = ctx

    layout = staticmethod(packet_tx_layout)

    def encode(self, n_streams, n_fec_frames, data, group_offsets, group_base, table, table_stride, frame_first, address, frame_bytes,
               start_byte, frames, stream_offsets, frame_stride, status, stream=None):
        """device buffers: group_offsets uint64 [groups + 1], group_base uint32 [S + 1], table PACKET_TX_ENTRY_DTYPE [S][table_stride],
        frame_first uint32 [S][K + 1], address uint16 [S], frame_bytes uint32 [S], start_byte uint64 [S], stream_offsets uint64 [S], status
        int32 [S][K] (asynchronous)"""
        check(lib().dabgpu_packet_tx_encode(self._ctx._h, n_streams, n_fec_frames, _ptr(data), _ptr(group_offsets), _ptr(group_base), _ptr(table),
                                            table_stride, _ptr(frame_first), _ptr(address), _ptr(frame_bytes), _ptr(start_byte), _ptr(frames),
                                            _ptr(stream_offsets), frame_stride, _ptr(status), Context._stream(stream)), "dabgpu_packet_tx_encode")

    def encode_host(self, groups, address, packet_length, frame_bytes, start_byte=0, continuity_index=0, n_fec_frames=1, fill=0):
        """one stream: lays the groups out and encodes them -> (layout status, uint8 [n_logical_frames][frame_bytes], int32 status [K], groups
        consumed, end start_byte, end continuity index)"""
        import numpy as np
        groups = [np.ascontiguousarray(g, dtype=np.uint8) for g in groups]
        st, table, first, consumed, end_start, end_ci = packet_tx_layout([g.size for g in groups], address, packet_length, frame_bytes, start_byte,
                                                                         continuity_index, n_fec_frames)
        if st != 0:
            return st, None, None, 0, end_start, end_ci
        K = int(n_fec_frames)
        offs = np.zeros(max(len(groups), 1), np.uint64)
        offs[:len(groups)] = np.cumsum([0] + [g.size for g in groups])[:len(groups)]
        data = np.concatenate(groups + [np.zeros(1, np.uint8)])
        n_logical = (int(start_byte) % int(frame_bytes) + K * PACKET_RING_BYTES + int(frame_bytes) - 1) // int(frame_bytes)
        frames = np.full((n_logical, int(frame_bytes)), fill, np.uint8)
        status = np.full(max(K, 1), -1, np.int32)
        check(lib().dabgpu_packet_tx_encode_host_sync(self._ctx._h, K, _ptr(data), data.size - 1, _ptr(offs), len(groups), _ptr(table), _ptr(first),
                                                      int(address), int(frame_bytes), int(start_byte), _ptr(frames), _ptr(status)),
              "dabgpu_packet_tx_encode_host_sync")
        return 0, frames, status[:K], consumed, end_start, end_ci


def packet_tx_offsets(tx_bank, subchannel_indices, n_frames=5):
    """where PacketTx.encode writes into a TxBank payload [n][n_frames][4][cif_in_bytes] so that the bank reads the sub-channels' logical frames:
    (stream_offsets uint64 [n * len(subchannel_indices)], ensemble major, frame_stride, frame_bytes uint32 of the same shape).  4 n_frames logical
    frames of frame_bytes hold the call's FEC frames of 2472 bytes; a trailing partial frame belongs to the next payload."""
    return dabplus_tx_offsets(tx_bank, subchannel_indices, n_frames)


def stream_cfg_default():
    c = StreamCfg()
    lib().dabgpu_stream_cfg_default(C.byref(c))
    return c


def ofdm_params(mode):
    """dict of the geometry of transmission mode 1..4 (host only)"""
    out = (C.c_int * 9)()
    check(lib().dabgpu_get_ofdm_params(int(mode), out), "dabgpu_get_ofdm_params")
    keys = ("nb_frame_symbols", "nb_symbol_period", "nb_null_period", "nb_fft", "nb_cyclic_prefix", "nb_data_carriers",
            "nb_frame_samples", "nb_sym_bits", "nb_frame_bits")
    return dict(zip(keys, list(out)))


def carrier_mapper(mode):
    import numpy as np
    m = np.zeros(ofdm_params(mode)["nb_data_carriers"], np.int32)
    check(lib().dabgpu_get_carrier_mapper(int(mode), _ptr(m)), "dabgpu_get_carrier_mapper")
    return m


def iq_format_from_mode(mode):
    return lib().dabgpu_iq_format_from_mode(mode.encode())


def iq_format_sample_bytes(fmt):
    return int(lib().dabgpu_iq_format_sample_bytes(int(fmt)))


def wav_parse_header(image):
    """host-only: WavHeader of a file image (numpy uint8 / bytes); raises DabGpuError where the reference's reader throws"""
    import numpy as np
    image = np.frombuffer(bytes(image), np.uint8) if isinstance(image, (bytes, bytearray)) else np.ascontiguousarray(image, np.uint8)
    h = WavHeader()
    check(lib().dabgpu_wav_parse_header(_ptr(image), image.size, C.byref(h)), "dabgpu_wav_parse_header")
    return h


def sync_cfg_default():
    c = SyncCfg()
    lib().dabgpu_sync_cfg_default(C.byref(c))
    return c


def soft_cfg_default():
    c = SoftCfg()
    lib().dabgpu_soft_cfg_default(C.byref(c))
    return c


def soft_scale(prs_useful, level=64.0):
    """the scale k of SOFT_CSI from the 2048 useful samples of a frame's phase reference symbol (dabgpu_soft_scale_host)"""
    import numpy as np
    x = np.ascontiguousarray(prs_useful, dtype=np.complex64).reshape(-1)
    if x.size != NB_FFT:
        raise ValueError("soft_scale: 2048 complex samples")
    return float(lib().dabgpu_soft_scale_host(_ptr(x), float(level)))


def diversity_table(branches):
    """a ctypes array of DiversityBranch from DiversityBranch records or (dqpsk, scale[, weight[, sync]]) tuples of buffers / addresses"""
    rows = []
    for b in branches:
        if isinstance(b, DiversityBranch):
            rows.append(b)
            continue
        f = list(b) + [None] * (4 - len(b))
        rows.append(DiversityBranch(*[getattr(_ptr(x), "value", None) for x in f[:4]]))
    return (DiversityBranch * len(rows))(*rows)


def diversity_plan(branches, n_frames, bits, bits_frame_stride=0, bits_layout=BITS_NATURAL, symbols_per_block=0):
    """dabgpu_diversity_plan (host only, nothing is dereferenced): the DiversityGeometry of a diversity_combine call with these arguments;
    DabGpuError with the reason when refused"""
    table = diversity_table(branches)
    g = DiversityGeometry()
    check(lib().dabgpu_diversity_plan(table if len(table) else None, len(table), n_frames, _ptr(bits), bits_frame_stride, int(bits_layout),
                                      int(symbols_per_block), C.byref(g)), "dabgpu_diversity_plan")
    return g


def noise_plan(iq, n_frames, stream_stride_samples, null_offset_samples, states=None, freq_offset=None, noise_power=None, signal_power=None,
               weight=None, snr=None, group_energy=None, valid=None, mode=1):
    """dabgpu_noise_plan (host only, nothing is dereferenced): the NoiseGeometry of a noise_estimate call with these arguments; raises
    DabGpuError with the reason where that call would be refused"""
    g = NoiseGeometry()
    check(lib().dabgpu_noise_plan(int(mode), _ptr(iq), n_frames, stream_stride_samples, null_offset_samples, _ptr(states), _ptr(freq_offset),
                                  _ptr(noise_power), _ptr(signal_power), _ptr(weight), _ptr(snr), _ptr(group_energy), _ptr(valid), C.byref(g)),
          "dabgpu_noise_plan")
    return g


def band_weight_table(band_weights, n_branches, what="band_weights"):
    """a ctypes array of n_branches device addresses from buffers / addresses / None (a branch without a band table)"""
    if len(band_weights) != n_branches:
        raise ValueError(f"{what}: one entry (a buffer or None) per branch")
    return (C.c_void_p * n_branches)(*[getattr(_ptr(x), "value", None) for x in band_weights])


def diversity_plan_symbols(branches, n_frames, bits, band_weights, symbol_weights, bits_frame_stride=0, bits_layout=BITS_NATURAL,
                           symbols_per_block=0):
    """dabgpu_diversity_plan_symbols (host only, nothing is dereferenced): the DiversityGeometry of a diversity_combine call with
    band_weights and symbol_weights (either None: no such table at all); DabGpuError with the reason when refused"""
    table = diversity_table(branches)
    g = DiversityGeometry()
    bands = None if band_weights is None else band_weight_table(band_weights, len(table))
    syms = None if symbol_weights is None else band_weight_table(symbol_weights, len(table), "symbol_weights")
    check(lib().dabgpu_diversity_plan_symbols(table if len(table) else None, len(table), n_frames, _ptr(bits), bits_frame_stride, int(bits_layout),
                                              int(symbols_per_block), bands, syms, C.byref(g)), "dabgpu_diversity_plan_symbols")
    return g


def sym_profile_plan(dqpsk, n_frames, sync=None, symbol_weight=None, symbol_noise=None, ref_noise=None, valid=None, mode=1):
    """dabgpu_sym_profile_plan (host only, nothing is dereferenced): the NoiseGeometry of a sym_profile call with these arguments; raises
    DabGpuError with the reason where that call would be refused"""
    g = NoiseGeometry()
    check(lib().dabgpu_sym_profile_plan(int(mode), _ptr(dqpsk), n_frames, _ptr(sync), _ptr(symbol_weight), _ptr(symbol_noise), _ptr(ref_noise),
                                        _ptr(valid), C.byref(g)), "dabgpu_sym_profile_plan")
    return g


def clock_estimate_plan(dqpsk, n_frames, sync=None, slope_in=None, gain=1.0, slope_out=None, residual=None, corr=None, valid=None, mode=1):
    """dabgpu_clock_estimate_plan (host only, nothing is dereferenced): the NoiseGeometry of a clock_estimate call with these arguments;
    raises DabGpuError with the reason where that call would be refused"""
    g = NoiseGeometry()
    check(lib().dabgpu_clock_estimate_plan(int(mode), _ptr(dqpsk), n_frames, _ptr(sync), _ptr(slope_in), float(gain), _ptr(slope_out), _ptr(residual),
                                           _ptr(corr), _ptr(valid), C.byref(g)), "dabgpu_clock_estimate_plan")
    return g


def clock_derotate_plan(dqpsk_in, dqpsk_out, n_frames, slope, sync=None, symbols_per_block=0, mode=1):
    """dabgpu_clock_derotate_plan (host only, nothing is dereferenced): the DiversityGeometry (run length, runs per frame, grid) of a
    clock_derotate call with these arguments; DabGpuError with the reason when refused"""
    g = DiversityGeometry()
    check(lib().dabgpu_clock_derotate_plan(int(mode), _ptr(dqpsk_in), _ptr(dqpsk_out), n_frames, _ptr(sync), _ptr(slope), int(symbols_per_block),
                                           C.byref(g)), "dabgpu_clock_derotate_plan")
    return g


def clock_slope_q64(ppm):
    """the slope word of a sampling-clock error of ppm: ppm * 1e-6 * 2552 / 2048 cycles per carrier as Q0.64"""
    return lib().dabgpu_clock_slope_q64(float(ppm))


def clock_ppm(slope_q64):
    return lib().dabgpu_clock_ppm(int(slope_q64))


def clock_estimate_host(dqpsk, slope_in=0, gain=1.0):
    """the sampling-clock estimator on the host (no device): one frame's products [75][1536] complex64 -> (new slope word, corr [2], valid)"""
    import numpy as np
    x = np.ascontiguousarray(dqpsk, dtype=np.complex64).reshape(75 * NB_CARRIERS)
    s, corr = C.c_int64(0), np.zeros(2, np.float32)
    st = lib().dabgpu_clock_estimate_host(_ptr(x), int(slope_in), float(gain), C.byref(s), _ptr(corr))
    if st < 0:
        raise DabGpuError("dabgpu_clock_estimate_host: null products or a gain outside (0, 1]")
    return s.value, corr, st


def clock_derotate_host(dqpsk, slope_q64):
    """the de-rotator on the host (no device): one frame's products [75][1536] complex64 -> the products without the ramp of slope_q64"""
    import numpy as np
    x = np.ascontiguousarray(dqpsk, dtype=np.complex64).reshape(75 * NB_CARRIERS)
    out = np.zeros_like(x)
    if lib().dabgpu_clock_derotate_host(_ptr(x), _ptr(out), int(slope_q64)) < 0:
        raise DabGpuError("dabgpu_clock_derotate_host: null products")
    return out.reshape(75, NB_CARRIERS)


def sym_profile_rows_host(dqpsk):
    """the symbol noise profile on the host (no device): one frame's products [75][1536] complex64 -> (symbol weights [75], symbol noise
    [75], reference noise, valid)"""
    import numpy as np
    x = np.ascontiguousarray(dqpsk, dtype=np.complex64).reshape(SYM_PROFILE_SYMBOLS * NB_CARRIERS)
    v, q, ref = np.zeros(SYM_PROFILE_SYMBOLS, np.float32), np.zeros(SYM_PROFILE_SYMBOLS, np.float32), C.c_float(0.0)
    st = lib().dabgpu_sym_profile_rows_host(_ptr(x), _ptr(v), _ptr(q), C.byref(ref))
    if st < 0:
        raise DabGpuError("dabgpu_sym_profile_rows_host: null products")
    return v, q, ref.value, st


def diversity_plan_banded(branches, n_frames, bits, band_weights, bits_frame_stride=0, bits_layout=BITS_NATURAL, symbols_per_block=0):
    """dabgpu_diversity_plan_banded (host only, nothing is dereferenced): the DiversityGeometry of a diversity_combine call with
    band_weights (None: no table at all); DabGpuError with the reason when refused"""
    table = diversity_table(branches)
    g = DiversityGeometry()
    bands = None if band_weights is None else band_weight_table(band_weights, len(table))
    check(lib().dabgpu_diversity_plan_banded(table if len(table) else None, len(table), n_frames, _ptr(bits), bits_frame_stride, int(bits_layout),
                                             int(symbols_per_block), bands, C.byref(g)), "dabgpu_diversity_plan_banded")
    return g


def noise_profile_plan(iq, n_frames, stream_stride_samples, null_offset_samples, states=None, freq_offset=None, exclude=None, profile_in=None,
                       alpha=1.0, profile_out=None, band_weight=None, mean_noise=None, carrier_power=None, valid=None, mode=1):
    """dabgpu_noise_profile_plan (host only, nothing is dereferenced): the NoiseGeometry of a noise_profile call with these arguments; raises
    DabGpuError with the reason where that call would be refused"""
    g = NoiseGeometry()
    check(lib().dabgpu_noise_profile_plan(int(mode), _ptr(iq), n_frames, stream_stride_samples, null_offset_samples, _ptr(states), _ptr(freq_offset),
                                          _ptr(exclude), _ptr(profile_in), float(alpha), _ptr(profile_out), _ptr(band_weight), _ptr(mean_noise),
                                          _ptr(carrier_power), _ptr(valid), C.byref(g)), "dabgpu_noise_profile_plan")
    return g


def noise_profile_exclude(transmitters):
    """the 48 exclusion words of the noise profile from TII ids: `transmitters` = (main_id, sub_id[, ...]) tuples
    (dabgpu_noise_profile_exclude_tii); every carrier of those transmitters is left out of its band"""
    import numpy as np
    main = np.array([int(t[0]) for t in transmitters], np.uint8)
    sub = np.array([int(t[1]) for t in transmitters], np.uint8)
    if any(not 0 <= int(t[0]) < 256 or not 0 <= int(t[1]) < 256 for t in transmitters):
        raise ValueError("noise_profile_exclude: ids must fit a byte")
    out = np.zeros(NOISE_PROFILE_EXCLUDE_WORDS, np.uint32)
    check(lib().dabgpu_noise_profile_exclude_tii(_ptr(main) if main.size else None, _ptr(sub) if sub.size else None, int(main.size), _ptr(out)),
          "dabgpu_noise_profile_exclude_tii")
    return out


def noise_profile_bands_host(carrier_power, exclude=None, profile_in=None, alpha=1.0):
    """steps 2 to 5 of the noise profile on the host: 1536 carrier powers -> (profile [128], band weights [128], mean noise, valid)"""
    import numpy as np
    cp = np.ascontiguousarray(carrier_power, dtype=np.float32).reshape(NB_CARRIERS)
    ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint32).reshape(NOISE_PROFILE_EXCLUDE_WORDS)
    pin = None if profile_in is None else np.ascontiguousarray(profile_in, dtype=np.float32).reshape(NOISE_PROFILE_BANDS)
    prof, bw, mean = np.zeros(NOISE_PROFILE_BANDS, np.float32), np.zeros(NOISE_PROFILE_BANDS, np.float32), C.c_float(0.0)
    st = lib().dabgpu_noise_profile_bands_host(_ptr(cp), _ptr(ex), _ptr(pin), float(alpha), _ptr(prof), _ptr(bw), C.byref(mean))
    if st < 0:
        raise DabGpuError("dabgpu_noise_profile_bands_host: alpha outside (0, 1]")
    return prof, bw, mean.value, st


def dd_profile_plan(dqpsk, n_frames, sync=None, exclude=None, profile_in=None, alpha=1.0, profile_out=None, band_weight=None, mean_noise=None,
                    carrier_noise=None, carrier_amplitude=None, valid=None, mode=1):
    """dabgpu_dd_profile_plan (host only, nothing is dereferenced): the NoiseGeometry of a dd_profile call with these arguments; raises
    DabGpuError with the reason where that call would be refused"""
    g = NoiseGeometry()
    check(lib().dabgpu_dd_profile_plan(int(mode), _ptr(dqpsk), n_frames, _ptr(sync), _ptr(exclude), _ptr(profile_in), float(alpha), _ptr(profile_out),
                                       _ptr(band_weight), _ptr(mean_noise), _ptr(carrier_noise), _ptr(carrier_amplitude), _ptr(valid), C.byref(g)),
          "dabgpu_dd_profile_plan")
    return g


def dd_profile_carriers_host(dqpsk):
    """steps 1 and 2 of the decision-directed noise profile on the host: one frame's products [75][1536] complex64 -> (carrier noise
    [1536], carrier amplitude [1536]); noise_profile_bands_host takes the first from there"""
    import numpy as np
    x = np.ascontiguousarray(dqpsk, dtype=np.complex64).reshape(75 * NB_CARRIERS)
    q, a = np.zeros(NB_CARRIERS, np.float32), np.zeros(NB_CARRIERS, np.float32)
    if lib().dabgpu_dd_profile_carriers_host(_ptr(x), _ptr(q), _ptr(a)) != 0:
        raise DabGpuError("dabgpu_dd_profile_carriers_host: null products")
    return q, a


def diversity_band_mean(band_weight):
    """the branch weight of a band table: dabgpu_diversity_band_mean_host"""
    import numpy as np
    bw = np.ascontiguousarray(band_weight, dtype=np.float32).reshape(NOISE_PROFILE_BANDS)
    return float(lib().dabgpu_diversity_band_mean_host(_ptr(bw)))


def noise_unbias():
    """the calibration constant of the noise estimate: noise_power = floor * noise_unbias()"""
    return float(lib().dabgpu_noise_unbias())


def noise_floor_host(group_energy, signal_power):
    """steps 2 .. 5 of the noise estimate on the host: 192 group energies and the frame power -> a NOISE_RECORD_DTYPE record"""
    import numpy as np
    E = np.ascontiguousarray(group_energy, dtype=np.float32).reshape(TII_COMBS * TII_GROUPS)
    rec = np.zeros(1, np.dtype(NOISE_RECORD_DTYPE))
    lib().dabgpu_noise_floor_host(_ptr(E), float(signal_power), _ptr(rec))
    return rec[0]


def diversity_scale(scales, weights=None, valid=None):
    """(k, live mask) of one frame from its branches' scales, weights (None: 1) and sync flags (None: valid): dabgpu_diversity_scale_host"""
    import numpy as np
    k = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32).reshape(k.size)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.int32).reshape(k.size)
    mask = C.c_uint32(0)
    out = lib().dabgpu_diversity_scale_host(_ptr(k), _ptr(w), _ptr(v), int(k.size), C.byref(mask))
    return float(out), mask.value


def subchannel_plan(sc):
    """(pi[], l[], n_decoded_bytes) of a SubChannel via the product's host tables"""
    pi = (C.c_int * 4)()
    lx = (C.c_int * 4)()
    nb = C.c_int(0)
    n = lib().dabgpu_subchannel_plan(C.byref(sc), pi, lx, C.byref(nb))
    if n < 0:
        raise DabGpuError("invalid sub-channel protection profile")
    return list(pi)[:n], list(lx)[:n], nb.value


def ber_plan(subchannels, n_ensembles, history_frames, ensemble_stride, out_ensemble_stride, bits_layout=BITS_NATURAL):
    """dabgpu_ber_plan (host only): the BerGeometry of a ber_frames call with these arguments; DabGpuError with the reason when refused"""
    n = len(subchannels)
    arr = (SubChannel * n)(*subchannels) if n else None
    g = BerGeometry()
    check(lib().dabgpu_ber_plan(arr, n, n_ensembles, history_frames, ensemble_stride, out_ensemble_stride, int(bits_layout), C.byref(g)),
          "dabgpu_ber_plan")
    return g


def tx_encode_plan(subchannels):
    """dabgpu_tx_encode_plan (host only): dict with `subs` (TxSubPlan per sub-channel), `fic` (the FIB group's), `cif_in_bytes`,
    `ring_slot_dwords` and `sched` = uint32 array [n][2] of (out_bit, keep_mask)"""
    import numpy as np
    n = len(subchannels)
    arr = (SubChannel * n)(*subchannels) if n else None
    plans = (TxSubPlan * (n + 1))()
    cif_in, ring, n_sched = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
    check(lib().dabgpu_tx_encode_plan(arr, n, plans, C.byref(cif_in), None, 0, C.byref(n_sched), C.byref(ring)), "dabgpu_tx_encode_plan")
    sched = np.zeros((n_sched.value, 2), np.uint32)
    check(lib().dabgpu_tx_encode_plan(arr, n, plans, None, _ptr(sched), n_sched.value, None, None), "dabgpu_tx_encode_plan")
    return dict(subs=[plans[i] for i in range(n)], fic=plans[n], cif_in_bytes=cif_in.value, ring_slot_dwords=ring.value, sched=sched)
