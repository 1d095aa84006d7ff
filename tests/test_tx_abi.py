"""CPU: the OFDM transmitter's C ABI -- declared, exported, listed in dabgpu.ABI_SYMBOLS -- and its argument checks, which run before
any device call (no GPU needed)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dabgpu_ofdm_modulate_frames", "dabgpu_ofdm_modulate_frames_host_sync")
INVALID_ARG = 2


@pytest.fixture(scope="module")
def dabgpu():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


def test_entries_declared_exported_and_listed(dabgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dabgpu.h")).read(), flags=re.S)
    assert "DABGPU_TX_PAYLOAD_REFERENCE = 0" in text and "DABGPU_TX_PAYLOAD_FRAME_BITS = 1" in text
    L = dabgpu.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(L, name)
        assert name in dabgpu.ABI_SYMBOLS
    assert L.dabgpu_abi_version() == 4
    assert (dabgpu.TX_PAYLOAD_REFERENCE, dabgpu.TX_PAYLOAD_FRAME_BITS) == (0, 1)


def test_bad_arguments_fail_before_the_device(dabgpu):
    L = dabgpu.lib()
    F32, U8, S16 = (dabgpu.IQ_FORMATS.index(k) for k in ("raw_f32l", "raw_u8", "raw_s16l"))
    pay = np.zeros(28800, np.uint8)
    out = np.zeros(2 * 196608 + 8, np.float32)
    fake = 0x1000                                                  # never dereferenced: every call below fails its argument check
    cases = [
        (None, 1, fake, 0, 1, F32),          # NULL context
        (fake, 0, fake, 0, 1, F32),          # no mode 0
        (fake, 5, fake, 0, 1, F32),          # no mode 5
        (fake, 1, fake, 2, 1, F32),          # no layout 2
        (fake, 1, fake, 0, 1, S16),          # complex float and u8 only
        (fake, 1, None, 0, 1, U8),           # NULL payload
    ]
    for ctx, mode, p, layout, n, fmt in cases:
        assert L.dabgpu_ofdm_modulate_frames(ctx, mode, p, layout, n, None, 0.0, fake, fmt, None) == INVALID_ARG, (mode, layout, fmt)
        assert L.dabgpu_ofdm_modulate_frames_host_sync(ctx, mode, pay.ctypes.data if p else None, layout, n, None, 0.0,
                                                       out.ctypes.data, fmt) == INVALID_ARG, (mode, layout, fmt)
    # NULL output with frames to write
    assert L.dabgpu_ofdm_modulate_frames(fake, 1, fake, 0, 1, None, 0.0, None, F32, None) == INVALID_ARG
    assert L.dabgpu_ofdm_modulate_frames_host_sync(fake, 1, pay.ctypes.data, 0, 1, None, 0.0, None, U8) == INVALID_ARG
    assert b"output" in L.dabgpu_last_error()
