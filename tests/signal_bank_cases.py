"""What the -m gpu tests of the signal-path banks (channel, fading channel, resampler, channeliser) share: the host form called three times
on ONE bank, so that both of its grow-only device buffers are first allocated, then outgrown, then larger than the call needs; and the life
of a Python handle."""
import gc

import numpy as np

GUARD = 0xA5
# (n_in or None for the whole input, n_out, wrap, u8 output).  The input buffer is sized by n_in and the output buffer by n_out: 64 in and 7
# out allocate both; the whole input and 2049 out, across a tile edge of every kernel, outgrow both; 101 out of the whole input fits both
HOST_CALLS = ((64, 7, True, False), (None, 2049, False, False), (None, 101, True, True))
HOST_TOTAL = sum(c[1] for c in HOST_CALLS)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def host_form_regrowth(host_sync, model, x, rows, f32, u8=None):
    """x [rows in][n_in] complex64, of which a call takes the first samples of every row (contiguous, rows n_in apart);
    host_sync(x, n_out, wrap, fmt, out, stride_bytes): the bank's *_host_sync entry point into `out`, rows of stride_bytes;
    model(x, pos, n_out, wrap, fmt): what the host model expects from position pos; u8 = None: the third call is complex float too.
    The caller's rows are 40 bytes wider than the samples and keep the guard pattern there.  -> the position reached"""
    pos = 0
    for n_in, n_out, wrap, small in HOST_CALLS:
        xc = x if n_in is None else np.ascontiguousarray(x[:, :n_in])
        fmt = u8 if small and u8 is not None else f32
        sb = 8 if fmt == f32 else 2
        stride = n_out * sb + 40
        out = np.full((rows, stride), GUARD, np.uint8)
        host_sync(xc, n_out, wrap, fmt, out, stride)
        assert np.all(out[:, n_out * sb:] == GUARD), f"call of {n_out}: bytes behind a row were written"
        data = np.ascontiguousarray(out[:, :n_out * sb])
        got = data.view(np.complex64) if sb == 8 else data.reshape(rows, n_out, 2)
        assert same_bits(got, model(xc, pos, n_out, wrap, fmt)), f"call of {n_out} at position {pos}"
        pos += n_out
    return pos


def handle_lifecycle(make):
    """make() -> a new object of a handle-owning class: close() twice, the closed handle is falsy; an unclosed one goes with its last
    reference (__del__ swallows exceptions, so that half only shows a crash)"""
    a = make()
    assert a._h
    a.close()
    assert not a._h
    a.close()
    assert not a._h
    b = make()
    assert b._h
    del b
    gc.collect()
