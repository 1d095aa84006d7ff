"""Large device buffers of which a test touches little (tests/test_gpu_addressing_*.py).

big(n) allocates lead + n bytes with torch.empty -- nothing fills them -- and returns the view that starts `lead` bytes in.  The lead
is there so that an offset which a kernel truncated to uint32_t, or sign-extended from int32_t, still lands INSIDE the allocation: the
wrap then shows as wrong bytes or a damaged canary, not as a fault.  A case writes only the regions it names: inputs, and canaries
(0xC3, the pattern of test_gpu_tx_encode.py) around every output region and at the low addresses where a wrapped write would land.
Everything is compared on the device or after copying the named regions alone."""
import numpy as np
import pytest

GIB = 1 << 30
WRAP = 1 << 32
LEAD = 1 << 31
CANARY = 0xC3
CANARY_BYTES = 4096
MAX_HELD = 12 * GIB            # what one test may hold at once


def need(n_bytes):
    """skip (with both numbers) where the device has less free memory than the case needs; a case never asks for more than MAX_HELD"""
    import torch
    assert n_bytes <= MAX_HELD + GIB // 2, f"a case may hold about 12 GiB, this one asks for {n_bytes}"
    free, _total = torch.cuda.mem_get_info()
    if free < n_bytes + GIB // 4:
        pytest.skip(f"device memory: {free} bytes free, {n_bytes} needed")


def big(n_bytes, lead=LEAD):
    """uint8 view of n_bytes that starts `lead` bytes into an untouched allocation of lead + n_bytes"""
    import torch
    need(lead + n_bytes)
    return torch.empty(lead + n_bytes, dtype=torch.uint8, device="cuda")[lead:]


def region(view, off, n):
    """n bytes at byte offset `off` of a view big() returned; off may be negative, down to -lead"""
    base = view._base if view._base is not None else view
    a = view.storage_offset() + off
    assert 0 <= a and a + n <= base.numel(), (off, n)
    return base[a:a + n]


def put(view, off, array):
    """host array (any dtype) -> bytes at `off`"""
    import torch
    h = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    region(view, off, h.size).copy_(torch.from_numpy(h).cuda())


def get(view, off, n, dtype=np.uint8):
    return region(view, off, n).cpu().numpy().view(dtype)


def wrap_offsets(off):
    """where a write meant for `off` >= 2^32 lands when its offset went through 32 bits: off mod 2^32 (uint32_t), and that value read
    as int32_t where it is negative (off - 2^32 for offsets below 2^33 is the first of the two)"""
    low = off % WRAP
    return [low] + ([low - WRAP] if low >= (1 << 31) else [])


class Canaries:
    """canary runs of CANARY_BYTES: set them before the call, check() after it"""

    def __init__(self):
        self.runs = []

    def at(self, view, off, n=CANARY_BYTES, lead=LEAD):
        if off < -lead:
            return
        r = region(view, off, n)
        r.fill_(CANARY)
        self.runs.append((r, off))

    def around(self, view, off, n, gap=CANARY_BYTES):
        """before and behind the output region [off, off + n)"""
        self.at(view, off - gap, gap)
        self.at(view, off + n, gap)

    def wrapped(self, view, off):
        """at the low addresses a 32-bit offset would make of `off`"""
        if off >= WRAP:
            for w in wrap_offsets(off):
                self.at(view, w)

    def check(self):
        for r, off in self.runs:
            assert bool((r == CANARY).all()), f"canary at offset {off} damaged"


def release():
    """hand the memory back once the caller has `del`ed its names"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
