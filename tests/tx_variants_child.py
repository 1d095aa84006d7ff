"""Child process of tests/test_gpu_ofdm_modulator_variants.py: for each transmission mode asked for, modulates N_FRAMES frames in each of
the eight (output format, payload layout, frequency shift) combinations through the asynchronous entry point and writes one .npy per
mode and combination: the whole device buffer as bytes, GUARD bytes of pattern in front of d_out and GUARD behind it included.

    python tx_variants_child.py SYMBOLS_PER_RUN SEED_BASE OUT_DIR MODE[,MODE...]

The symbols per run of the transmitter kernels are a launch decision that libdabgpu reads once per process (DABGPU_TX_SPB); the parent
sets it in this process's environment, which is why every run length is a process of its own (the modes that share a run length share
the process: starting the runtime is most of a child's life).  Device memory comes from the HIP runtime directly (hipMalloc / hipMemcpy
through ctypes): importing torch would double that life again.
Exit status 0 = everything written; 2 = a refused call or a HIP error (message on stderr)."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_FRAMES = 2
GUARD = 4096                                   # bytes of pattern on either side of d_out (a multiple of 16: d_out stays 16-byte aligned)
FUZZ_STRIDE = 1000003                          # tests/conftest.py: DAB_FUZZ_OFFSET shifts every integer seed by k x this
MODE_SYMBOLS = {1: 76, 2: 76, 3: 153, 4: 76}


def guard_pattern():
    return ((np.arange(GUARD, dtype=np.uint64) * 2654435761 >> 7) & 0xFF).astype(np.uint8)


def payloads(seed, n_bytes):
    """[N_FRAMES][n_bytes] uint8; the parent calls this too (there numpy's generator is already shifted under DAB_FUZZ_OFFSET)"""
    return np.random.default_rng(int(seed)).integers(0, 256, (N_FRAMES, n_bytes), dtype=np.uint8)


def combinations():
    """(name, output format is u8, payload layout, shifted) in a fixed order"""
    return [(f"{'u8' if u8 else 'f32'}_{'bits' if layout else 'ref'}_{'pll' if pll else 'plain'}", u8, layout, pll)
            for u8 in (False, True) for layout in (0, 1) for pll in (False, True)]


class Hip:
    """the four runtime calls this script needs, from the libamdhip64 that libdabgpu.so has already brought into the process"""

    def __init__(self):
        path = None
        with open("/proc/self/maps") as maps:
            for line in maps:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        if path is None:
            raise RuntimeError("libamdhip64 is not loaded (load libdabgpu.so first)")
        self.lib = C.CDLL(path)
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipGetErrorString.restype = C.c_char_p

    def ck(self, status, what):
        if status != 0:
            raise RuntimeError(f"{what}: {self.lib.hipGetErrorString(status).decode()}")

    def malloc(self, n_bytes):
        p = C.c_void_p()
        self.ck(self.lib.hipMalloc(C.byref(p), max(int(n_bytes), 16)), "hipMalloc")
        return p.value

    def upload(self, dst, host):
        host = np.ascontiguousarray(host)
        self.ck(self.lib.hipMemcpy(dst, host.ctypes.data, host.nbytes, 1), "hipMemcpy to the device")

    def download(self, src, n_bytes):
        out = np.empty(int(n_bytes), np.uint8)
        self.ck(self.lib.hipMemcpy(out.ctypes.data, src, out.nbytes, 2), "hipMemcpy to the host")    # (synchronises with the null stream)
        return out

    def free(self, p):
        self.lib.hipFree(p)


def seed_of(seed_base, mode):
    return int(seed_base) + mode


def file_name(mode, name):
    return f"mode{mode}_{name}.npy"


def main(argv):
    spb, seed_base, out_dir, modes = int(argv[1]), int(argv[2]), argv[3], [int(m) for m in argv[4].split(",")]
    assert int(os.environ.get("DABGPU_TX_SPB", "0")) == spb, "the parent sets DABGPU_TX_SPB to the run length it asks for"
    seed_base += FUZZ_STRIDE * int(os.environ.get("DAB_FUZZ_OFFSET", "0") or 0)
    for p in (ROOT, os.path.join(ROOT, "dab-radio_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import dabgpu
    import tx_model as TX
    f32, u8 = dabgpu.IQ_FORMATS.index("raw_f32l"), dabgpu.IQ_FORMATS.index("raw_u8")
    ctx = dabgpu.Context(0)
    hip = Hip()
    pattern = guard_pattern()
    for mode in modes:
        g = dabgpu.ofdm_params(mode)
        S, n_bytes = g["nb_frame_samples"], g["nb_frame_bits"] // 8
        assert g["nb_frame_symbols"] == MODE_SYMBOLS[mode]
        pay = payloads(seed_of(seed_base, mode), n_bytes)
        d_pay = hip.malloc(pay.nbytes)
        hip.upload(d_pay, pay)
        for name, is_u8, layout, pll in combinations():
            out_bytes = N_FRAMES * S * (2 if is_u8 else 8)
            host = np.full(2 * GUARD + out_bytes, 0xA5, np.uint8)      # (0xA5: no stale result can stand in for a sample that was not written)
            host[:GUARD] = pattern
            host[GUARD + out_bytes:] = pattern
            d_buf = hip.malloc(host.nbytes)
            assert d_buf % 16 == 0
            hip.upload(d_buf, host)
            ctx.ofdm_modulate_frames(mode, d_pay, N_FRAMES, d_buf + GUARD, layout=layout, out_format=u8 if is_u8 else f32,
                                     freq_norm=float(TX.SERIES_SHIFT) if pll else 0.0, stream=0)
            ctx.synchronize(stream=0)
            np.save(os.path.join(out_dir, file_name(mode, name)), hip.download(d_buf, host.nbytes))
            hip.free(d_buf)
        hip.free(d_pay)
    ctx.close()
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main(sys.argv))
    except Exception as e:                                              # a refused call or a HIP error: say which, exit 2
        sys.stderr.write(f"tx_variants_child: {type(e).__name__}: {e}\n")
        sys.exit(2)
