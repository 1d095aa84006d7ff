"""Shared by the device tests of the channel BER (not a test module): the two configurations of tests/test_gpu_ber.py, their random
inputs -- int8 rings with 0, +-127 and -128 among the values, random "decoded" bytes -- and the model's records (tests/ber_model.py),
computed once per (configuration, history, seed) and left unchanged."""
import numpy as np

import ber_model as M
import tx_encode_cases as T

CONFIG_A = [dict(start=1, length=4, is_uep=0, uep_index=0, eep_level=3, eep_type=0),
            dict(start=5, length=6, is_uep=0, uep_index=0, eep_level=2, eep_type=0),
            dict(start=12, length=18, is_uep=0, uep_index=0, eep_level=2, eep_type=1),
            dict(start=31, length=35, is_uep=1, uep_index=4, eep_level=0, eep_type=0),
            dict(start=101, length=6, is_uep=0, uep_index=0, eep_level=2, eep_type=0),
            dict(start=816, length=48, is_uep=0, uep_index=0, eep_level=2, eep_type=0)]
CONFIG_B = [dict(start=0, length=864, is_uep=0, uep_index=0, eep_level=3, eep_type=0)]
CONFIGS = {"A": (CONFIG_A, 3), "B": (CONFIG_B, 1)}


def random_ring(rng, n_ens, H):
    r = rng.integers(-128, 128, (n_ens, H, M.FRAME_BITS), dtype=np.int64).astype(np.int8)
    pick = rng.integers(0, 20, r.shape)
    r[pick == 0] = 0
    r[pick == 1] = 0
    r[pick == 2] = 127
    r[pick == 3] = -127
    r[pick == 4] = -128
    return r


class Case:
    """random inputs of a configuration and the model's records, computed once per (configuration, history, seed)"""
    cache = {}

    def __init__(self, oracle, name, H, seed):
        dicts, self.n_ens = CONFIGS[name]
        self.dicts, self.H = dicts, H
        self.osubs = [T.o_sub(oracle, d) for d in dicts]
        self.nb = sum(oracle.subchannel_plan(s)[2] for s in self.osubs)
        rng = np.random.default_rng(seed)
        self.ring = random_ring(rng, self.n_ens, H)
        self.fib = rng.integers(0, 256, (self.n_ens, 4, 96), dtype=np.uint8)
        self.msc = rng.integers(0, 256, (self.n_ens, 4, self.nb), dtype=np.uint8)
        self.oracle = oracle
        self.models = {}

    @classmethod
    def get(cls, oracle, name, H, seed=8100):
        key = (name, H, seed)
        if key not in cls.cache:
            cls.cache[key] = cls(oracle, name, H, seed)
        return cls.cache[key]

    def model(self, slots):
        """slots: newest slot per ensemble -> (fic [n][4], msc [n][4][n_sub])"""
        fic = np.zeros((self.n_ens, 4), M.BER_DTYPE)
        msc = np.zeros((self.n_ens, 4, len(self.osubs)), M.BER_DTYPE)
        for e, sl in enumerate(slots):
            if (e, sl) not in self.models:
                self.models[(e, sl)] = M.ber_frames(self.oracle, self.ring[e], sl, self.osubs, self.fib[e], self.msc[e])
            fic[e], msc[e] = self.models[(e, sl)]
        return fic, msc

    def device(self, dabgpu, torch, layout):
        ring = M.to_classed(self.ring) if layout == dabgpu.BITS_MSC_CLASSED else self.ring
        return (torch.from_numpy(ring).cuda(), torch.from_numpy(self.fib).cuda(), torch.from_numpy(self.msc).cuda(),
                [T.g_sub(dabgpu, d) for d in self.dicts])


def records(torch, *shape):
    return torch.full(tuple(shape) + (16,), 0xA5, dtype=torch.uint8, device="cuda")


def as_records(t):
    return t.cpu().numpy().view(M.BER_DTYPE).reshape(t.shape[:-1])
