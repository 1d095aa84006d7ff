"""-m gpu: the packet-mode mirror classes (dab-radio_amd/host/dab/msc/msc_reed_solomon_data_packet_processor.h, dab/tx/dab_packet_encoder.h)
through tests/cpp/packet_fec_harness.cpp: MSC_Reed_Solomon_Data_Packet_Processor fed the committed sequences hands its callback the
reference's log in content and order and returns the reference's (= the model's) ReadPacket values; DAB_Packet_Encoder's frames are the
model's, block by block."""
import os
import subprocess

import numpy as np
import pytest

import packet_fec_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "packet_fec_harness")


@pytest.fixture(scope="module")
def env():
    if not os.path.exists(HARNESS):
        import __graft_entry__ as g
        g.build()
    e = dict(os.environ)
    e["LD_LIBRARY_PATH"] = os.path.join(ROOT, "dab-radio_amd") + ":/opt/rocm/lib:" + e.get("LD_LIBRARY_PATH", "")
    return e


def test_mirror_class_equals_the_reference_log(env, tmp_path):
    v = np.load(os.path.join(ROOT, "tests", "golden", "packet_fec_vectors.npz"))
    names = [str(n) for n in v["names"]]
    # every situation, the long layout sequence left to the bank tests (a launch per packet here)
    for name in ("clean_mixed", "errors_9_plus", "fec_length_field", "data_length_shorter", "uncorrectable_row0_wrong_header", "pop_into_fec_region",
                 "counter_repeated", "starts_mid_frame_discards", "ends_in_1_byte", "ends_in_truncated_packet"):
        i = names.index(name)
        lens = v[f"buf_len_{i}"]
        ends = np.cumsum(lens)
        bufs = [v[f"buf_{i}"][e - n:e] for n, e in zip(lens, ends)]
        (tmp_path / "in.bin").write_bytes(np.uint32(len(bufs)).tobytes() + b"".join(np.uint32(len(b)).tobytes() + b.tobytes() for b in bufs))
        res = subprocess.run([HARNESS, "rx", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, env=env, timeout=300)
        assert res.returncode == 0, res.stderr.decode()[-2000:]
        raw = np.fromfile(tmp_path / "out.bin", np.uint8)
        n_ret = int(raw[:4].view("<u4")[0])
        rets = raw[4:4 + 4 * n_ret].view("<u4")
        n_cb, n_log = (int(x) for x in raw[4 + 4 * n_ret:12 + 4 * n_ret].view("<u4"))
        log = raw[12 + 4 * n_ret:]
        assert log.size == n_log
        proc, model_rets = M.Processor(), []
        for b in bufs:
            model_rets += proc.read_buffer(b)
        assert rets.tolist() == model_rets == [int(r) for r in v[f"ret_{i}"]], name
        assert n_cb == int(v[f"n_cb_{i}"]) and np.array_equal(log, v[f"log_{i}"]), name


def test_encoder_class_equals_the_model_block_by_block(env, tmp_path):
    rng = np.random.default_rng(8300)
    address, length, fb = 0x0F3, 72, 168
    blocks = [(2, [int(x) for x in rng.integers(0, 600, 14)]), (1, [int(x) for x in rng.integers(0, 300, 3)]), (3, [0, 1, 8191])]
    groups_all = []
    blob = np.array([address, length, fb, len(blocks)], np.uint32).tobytes()
    for k, lens in blocks:
        gs = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
        groups_all += gs
        blob += np.array([k, len(gs)], np.uint32).tobytes() + b"".join(np.uint32(len(g)).tobytes() + g.tobytes() for g in gs)
    (tmp_path / "in.bin").write_bytes(blob)
    res = subprocess.run([HARNESS, "tx", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    n = int(raw[:4].view("<u4")[0])
    frames, total = raw[4:4 + n], int(raw[4 + n:8 + n].view("<u4")[0])
    # the model, block by block with the same carry-over of groups, start byte and continuity index
    start, ci, taken, stream, offered = 0, 0, 0, [], 0
    for k, lens in blocks:
        offered += len(lens)
        pending = groups_all[taken:offered]
        st, ent, first, consumed, start2, ci = M.layout([len(g) for g in pending], address, length, fb, start, ci, k)
        assert st == 0
        stream.append(M.encode(pending, ent, first, address))
        taken, start = taken + consumed, start2
    s = np.concatenate(stream)
    exp = np.zeros((s.size + fb - 1) // fb * fb, np.uint8)
    exp[:s.size] = s
    assert total == taken and taken >= len(groups_all) - 1
    assert np.array_equal(frames, exp)
    res = M.run_frames(list(exp.reshape(-1, fb)))
    assert all(f["rs_count"] == [0] * 12 for f in res["fec_frames"]) and len(res["fec_frames"]) == 6
    ra = M.Reassembler(address)
    ra.last_ci = 3
    assert ra.feed(res["packets"], res["records"]) == [bytes(g) for g in groups_all[:taken]]
