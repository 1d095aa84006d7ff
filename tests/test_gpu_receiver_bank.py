"""-m gpu: the receiver bank (dab-radio_amd/csrc/receiver_bank.hip + receiver_bank_sched.cpp) driven through the C ABI in the orders the synchroniser, frame,
synchroniser, frame tests (tests/test_gpu_receiver.py, the mirror harness) never take: frames posted BACK TO BACK with no synchroniser in between -- up to
R - 1 = 7 of them, which dabgpu_receiver_submit_frame allows -- by one member and by several members at once, under the bank's knobs, and with display views
asked of one frame among them.  A member uploads frame g into buffer g % RX_BANK_IQ_FRAMES of its own on a stream that waits for nothing; with two buffers
the third post overwrote the first frame's samples before its round had read them, and that frame came back with a neighbour's bits.

Every case: three ordinary cycles (stage, synchroniser, record, frame) put three different frames into the receiver's three staging buffers and bring the
record up; one more synchroniser; then K dabgpu_receiver_submit_frame calls in a row with nothing written in between -- post k reads staging buffer
(cur + k) % 3 as it stands.  Expected for every generation: the oracle's composition (OracleReceiver of tests/test_gpu_receiver.py) over the same samples
in the same order -- soft bits, the fine-frequency word (carried from frame to frame) and the total phase as uint32 patterns, four FIB groups with CRC mask
and path error, every CIF's bytes and path error once the de-interleaver has filled.  Second witness: private receivers of the same process given the same
calls must deliver the same bytes.

The bank is a singleton of its process and reads DABGPU_BANK_* when it is made: the device part of a case runs in ONE fresh interpreter (this file as a
script) under subprocess.run(timeout=...), so a bank that hangs ends its test and not the session; it is not tried again.  The child only drives the
device and writes down what came back; the expectations and every comparison are made here, once per member, and shared by the cases."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "dab-radio_amd"), os.path.join(ROOT, "oracle"), ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_gpu_receiver import Frame, OracleReceiver, _api, assert_frame, fetch_frame   # noqa: E402,F401  (Frame: what fetch_frame fills)

LEAD = 30000                                   # make_ensemble_stream's lead-in with timing_pad 0: the first NULL symbol starts here
SUBS = ((0, 48, False, 0, 2, 0), (100, 58, True, 29, 0, 0))          # start, length, UEP?, UEP row, EEP level, EEP type: the two of tests/test_gpu_receiver.py
# seed, carrier offset (cycles / sample), where the receiver believes the frame starts relative to where it does: every member its own stream
MEMBERS = ((41, 1.9e-3, -63), (42, -2.3e-3, 41), (43, 0.7e-3, 99), (44, 1.2e-3, -20), (45, -1.1e-3, 7))
CYCLES = 3                                     # ordinary cycles in front: the three staging buffers then hold frames 0, 1, 2 and `cur` is 0 again
NOT_READY = 4
NULL, FRAME = 2656, 196608                     # mode I: samples of the NULL symbol, of a transmission frame


def _subs(O):
    return [O.subchannel(s[0], s[1], is_uep=True, uep_index=s[3]) if s[2] else O.subchannel(s[0], s[1], eep_level=s[4], eep_type=s[5]) for s in SUBS]


def _stage_of(stream, j, toff, cap):
    """the staging buffer of frame j: NULL | frame j as the receiver cuts them, the PRS `toff` samples before where it expects it"""
    stage = np.zeros(cap, np.complex64)
    seg = stream[LEAD + j * FRAME - toff:][:cap]
    stage[:seg.size] = seg
    return stage


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the child: device work only
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _child(spec_path, out_path):
    import dabgpu
    with open(spec_path, "rb") as f:
        spec = pickle.load(f)
    L = _api(dabgpu)
    L.dabgpu_receiver_create_banked.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    ck = lambda st, what: dabgpu.check(st, what)               # noqa: E731
    cfg = dabgpu.sync_cfg_default()
    K, views_at = spec["K"], spec["views_at"]
    streams = {m: np.load(p) for m, p in spec["streams"].items()}
    dsubs = (dabgpu.SubChannel * len(SUBS))(*[dabgpu.SubChannel(*s) for s in SUBS])

    class Rx:
        pass

    def make(form, member):
        r = Rx()
        r.form, r.member, r.h = form, member, C.c_void_p()
        if form == "banked":
            ck(L.dabgpu_receiver_create_banked(C.byref(r.h), 0), "dabgpu_receiver_create_banked")
        else:
            ck(L.dabgpu_receiver_create(C.byref(r.h), 0, 1, None, None), "dabgpu_receiver_create")
        ck(L.dabgpu_receiver_set_subchannels(r.h, dsubs, len(SUBS), 1), "dabgpu_receiver_set_subchannels")
        r.ses = L.dabgpu_receiver_session(r.h)
        r.syncs, r.frames, r.post_us, r.eighth, r.fft, r.cap = [], {}, [], None, None, 0
        return r

    def sync(r):
        ck(L.dabgpu_receiver_submit_sync(r.h, C.byref(cfg), NULL), "dabgpu_receiver_submit_sync")
        rec = dabgpu.SyncState()
        ck(L.dabgpu_receiver_wait_sync(r.h, C.byref(rec), None, None), "dabgpu_receiver_wait_sync")
        r.syncs.append((rec.sync_valid, rec.fine_time_offset, int(np.float32(rec.freq_coarse).view(np.uint32)), int(np.float32(rec.freq_fine).view(np.uint32))))
        return rec.fine_time_offset

    def post(r, off, want_views=0):
        gen = C.c_uint64()
        ck(L.dabgpu_receiver_submit_frame(r.h, NULL + off, cfg.fine_freq_update_beta, want_views, 0, C.byref(gen)), "dabgpu_receiver_submit_frame")
        return gen.value

    def warm_up(r):
        toff = MEMBERS[r.member][2]
        for j in range(CYCLES):
            h, cap = C.c_void_p(), C.c_size_t()
            ck(L.dabgpu_receiver_stage(r.h, C.byref(h), C.byref(cap)), "dabgpu_receiver_stage")
            r.cap = cap.value
            stage = np.ctypeslib.as_array(C.cast(h, C.POINTER(C.c_float)), shape=(2 * cap.value,)).view(np.complex64)
            stage[:] = _stage_of(streams[r.member], j, toff, cap.value)
            off = sync(r)
            assert post(r, off) == j
            r.frames[j] = fetch_frame(L, ck, r.h, r.ses, j, dsubs)
        r.off = sync(r)

    def collect(r):
        for k in range(K):
            g = CYCLES + k
            r.frames[g] = fetch_frame(L, ck, r.h, r.ses, g, dsubs)
            if k == views_at:
                n = 77 * 2048 * 2
                r.fft = np.ctypeslib.as_array(C.cast(r.frames[g]["fft_ptr"], C.POINTER(C.c_float)), shape=(n,)).copy()

    group = {}
    try:
        # the private receivers first, one after the other (nothing of theirs is under way when the bank's members post)
        group["private"] = [make("private", m) for m in spec["members"]]
        for r in group["private"]:
            warm_up(r)
            for k in range(K):
                assert post(r, r.off, 1 if k == views_at else 0) == CYCLES + k
            collect(r)
        # the bank's members: the posts interleaved member by member, nothing between them; collected after the last post
        group["banked"] = [make("banked", m) for m in spec["members"]]
        for r in group["banked"]:
            warm_up(r)
        t0 = time.perf_counter()
        for k in range(K):
            for r in group["banked"]:
                assert post(r, r.off, 1 if k == views_at else 0) == CYCLES + k
                r.post_us.append((time.perf_counter() - t0) * 1e6)
        if spec["eighth"]:
            for r in group["banked"]:
                r.eighth = L.dabgpu_receiver_submit_frame(r.h, NULL + r.off, cfg.fine_freq_update_beta, 0, 0, None)
                r.post_us.append((time.perf_counter() - t0) * 1e6)
        for r in group["banked"]:
            collect(r)
        out = [dict(form=r.form, member=r.member, cap=r.cap, syncs=r.syncs, frames=r.frames, post_us=r.post_us, eighth=r.eighth, fft=r.fft)
               for rs in group.values() for r in rs]
    finally:
        for rs in group.values():
            for r in rs:
                L.dabgpu_receiver_destroy(r.h)
    with open(out_path, "wb") as f:
        pickle.dump(out, f)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the tests: expectations once per member, a child per case, the comparisons
# ------------------------------------------------------------------------------------------------------------------------------------------------------
K_MAX = 7
VIEWS_AT = 1                                   # the views case: the middle one of three back-to-back frames


class _Expected:
    """member -> its stream (a file the children read) and the oracle's answers for CYCLES ordinary frames, a synchroniser, K_MAX frames back to back"""

    def __init__(self, O, directory):
        self.O, self.dir, self.subs, self.by_member = O, directory, _subs(O), {}
        self.cap = O.NB_NULL_PERIOD + (2048 - 504) + O.NB_FRAME_SAMPLES

    def member(self, m):
        if m not in self.by_member:
            import stream_model as SM
            O = self.O
            seed, cfo, toff = MEMBERS[m]
            stream, _ = SM.make_ensemble_stream(O, CYCLES, self.subs, seed=seed, cfo=cfo, timing_pad=0, noise=2.0, amplitude=1.0)
            path = os.path.join(self.dir, f"member{m}.npy")
            np.save(path, stream)
            stages = [_stage_of(stream, j, toff, self.cap) for j in range(CYCLES)]
            orx = OracleReceiver(O, self.subs)
            syncs, frames = [], []

            def sync(stage):
                ok, off, _ = orx.sync(stage)
                assert ok and off == toff, (m, off)
                syncs.append((1, off, int(np.float32(orx.st.freq_coarse).view(np.uint32)), int(np.float32(orx.st.freq_fine).view(np.uint32))))
            for j in range(CYCLES):
                sync(stages[j])
                frames.append(orx.frame(stages[j], toff))
            sync(stages[0])
            for k in range(K_MAX):
                frames.append(orx.frame(stages[k % CYCLES], toff, want_fft=(k == VIEWS_AT)))
            self.by_member[m] = dict(path=path, syncs=syncs, frames=frames)
        return self.by_member[m]


@pytest.fixture(scope="module")
def expected(oracle, tmp_path_factory):
    return _Expected(oracle, str(tmp_path_factory.mktemp("bank_streams")))


def _run_child(tmp_path, expected, members, K, views_at=None, eighth=False, env=None):
    spec = dict(members=list(members), K=K, views_at=views_at, eighth=eighth, streams={m: expected.member(m)["path"] for m in members})
    spec_path, out_path = str(tmp_path / "spec.pkl"), str(tmp_path / "out.pkl")
    with open(spec_path, "wb") as f:
        pickle.dump(spec, f)
    # what the child does: starts an interpreter, loads the library and the device runtime (the bulk: tens of seconds at the worst on a busy machine), makes
    # 2 receivers per member (~20 page-locked allocations each), runs CYCLES + K frames of a few ms on each, reads its streams and writes ~0.3 MB per frame
    timeout = 60 + 10 * len(members) + 1 * 2 * len(members) * (CYCLES + K)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), spec_path, out_path]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
    with open(out_path, "rb") as f:
        return pickle.load(f)


def _closest(bits, frames):
    """which expected generation a delivered frame's soft bits are nearest to: (generation, share of equal bytes)"""
    share = [float(np.mean(bits == e["bits"])) for e in frames]
    g = int(np.argmax(share))
    return g, round(share[g], 4)


def _check(out, expected, members, K, views_at=None):
    by = {(r["form"], r["member"]): r for r in out}
    assert sorted(by) == sorted((f, m) for f in ("banked", "private") for m in members)
    for m in members:
        e = expected.member(m)
        frames = e["frames"][:CYCLES + K]
        # the K frames posted back to back are K different frames: one delivered with another's samples cannot pass for its own
        for a in range(CYCLES, CYCLES + K):
            for b in range(a + 1, CYCLES + K):
                assert not np.array_equal(frames[a]["bits"], frames[b]["bits"]), (a, b)
        for form in ("banked", "private"):
            r = by[(form, m)]
            assert r["cap"] == expected.cap
            assert r["syncs"] == e["syncs"], (form, m, r["syncs"], e["syncs"])
            wrong = {g: _closest(r["frames"][g]["bits"], frames) for g in range(CYCLES + K) if not np.array_equal(r["frames"][g]["bits"], frames[g]["bits"])}
            print(f"{form} member {m}, K = {K}: posts at us {[round(t) for t in r['post_us']]}; generations with another frame's soft bits -> (nearest expected generation, "
                  f"share of equal bytes): {wrong}")
            assert not wrong, (form, m, K, wrong)
            for g in range(CYCLES + K):
                assert_frame(r["frames"][g], frames[g], g)
        # the second witness: a private receiver given the same calls
        b, p = by[("banked", m)], by[("private", m)]
        for g in range(CYCLES + K):
            fb, fp = b["frames"][g], p["frames"][g]
            assert np.array_equal(fb["bits"], fp["bits"]) and fb["fine"].view(np.uint32) == fp["fine"].view(np.uint32) and fb["total"].view(np.uint32) == fp["total"].view(np.uint32), (m, g)
            for grp in range(4):
                assert np.array_equal(fb["fib"][grp][0], fp["fib"][grp][0]) and fb["fib"][grp][1:] == fp["fib"][grp][1:], (m, g, grp)
            for c in range(4):
                for si in range(len(SUBS)):
                    if frames[g]["msc"][c][si] is not None:
                        assert np.array_equal(fb["msc"][c][si][0], fp["msc"][c][si][0]) and fb["msc"][c][si][1] == fp["msc"][c][si][1], (m, g, c, si)
        if views_at is not None:
            want = np.ascontiguousarray(frames[CYCLES + views_at]["fft"]).view(np.uint32)
            for form in ("banked", "private"):
                assert np.array_equal(by[(form, m)]["fft"].view(np.uint32), want), (form, m, "fft of the frame that asked for views")


@pytest.mark.parametrize("K", [2, 3, 5, 7])
def test_one_member_posts_frames_back_to_back(tmp_path, expected, K):
    """Case 1.  K = 7 is all that post_frame accepts with none delivered: the eighth post is answered DABGPU_ERR_NOT_READY and changes nothing of the seven.
    (The bank counts frames not yet DELIVERED: the eighth post must arrive before the first round is handed out.  Measured: the eight posts take 0.25 ms --
    a post returns once the upload two frames back has left its staging buffer --, and the first round is not even formed before the worker's 4 x 50 us look
    for a synchroniser behind the frame have passed, then costs its ~25 runtime calls, the demodulation and a decode.)
    With two sample buffers per member the device gave, counting from the first back-to-back post: K = 2 right; K = 3: frame 0 a mixture of its own samples
    and frame 2's (73 % of its soft bits equal frame 2's), frames 1 and 2 off through the fine-frequency word it left (94 % and 99 % their own); K = 5 all five
    wrong; K = 7: frames 1 to 5 wrong, frame 4 with the soft bits expected of frame 6 (share of equal bytes 1.0000)."""
    out = _run_child(tmp_path, expected, [0], K, eighth=(K == 7))
    if K == 7:
        eighth = [r["eighth"] for r in out if r["form"] == "banked"]
        print("the eighth post's status:", eighth)
    _check(out, expected, [0], K)
    if K == 7:
        assert eighth == [NOT_READY], eighth


@pytest.mark.parametrize("n", [2, 5])
def test_members_post_back_to_back_interleaved(tmp_path, expected, n):
    """Case 2.  n members, each on its own stream (seed, carrier offset, timing); after its synchroniser each posts 4 frames, the posts interleaved member by
    member; default knobs.  Every member's frames are its own oracle's and its private receiver's."""
    out = _run_child(tmp_path, expected, list(range(n)), 4)
    _check(out, expected, list(range(n)), 4)


@pytest.mark.parametrize("knobs", [{"DABGPU_BANK_ROUNDS": "1", "DABGPU_BANK_GATHER_US": "0"}, {"DABGPU_BANK_ROUNDS": "8"}], ids=["rounds1_gather0", "rounds8"])
def test_back_to_back_frames_under_the_banks_knobs(tmp_path, expected, knobs):
    """Case 3.  Case 1 with K = 7 under the two settings tests/test_gpu_cpp_mirror.py runs the bank with: the same bytes under both"""
    out = _run_child(tmp_path, expected, [0], 7, env=knobs)
    _check(out, expected, [0], 7)


def test_views_of_the_middle_frame_of_three(tmp_path, expected):
    """Case 4.  K = 3 with want_views = 1 on the middle frame only (its round runs the demodulator once more over the batch row for the display buffers): that
    frame's fft equals oracle.demod_frame(want_fft=True) as uint32 patterns, and the frames on either side are what they are without it"""
    out = _run_child(tmp_path, expected, [0], 3, views_at=VIEWS_AT)
    _check(out, expected, [0], 3, views_at=VIEWS_AT)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
