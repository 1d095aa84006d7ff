"""CPU: the channel BER planner (dabgpu_ber_plan, plain C++ in dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal in the order
include/dabgpu.h states, the edges (no sub-channel, 64 of them, a sub-channel ending at CU 864, UEP rows whose code word is shorter than
their capacity units, the sub-channel that fills the CIF), the launch record against dabgpu_tx_encode_plan, and a stand-alone fuzz program
(tests/cpp/ber_plan_fuzz.cpp, its own main) built with -fsanitize=address,undefined and run directly."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
FRAME = 230400


@pytest.fixture(scope="module")
def dabgpu():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


def eep(dabgpu, start, length, level=2, typ=0):
    return dabgpu.SubChannel(start, length, 0, 0, level, typ)


def refused(dabgpu, match, *args, **kw):
    with pytest.raises(dabgpu.DabGpuError, match=match):
        dabgpu.ber_plan(*args, **kw)


def test_every_refusal_in_its_order(dabgpu):
    good = [eep(dabgpu, 0, 48), eep(dabgpu, 48, 48)]
    nb = 4 * sum(dabgpu.subchannel_plan(s)[2] for s in good)
    assert dabgpu.ber_plan(good, 3, 5, 5 * FRAME, nb).codewords_per_ensemble == 12
    # each call is wrong in everything that is checked AFTER the refusal it expects
    # 1. the sub-channel count (more than 64), before any descriptor is looked at
    many = [eep(dabgpu, 13 * k, 6) for k in range(64)] + [eep(dabgpu, 900, 6)]
    refused(dabgpu, r"65 sub-channels", many, 0, 4, 7, 1, bits_layout=9)
    assert dabgpu.lib().dabgpu_ber_plan(None, 1, 1, 5, 5 * FRAME, 0, 0, dabgpu.C.byref(dabgpu.BerGeometry())) == 2
    # 2. what the decoders refuse, in list order
    bad_profile, outside = dabgpu.SubChannel(0, 48, 1, 64, 0, 0), eep(dabgpu, 840, 48)
    L = dabgpu.lib()
    for subs in ([bad_profile, outside], [outside, bad_profile], [good[0], dabgpu.SubChannel(100, 64, 1, 34, 0, 0)]):
        first_bad = next(s for s in subs if L.dabgpu_subchannel_validate(dabgpu.C.byref(s)) != 0)
        assert L.dabgpu_subchannel_validate(dabgpu.C.byref(first_bad)) == 2
        reason = L.dabgpu_last_error().decode()
        with pytest.raises(dabgpu.DabGpuError) as e:
            dabgpu.ber_plan(subs, 0, 4, 7, 1, bits_layout=9)
        assert reason and reason in str(e.value)
    # 3. what the encoder's plan refuses: two sub-channels that overlap
    refused(dabgpu, r"overlaps", [eep(dabgpu, 0, 48), eep(dabgpu, 40, 48)], 0, 4, 7, 1, bits_layout=9)
    # 4. the ensemble count
    refused(dabgpu, r"0 ensembles", good, 0, 4, 7, 1, bits_layout=9)
    refused(dabgpu, r"1048577 ensembles", good, (1 << 20) + 1, 4, 7, 1, bits_layout=9)
    # 5. the layout
    refused(dabgpu, r"unknown bits_layout 9", good, 1, 4, 7, 1, bits_layout=9)
    refused(dabgpu, r"unknown bits_layout -1", good, 1, 4, 7, 1, bits_layout=-1)
    # 6. the history
    refused(dabgpu, r"history_frames 4", good, 1, 4, 7, 1)
    refused(dabgpu, r"history_frames -3", good, 1, -3, 7, 1)
    # 7. the ring's stride: too small, not a multiple of 16
    refused(dabgpu, r"ensemble_stride", good, 1, 5, 5 * FRAME - 16, 1)
    refused(dabgpu, r"ensemble_stride", good, 1, 5, 5 * FRAME + 8, 1)
    refused(dabgpu, r"ensemble_stride", good, 1, 6, 5 * FRAME, 1)
    # 8. the output stride: too small, not a multiple of 4
    refused(dabgpu, r"out_ensemble_stride", good, 1, 5, 5 * FRAME, nb - 4)
    refused(dabgpu, r"out_ensemble_stride", good, 1, 5, 5 * FRAME, nb + 2)
    assert dabgpu.ber_plan(good, 1 << 20, 5, 5 * FRAME + 16, nb + 4, bits_layout=1).grid == (1 << 20) * 12 // 4
    assert dabgpu.lib().dabgpu_ber_plan(None, 0, 1, 5, 5 * FRAME, 0, 0, None) == 2


def check_against_the_encoder_plan(dabgpu, subs, n_ens=7):
    tx = dabgpu.tx_encode_plan(subs)
    g = dabgpu.ber_plan(subs, n_ens, 5, 5 * FRAME, 4 * tx["cif_in_bytes"])
    plans = tx["subs"] + [tx["fic"]]
    assert g.n_sub == len(subs) and g.codewords_per_ensemble == 4 * len(subs) + 4 and g.cif_bytes == tx["cif_in_bytes"]
    assert g.n_sched == len(tx["sched"]) and [g.sched_offset[i] for i in range(len(plans))] == [p.sched_offset for p in plans]
    assert g.max_kept_bits == max(p.kept_bits for p in plans)
    assert g.lds_bytes == 64 * ((max(p.length for p in plans) + 7) // 8)
    assert g.waves_per_block == 4 and g.block_threads == 256 and g.grid == (n_ens * g.codewords_per_ensemble + 3) // 4
    return g, plans


def test_edges(dabgpu):
    # FIC only: the FIB group's 2304 bits in 5 blocks of 512
    g, plans = check_against_the_encoder_plan(dabgpu, [])
    assert g.codewords_per_ensemble == 4 and g.lds_bytes == 320 and g.max_kept_bits == 2304 and g.cif_bytes == 0 and g.grid == 7
    assert dabgpu.ber_plan([], 1, 5, 5 * FRAME, 0).grid == 1           # (no output stride to check without sub-channels)
    # 64 sub-channels, the last ending at CU 864
    subs = [eep(dabgpu, 13 * k, 6) for k in range(63)] + [eep(dabgpu, 858, 6)]
    g, plans = check_against_the_encoder_plan(dabgpu, subs)
    assert g.codewords_per_ensemble == 260 and len(set(g.sched_offset[i] for i in range(64))) == 1 and g.lds_bytes == 320
    # UEP rows whose code word is shorter than their capacity units
    for row, length, kept in ((4, 35, 2236), (13, 52, 3320), (63, 416, 26616)):
        g, plans = check_against_the_encoder_plan(dabgpu, [dabgpu.SubChannel(3, length, 1, row, 0, 0)])
        assert plans[0].kept_bits == kept < 64 * length and g.max_kept_bits == max(kept, 2304) and g.lds_bytes == 64 * ((length + 7) // 8)
    # the sub-channel that fills the CIF: 6912 bytes of LDS per code word
    g, plans = check_against_the_encoder_plan(dabgpu, [eep(dabgpu, 0, 864, 3, 0)], n_ens=1)
    assert g.lds_bytes == 6912 and g.max_kept_bits == 55296 and g.grid == 2
    g, plans = check_against_the_encoder_plan(dabgpu, [eep(dabgpu, 0, 864, 0, 0)], n_ens=1)
    assert g.lds_bytes == 6912 and g.max_kept_bits == 55296


def test_fuzz_program_under_sanitizers(tmp_path):
    exe = tmp_path / "ber_plan_fuzz"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "ber_plan_fuzz.cpp"),
                    os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)], check=True, timeout=600)
    res = subprocess.run([str(exe), "20000", "7800"], capture_output=True, timeout=600)
    assert res.returncode == 0, (res.stdout.decode()[-500:], res.stderr.decode()[-3000:])
    out = json.loads(res.stdout.decode().strip().splitlines()[-1])
    assert out["failed_checks"] == 0 and out["iterations"] == 20000 and out["accepted"] > 1000
