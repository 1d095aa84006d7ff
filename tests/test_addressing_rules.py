"""The host rule that keeps the lane and octet Viterbi mappings away from rings whose offsets do not fit 32 bits (no GPU).

The decode planner (choose_lane_subchannels) and the generic batch (uniform_batch) used to word the rule differently:
`hist_frames * 230400 < 2^32` against `(n_slots / cifs + 1) * frame_stride + cifs * cif_stride < 2^32`.  Both were safe, but they
disagreed: the planner let rings of up to 18641 frames through to the lanes, the generic batch only up to 18639.  They are one function
now, dabgpu_host_ring_fits_lanes, and it states the kernel's real reach.

The reach.  vit_prep_kernel (viterbi_lanes.hip) forms in uint32_t, per lane,
    aoff = fr * frame_stride + ci * cif_stride            fr = slot / cifs_per_frame, ci = slot - fr * cifs_per_frame
    aoff += (lane & 15) * (cif_stride >> 4)               class-order rows only
with slot in [0, n_slots), and then reads src[(size_t)aoff + (i >> ish)]: the bit's index inside the row is added in 64 bits.  So
the largest 32-bit value is reached in the last frame, the last CIF of a frame and class 15:
    max = ((n_slots - 1) / cifs) * frame_stride + (cifs - 1) * cif_stride + 15 * (cif_stride / 16)
For a decode call's ring of H frames (n_slots = 4 H, strides 230400 and 55296): (H - 1) * 230400 + 165888 + 51840, which is
4 294 873 728 < 2^32 at H = 18641 and 4 295 104 128 >= 2^32 at H = 18642.  (vit_prep_ring4_kernel and vit_prep_ring4c_kernel, which
the decode calls use on aligned rings, widen every term to size_t; they are held to the same rule.)

kernel_reach() below and the closed forms in these tests restate that expression from a reading of viterbi_lanes.hip:382-388; nothing
here parses the kernel.  An edit of vit_prep_kernel that changes what goes into aoff (the 9216 FIC bytes, say) would pass this file and
is caught only on the device, by the H = 18641 cases of tests/test_gpu_addressing_ring.py."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
AUTO, WAVE, LANE, OCTET = 0, 1, 2, 3
FRAME, CIF = 230400, 55296
SIZES = [18640, 18641, 18642, 18643]


def kernel_reach(n_slots, cifs, frame_stride, cif_stride, classed):
    """the largest aoff of vit_prep_kernel, by running its expression over every slot of the top frames in 64 bits"""
    slot = np.arange(max(0, n_slots - 4 * cifs), n_slots, dtype=np.uint64)
    fr = slot // np.uint64(cifs)
    ci = slot - fr * np.uint64(cifs)
    aoff = fr * np.uint64(frame_stride) + ci * np.uint64(cif_stride)
    if classed:
        aoff = aoff[:, None] + np.arange(16, dtype=np.uint64)[None, :] * np.uint64(cif_stride >> 4)
    return int(aoff.max())


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("addressing") / "addressing_rules_driver"
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "addressing_rules_driver.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]

    def run(*args):
        out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-2000:]
        return [json.loads(line) for line in out.stdout.strip().splitlines()]
    return run


def test_the_derived_reach_is_the_kernel_expression():
    for H in SIZES + [5, 16]:
        for classed in (False, True):
            closed = (H - 1) * FRAME + 3 * CIF + (15 * (CIF // 16) if classed else 0)
            assert kernel_reach(4 * H, 4, FRAME, CIF, classed) == closed
    assert (18641 - 1) * FRAME + 3 * CIF + 15 * (CIF // 16) == 4294873728 < 1 << 32
    assert (18642 - 1) * FRAME + 3 * CIF + 15 * (CIF // 16) == 4295104128 >= 1 << 32
    assert 18641 * FRAME == (1 << 32) - 80896                 # the ring's end, 80 896 bytes below 2^32


def test_planner_mapping_at_the_edge(driver):
    """every forced mapping at each size; the planner takes no layout (one answer for natural and class order), so the reach is the
    class-order one for both"""
    small = {(p["n_ens"], p["forced"]): p for p in driver(5)[0]["plans"]}
    assert small[(4096, AUTO)]["mapping"] in (LANE, OCTET), "the cost model must choose a lane mapping somewhere for AUTO to be a case"
    for rec in driver(*SIZES):
        H, fits = rec["H"], rec["H"] <= 18641
        for p in rec["plans"]:
            assert p["status"] == 0
            key = (p["n_ens"], p["forced"])
            if not fits or p["forced"] == WAVE:
                assert (p["mapping"], p["k_wave"], p["n_lane"]) == (WAVE, 3, 0), (H, p)
            elif p["forced"] in (LANE, OCTET):
                assert (p["mapping"], p["k_wave"], p["n_lane"]) == (p["forced"], 0, 3), (H, p)
            else:                                              # AUTO below the edge: the cost model's choice, as for a small ring
                assert (p["mapping"], p["k_wave"], p["n_lane"]) == tuple(small[key][k] for k in ("mapping", "k_wave", "n_lane")), (H, p)
            if p["n_lane"]:
                assert max(kernel_reach(4 * H, 4, FRAME, CIF, c) for c in (False, True)) < 1 << 32, H


def test_generic_batch_rule_at_the_edge_and_agrees_with_the_planner(driver):
    for rec in driver(*SIZES):
        assert rec["batch_lanes"] == (rec["H"] <= 18641), rec
        lane_plan = next(p for p in rec["plans"] if p["n_ens"] == 1 and p["forced"] == LANE)
        assert rec["batch_lanes"] == (lane_plan["mapping"] == LANE), "the two rules disagree"
        if rec["batch_lanes"]:
            assert kernel_reach(4 * rec["H"], 4, FRAME, CIF, True) < 1 << 32


def test_rule_is_exact_for_other_ring_geometries(driver):
    """ring-form code words are free in their geometry: the rule lets through exactly what the kernel's expression keeps below 2^32"""
    rng = np.random.default_rng(5)
    geo = [(16, 1, 1 << 28, 64), (16, 1, (1 << 28) + 16, 64), (17, 1, 1 << 28, 0), (64, 4, 1 << 28, 1 << 26), (64, 4, 286331153, 1024),
           (16, 16, 0, 1 << 28), (16, 16, 0, (1 << 28) + 16), (4294967295, 4, 4, 1), (4294967295, 4, 5, 1), (4294967295, 1, 4294967295, 4294967295)]
    for _ in range(200):
        cifs = int(rng.choice([1, 2, 3, 4, 8, 16]))
        n_slots = int(rng.integers(16, 1 << 17))
        cs = int(rng.integers(0, 1 << 20)) & ~15
        target = (1 << 32) - 3 * cs - int(rng.integers(-2, 3)) * cs // 4            # strides that put the reach near 2^32
        fs = max(1, target // max(1, (n_slots - 1) // cifs))
        geo.append((n_slots, cifs, min(fs, (1 << 32) - 1), cs))
    got = driver(*[":".join(str(v) for v in g) for g in geo])
    seen = set()
    for g, rec in zip(geo, got):
        n_slots, cifs, fs, cs = g
        reach = ((n_slots - 1) // cifs) * fs + (cifs - 1) * cs + 15 * (cs >> 4)
        assert rec["batch_lanes"] == (reach < 1 << 32), (g, reach)
        seen.add(rec["batch_lanes"])
    assert seen == {True, False}
