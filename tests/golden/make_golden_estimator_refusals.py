"""Writes tests/golden/estimator_refusals.json: status and full message of every refusal of the per-frame estimators' planners
(dabgpu_noise_plan, _noise_profile_plan, _dd_profile_plan, _sym_profile_plan, _clock_estimate_plan, _clock_derotate_plan), of the TII
bank's window check and of the window checks of the NULL-window host forms, as the library words them today.  DATA only: what the
project's own code printed.  Run from the repo root, for the tree whose wording is to be recorded (default: this one):

    python tests/golden/make_golden_estimator_refusals.py [tree]

The planners are driven through the `plan` sub-commands of tests/cpp/*_plan_fuzz.cpp, built from the tree's sources; the three entry points
of libdabgpu.so refuse before they touch their handle, so a made-up handle reaches their checks without a device.
tests/test_estimator_refusals.py replays CASES and compares status and whole string."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "estimator_refusals.json")

FRAME, STATE = 75 * 1536 * 8, 128 * 4
TOP = 1 << 40

# per planner: the driver, its sub-command, the argument order, a call that is accepted
PLANNERS = {
    "noise_plan": ("noise_plan_fuzz", "plan", "mode iq n_frames stride off states freq noise signal weight snr energy valid null_out",
                   dict(mode=1, iq=0x10000, n_frames=3, stride=200000, off=700, weight=0x50000)),
    "noise_profile_plan": ("noise_profile_plan_fuzz", "plan",
                           "mode iq n_frames stride off alpha states freq exclude pin pout weight mean power valid null_out",
                           dict(mode=1, iq=0x10000, n_frames=3, stride=200000, off=700, alpha="0.25", weight=0x50000)),
    "dd_profile_plan": ("dd_profile_plan_fuzz", "plan", "mode dq n_frames alpha sync exclude pin pout weight mean noise amp valid null_out",
                        dict(mode=1, dq=0x1000000, n_frames=3, alpha="0.25", weight=0x50000)),
    "sym_profile_plan": ("sym_profile_plan_fuzz", "plan", "mode dq n_frames sync weight noise ref valid null_out",
                         dict(mode=1, dq=0x1000000, n_frames=3, weight=0x50000)),
    "clock_estimate_plan": ("clock_plan_fuzz", "eplan", "mode dq n_frames sync slope_in gain slope_out residual corr valid null_out",
                            dict(mode=1, dq=0x1000000, n_frames=3, gain="1.0", slope_out=0x50000)),
    "clock_derotate_plan": ("clock_plan_fuzz", "dplan", "mode src dst n_frames sync slope spb null_out",
                            dict(mode=1, src=0x1000000, dst=0x1000000, n_frames=3, slope=0x50000)),
}
OPENING = [dict(null_out=1), dict(mode=0), dict(mode=4), dict(n_frames=0), dict(n_frames=(1 << 24) + 1),
           dict(mode=2, n_frames=0), dict(null_out=1, mode=3)]
NULL_WINDOW = [dict(stride=0), dict(stride=TOP + 1), dict(off=TOP + 1, stride=TOP), dict(states=0x60000, stride=700 + 2656 + 1542),
               dict(n_frames=0, stride=0)]
CASES = {
    "noise_plan": OPENING + NULL_WINDOW + [
        dict(iq=0), dict(iq=0x10004), dict(iq=0, states=0x60002), dict(iq=0x10001, stride=0), dict(states=0x60002), dict(freq=0x70001),
        dict(noise=0x80002), dict(signal=0x80003), dict(weight=0x50001), dict(snr=0x80001), dict(energy=0x90002), dict(valid=0xA0001),
        dict(stride=700 + 5208 - 1), dict(valid=0xA0002, stride=5), dict(weight=0), dict(weight=0, states=0x60000, freq=0x70000),
        dict(weight=0, stride=3)],
    "noise_profile_plan": OPENING + NULL_WINDOW + [
        dict(iq=0), dict(iq=0x10004), dict(iq=0, alpha="0.0"), dict(states=0x60002), dict(exclude=0x71002), dict(pin=0x800003), dict(pout=0x900001),
        dict(mean=0x80202), dict(power=0x90001), dict(valid=0xA0002), dict(stride=700 + 2656 - 1), dict(alpha="0.0"), dict(alpha="-0.25"),
        dict(alpha="1.5"), dict(alpha="nan"), dict(alpha="inf"), dict(alpha="2.0", stride=0), dict(pin=0x800000, pout=0x800004),
        dict(pin=0x800000 + 3 * STATE - 4, pout=0x800000), dict(pin=0x800000, pout=0x800004, alpha="0.0"),
        dict(pin=0x800000, pout=0x800004, weight=0), dict(weight=0), dict(weight=0, pin=0x800000, exclude=0x71000)],
    "dd_profile_plan": OPENING + [
        dict(dq=0), dict(dq=0x1000008), dict(dq=0x1000001), dict(dq=0, sync=0x60002), dict(sync=0x60002), dict(exclude=0x71001), dict(pin=0x800002),
        dict(pout=0x900003), dict(weight=0x50002), dict(mean=0x80201), dict(valid=0xA0002), dict(noise=0x90004), dict(amp=0x98004),
        dict(noise=0x90004, amp=0x98002), dict(noise=0x90004, valid=0xA0002), dict(alpha="0.0"), dict(alpha="nan"), dict(alpha="1.0000001"),
        dict(alpha="0.0", amp=0x98004), dict(pin=0x800000, pout=0x800004), dict(pin=0x800000, pout=0x800000 + 3 * STATE - 4),
        dict(pin=0x800000, pout=0x800004, alpha="-1.0"), dict(weight=0), dict(weight=0, pin=0x800000, sync=0x60000),
        dict(weight=0, pin=0x800000, pout=0)],
    "sym_profile_plan": OPENING + [
        dict(dq=0), dict(dq=0x1000008), dict(dq=0x1000004), dict(dq=0, weight=0), dict(sync=0x60001), dict(weight=0x50002), dict(noise=0x80003),
        dict(ref=0x90001), dict(valid=0xA0002), dict(dq=0x1000008, valid=0xA0002), dict(weight=0), dict(weight=0, sync=0x60000),
        dict(weight=0, sync=0x60002)],
    "clock_estimate_plan": OPENING + [
        dict(dq=0), dict(dq=0x1000008), dict(dq=0, gain="0.0"), dict(slope_in=0x70004), dict(slope_out=0x50004), dict(residual=0x90004),
        dict(slope_in=0x70004, sync=0x60002), dict(sync=0x60002), dict(corr=0x98002), dict(valid=0xA0001), dict(gain="0.0"), dict(gain="-0.5"),
        dict(gain="1.0000001"), dict(gain="nan"), dict(gain="inf"), dict(gain="0.0", valid=0xA0001), dict(slope_in=0x50008), dict(slope_in=0x50010),
        dict(slope_in=0x50000 + 16, slope_out=0x50000, gain="2.0"), dict(slope_out=0), dict(slope_out=0, slope_in=0x70000, sync=0x60000),
        dict(slope_out=0, slope_in=0x50008)],
    "clock_derotate_plan": OPENING + [
        dict(src=0), dict(dst=0), dict(src=0, dst=0), dict(src=0x1000008), dict(dst=0x2000004), dict(src=0, slope=0), dict(dst=0x1000010),
        dict(src=0x1000000 + 3 * FRAME - 16), dict(dst=0x1000010, slope=0), dict(slope=0), dict(slope=0x50004), dict(slope=0, sync=0x60002),
        dict(sync=0x60002), dict(sync=0x60001, spb=76), dict(spb=-1), dict(spb=76), dict(slope=0x50004, spb=99)],
}

# the entry points of the library that refuse in front of their handle: (function, arguments behind the handle, defaults)
LIB_DEFAULTS = {
    "dabgpu_tii_bank_process": dict(iq=0x10000, stride=200000, off=700, states=0, freq=0, decide=0, results=0, counts=0, stream=0),
    "dabgpu_noise_estimate_host_sync": dict(iq=0x10000, n=200000, off=700, freq=0.0, fto=0, out=None),
    "dabgpu_noise_profile_host_sync": dict(iq=0x10000, n=200000, off=700, freq=0.0, fto=0, exclude=0, profile=0, alpha=0.25, weight=0, mean=0, power=0,
                                           valid=0),
}
LIB_CASES = {
    "dabgpu_tii_bank_process": [dict(iq=0), dict(iq=0x10004), dict(iq=0, stride=0), dict(stride=0), dict(stride=700 + 2656 - 1), dict(stride=TOP + 1),
                                dict(off=TOP + 1, stride=TOP), dict(states=0x60000, stride=700 + 2656 + 1542), dict(iq=0x10001, stride=1),
                                dict(stride=0, decide=1), dict(decide=1), dict(states=0x60002), dict(decide=1, results=0x70000, counts=0x80002)],
    "dabgpu_noise_estimate_host_sync": [dict(fto=-505), dict(fto=1544), dict(n=700 + 5208 - 1), dict(off=0, fto=-1), dict(off=TOP + 1),
                                        dict(n=TOP + 1), dict(fto=1543, n=700 + 1543 + 5207), dict(fto=2000, n=0)],
    "dabgpu_noise_profile_host_sync": [dict(alpha=0.0), dict(alpha=0.0, fto=-505), dict(fto=-505), dict(fto=1544), dict(n=700 + 2656 - 1),
                                       dict(off=0, fto=-1), dict(off=TOP + 1), dict(n=TOP + 1), dict(fto=1543, n=700 + 1543 + 2655),
                                       dict(fto=2000, n=0)],
}
FAKE_HANDLE = 0x1000


def build_drivers(out_dir, root=ROOT):
    """the five plan drivers, built plain from root's sources: {driver name: path}"""
    csrc = os.path.join(root, "dab-radio_amd", "csrc")
    exes = {}
    for name in sorted({p[0] for p in PLANNERS.values()}):
        exes[name] = os.path.join(str(out_dir), name)
        res = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(root, "include"), "-I" + csrc,
                              os.path.join(root, "tests", "cpp", name + ".cpp"), os.path.join(csrc, "dabgpu_host_logic.cpp"), "-o", exes[name]],
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-4000:]
    return exes


def key(kw):
    return ",".join("%s=%s" % (k, kw[k]) for k in sorted(kw))


def run_planner(exes, planner, kw):
    driver, sub, order, defaults = PLANNERS[planner]
    args = dict(defaults, **kw)
    argv = [str(args.get(name, 0)) for name in order.split()]
    res = subprocess.run([exes[driver], sub] + argv, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout)
    return [out["status"], out["error"]]


def run_lib(L, fn, kw):
    args = dict(LIB_DEFAULTS[fn], **kw)
    rec = (C.c_uint32 * 8)()
    vals = [C.byref(rec) if v is None else v for v in args.values()]
    st = getattr(L, fn)(C.c_void_p(FAKE_HANDLE), *vals)
    return [st, L.dabgpu_last_error().decode()]


def collect(exes, L):
    out = {}
    for planner, cases in CASES.items():
        out[planner] = {key(kw): run_planner(exes, planner, kw) for kw in cases}
    for fn, cases in LIB_CASES.items():
        out[fn] = {key(kw): run_lib(L, fn, kw) for kw in cases}
    return out


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
    if root != ROOT:
        os.environ["DABGPU_LIB"] = os.path.join(root, "dab-radio_amd", "libdabgpu.so")
    sys.path.insert(0, os.path.join(ROOT, "dab-radio_amd"))
    import dabgpu
    with tempfile.TemporaryDirectory() as tmp:
        table = collect(build_drivers(tmp, root), dabgpu.lib())
    for name, cases in table.items():
        assert all(st != 0 and text for st, text in cases.values()), (name, [k for k, v in cases.items() if v[0] == 0])
    with open(OUT, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d refusals" % (OUT, sum(len(c) for c in table.values())))


if __name__ == "__main__":
    main()
