"""Writes tests/golden/diversity_refusals.json: what the receive-diversity planners (dabgpu_diversity_plan, _plan_banded, _plan_symbols)
answer -- status, whole message and geometry -- and status and whole message of the three dabgpu_diversity_combine_frames* calls and the
three *_host_sync forms wherever they answer without a device, as the library words them today.  DATA only: what the project's own code
printed.  Run from the repo root, for the tree whose wording is to be recorded (default: this one):

    python tests/golden/make_golden_diversity_refusals.py [tree]

The planners are driven through the sub-commands of tests/cpp/diversity_plan_fuzz.cpp (plan), noise_profile_plan_fuzz.cpp (banded) and
sym_profile_plan_fuzz.cpp (dplan), built from the tree's sources.  The six entry points of libdabgpu.so refuse before they touch their
handle, so a made-up handle reaches their checks without a device: no case here is a device call that is accepted with frames to
combine, and none an accepted host form (either would bind the handle); a device call accepted with n_frames 0 returns before that.
tests/test_diversity_refusals.py replays the tables and compares status and whole string."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "diversity_refusals.json")

MANY = (1 << 24) + 1
# per planner: the driver, its sub-command, the argument order, a call that is accepted
PLANNERS = {
    "diversity_plan": ("diversity_plan_fuzz", "plan", "nb nf layout spb stride bits dq scale weight sync null_table null_out last",
                       dict(nb=2, nf=3, bits=0x30000, dq=0x1000000, scale=0x20000)),
    # branch 0 as given, the others well formed with band1
    "diversity_plan_banded": ("noise_profile_plan_fuzz", "banded", "nb nf bits stride layout spb dq0 scale0 weight0 band0 band1 null_bands",
                              dict(nb=2, nf=3, bits=0x30000, dq0=0x1000000, scale0=0x20000, band0=0x500000, band1=0x600000)),
    # every branch the same addresses; tables: 0 both arrays null, 1 the band array only, 2 the symbol array only, 3 both
    "diversity_plan_symbols": ("sym_profile_plan_fuzz", "dplan", "nb nf bits stride layout spb dq scale weight sync band sym tables",
                               dict(nb=2, nf=3, bits=0x30000, dq=0x1000000, scale=0x20000, band=0x500000, sym=0x700000, tables=3)),
}
SCALAR = [dict(nb=0), dict(nb=9), dict(nb=-1), dict(nf=MANY), dict(layout=2), dict(layout=-1), dict(spb=-1), dict(spb=76), dict(stride=8),
          dict(stride=230400 + 8), dict(stride=230400 - 16), dict(bits=0), dict(bits=0x30008),
          dict(nb=0, layout=5), dict(nf=MANY, spb=99), dict(layout=3, stride=1), dict(spb=80, bits=0)]            # the first in the order wins
ACCEPTED = [dict(), dict(nf=0), dict(nf=1024), dict(spb=75), dict(nb=8, spb=1, stride=230400 + 16, layout=1)]
CASES = {
    "diversity_plan": SCALAR + ACCEPTED + [
        dict(null_table=1), dict(null_out=1), dict(null_table=1, null_out=1), dict(null_table=1, nb=0), dict(dq=0), dict(scale=0), dict(dq=0x1000008),
        dict(scale=0x20002), dict(weight=0x50001), dict(sync=0x60002), dict(bits=0, dq=0), dict(dq=0, scale=0x20002), dict(dq=0x1000004, weight=0x50002),
        dict(nb=3, dq=0, last=1), dict(nb=8, sync=0x60001, last=1), dict(weight=0x50000, sync=0x60000)],
    "diversity_plan_banded": SCALAR + ACCEPTED + [
        dict(band0=0x500002), dict(band1=0x600001), dict(weight0=0x50000), dict(weight0=0x50000, band0=0x500002), dict(weight0=0x50000, band1=0x600002),
        dict(weight0=0x50000, band0=0), dict(band0=0, band1=0), dict(band0=0, band1=0, weight0=0x50000), dict(null_bands=1),
        dict(null_bands=1, weight0=0x50000, band0=0x500002), dict(nb=1, band0=0), dict(nb=8, band0=0, band1=0x600002),
        # a scalar fault and a band fault at once: the scalar checks come first
        dict(layout=2, band0=0x500002), dict(dq0=0, weight0=0x50000), dict(scale0=0x20002, band0=0x500001), dict(bits=0x30004, band1=0x600002),
        dict(weight0=0x50002, band0=0x500000)],
    "diversity_plan_symbols": SCALAR + ACCEPTED + [
        dict(sym=0x700002), dict(sym=0x700001, tables=2), dict(sym=0x700002, tables=1), dict(sym=0x700002, tables=0), dict(band=0x500002),
        dict(band=0x500002, tables=2), dict(weight=0x50000), dict(weight=0x50000, tables=2), dict(weight=0x50000, band=0), dict(band=0, sym=0),
        dict(band=0), dict(sym=0), dict(tables=0), dict(tables=1), dict(tables=2), dict(sym=0, tables=2), dict(band=0, tables=1),
        # two faults at once: scalar before band before symbol
        dict(band=0x500002, sym=0x700002), dict(weight=0x50000, sym=0x700002), dict(layout=2, sym=0x700002), dict(dq=0, band=0x500001),
        dict(sync=0x60002, band=0x500001, sym=0x700003), dict(nb=9, weight=0x50000)],
}

# ---- the entry points of the library: per function its cases; arguments as words, so that a case is a row of the JSON table ----
# device calls: ctx 1 = a made-up handle; n_frames 0 unless a case says otherwise; every branch the same record; bands / syms: "null" = no
# array, else one letter per branch: a = an aligned address, m = a misaligned one, - = a null entry
DEVICE = {"dabgpu_diversity_combine_frames": 0, "dabgpu_diversity_combine_frames_banded": 1, "dabgpu_diversity_combine_frames_symbols": 2}
DEVICE_DEFAULTS = dict(ctx=1, nb=2, nf=0, bits=0x30000, stride=0, layout=0, spb=0, k_out=0, mask_out=0, dq=0x1000000, scale=0x20000, weight=0, sync=0,
                       bands="aa", syms="aa", null_table=0)
ALIGN = [dict(k_out=0x80002), dict(mask_out=0x90001), dict(k_out=0x80001, mask_out=0x90002)]
DEVICE_COMMON = [dict(ctx=0), dict(ctx=0, nb=0), dict(ctx=0, k_out=0x80002)] + ALIGN + [
    dict(), dict(k_out=0x80000, mask_out=0x90000), dict(nb=8, bands="a-a-a-a-", syms="-a-aa---", spb=75, layout=1),                # accepted, no frame
    dict(null_table=1), dict(nb=0), dict(nb=9), dict(nf=MANY), dict(layout=2), dict(spb=76), dict(stride=24), dict(bits=0), dict(bits=0x30001),
    dict(dq=0), dict(dq=0x1000004), dict(scale=0x20001), dict(sync=0x60002), dict(layout=2, k_out=0x80002), dict(bits=8, mask_out=0x90002)]


def under(paths):
    """the alignment refusals under a delegation path each"""
    return [dict(p, **a) for p in paths for a in ALIGN] + [dict(p) for p in paths]


DEVICE_CASES = {
    "dabgpu_diversity_combine_frames": DEVICE_COMMON + [dict(weight=0x50000), dict(weight=0x50002)],
    "dabgpu_diversity_combine_frames_banded": DEVICE_COMMON + under([dict(bands="null"), dict(bands="--")]) + [
        dict(bands="m-"), dict(bands="-m"), dict(bands="a-", weight=0x50000), dict(bands="null", weight=0x50000), dict(bands="--", weight=0x50000),
        dict(bands="m-", weight=0x50000), dict(bands="m-", layout=2), dict(bands="m-", k_out=0x80002), dict(bands="-a", k_out=0x80002),
        dict(bands="null", ctx=0), dict(bands="--", ctx=0)],
    "dabgpu_diversity_combine_frames_symbols": DEVICE_COMMON + under([
        dict(syms="null"), dict(syms="--", bands="a-"), dict(syms="--", bands="--"), dict(syms="a-", bands="null"), dict(syms="null", bands="null"),
        dict(syms="--", bands="null"), dict(syms="null", bands="--")]) + [
        dict(syms="m-"), dict(syms="-m", bands="null"), dict(bands="-m"), dict(bands="m-", syms="m-"), dict(bands="a-", syms="m-", weight=0x50000),
        dict(syms="m-", layout=2), dict(syms="m-", k_out=0x80002), dict(syms="null", bands="m-"), dict(syms="--", bands="a-", weight=0x50000),
        dict(syms="null", bands="null", ctx=0), dict(syms="--", bands="--", ctx=0), dict(syms="null", bands="null", weight=0x50002)],
}

# host forms: dq one letter per branch (p = products, at a made-up address that a refused call never reads; - = none) or "null"; scale,
# weight, valid one value per branch or "null"; bands / syms "null" or a letter per branch (t = a table of ones in host memory, - = none)
HOST = {"dabgpu_diversity_combine_host_sync": 0, "dabgpu_diversity_combine_banded_host_sync": 1, "dabgpu_diversity_combine_symbols_host_sync": 2}
HOST_DEFAULTS = dict(ctx=1, dq="pp-", scale="1,1,1", weight="null", valid="null", nb=3, layout=0, bits=0x30000, bands="tt-", syms="t-t")
HOST_COMMON = [dict(ctx=0), dict(dq="null"), dict(scale="null"), dict(bits=0), dict(ctx=0, nb=0), dict(bits=0, layout=7), dict(nb=0), dict(nb=9),
               dict(nb=-3, layout=2), dict(layout=2), dict(layout=-1), dict(layout=2, dq="---"),
               # a live branch without products: under its scalar weight, under a band table (the scalar form has none), with h_valid null
               dict(), dict(weight="1,1,0.5"), dict(weight="2,0,3", dq="p--", scale="1,0,1"), dict(dq="-pp", bands="t--"),
               dict(dq="p--", bands="-t-", weight="1,0,1"), dict(valid="1,1,1"), dict(valid="0,1,0", dq="---"), dict(valid="0,0,1"),
               dict(nb=1, dq="-"), dict(nb=8, dq="ppppppp-", scale="1,1,1,1,1,1,1,1", bands="tttttttt", syms="--------")]
HOST_CASES = {
    "dabgpu_diversity_combine_host_sync": HOST_COMMON,
    # a null array makes the form the narrower one, prefix included; an array of null entries does not
    "dabgpu_diversity_combine_banded_host_sync": HOST_COMMON + [
        dict(bands="null"), dict(bands="null", ctx=0), dict(bands="null", nb=9), dict(bands="null", layout=2), dict(bands="---"), dict(bands="---", nb=0),
        dict(bands="---", layout=3), dict(bands="---", bits=0)],
    "dabgpu_diversity_combine_symbols_host_sync": HOST_COMMON + [
        dict(syms="null"), dict(syms="null", ctx=0), dict(syms="null", nb=9), dict(syms="null", layout=2), dict(syms="null", bands="null"),
        dict(syms="null", bands="null", ctx=0), dict(syms="null", bands="null", nb=0), dict(syms="null", bands="null", layout=2),
        dict(syms="null", bands="---"), dict(syms="---"), dict(syms="---", bands="null"), dict(syms="---", bands="null", bits=0),
        dict(syms="---", bands="---", nb=9), dict(bands="null"), dict(bands="null", layout=2)],
}
LIB_CASES = dict(DEVICE_CASES, **HOST_CASES)
FAKE_HANDLE = 0x1000
ADDRESS = {"a": 0x500000, "m": 0x500002, "p": 0x1000000}


def build_drivers(out_dir, root=ROOT):
    """the three plan drivers, built plain from root's sources: {driver name: path}"""
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
    """the driver's whole answer: status, error and the geometry left behind"""
    driver, sub, order, defaults = PLANNERS[planner]
    args = dict(defaults, **kw)
    argv = [str(args.get(name, 0)) for name in order.split()]
    res = subprocess.run([exes[driver], sub] + argv, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def pointer_table(spec, n, tables=None):
    """a ctypes array of max(n, len(spec)) addresses from one letter per branch, or None for "null" """
    if spec == "null":
        return None
    rows = [None if ch == "-" else (tables[i].ctypes.data if ch == "t" else ADDRESS[ch] + 0x1000 * i) for i, ch in enumerate(spec)]
    return (C.c_void_p * max(n, len(rows), 1))(*rows)


def floats(spec, dtype=np.float32):
    return None if spec == "null" else np.array([float(x) for x in spec.split(",")], dtype)


def run_device(L, fn, kw):
    import dabgpu
    a = dict(DEVICE_DEFAULTS, **kw)
    assert a["ctx"] == 0 or a["nf"] == 0 or a["nf"] > 1 << 24, "a device call that could be accepted with frames to combine"
    table = (dabgpu.DiversityBranch * 16)(*[dabgpu.DiversityBranch(a["dq"] or None, a["scale"] or None, a["weight"] or None, a["sync"] or None)
                                            for _ in range(16)])
    args = [C.c_void_p(FAKE_HANDLE if a["ctx"] else None), None if a["null_table"] else table, a["nb"], a["nf"], a["bits"], a["stride"], a["layout"],
            a["spb"], a["k_out"], a["mask_out"]]
    if DEVICE[fn] >= 1:
        args.append(pointer_table(a["bands"], 16))
    if DEVICE[fn] >= 2:
        args.append(pointer_table(a["syms"], 16))
    st = getattr(L, fn)(*args, None)
    return [st, L.dabgpu_last_error().decode() if st else ""]


def run_host(L, fn, kw):
    a = dict(HOST_DEFAULTS, **kw)
    nb = a["nb"]
    scale, weight, valid = floats(a["scale"]), floats(a["weight"]), floats(a["valid"], np.int32)
    refused = not a["ctx"] or a["dq"] == "null" or scale is None or not a["bits"] or nb < 1 or nb > 8 or a["layout"] not in (0, 1)
    banded = HOST[fn] >= 1 and a["bands"] != "null"
    for b in range(0 if refused else nb):                              # the live rule, restated: the tables here are ones
        w = 1.0 if (banded and a["bands"][b] == "t") or weight is None else weight[b]
        refused = refused or (a["dq"][b] == "-" and (valid is None or valid[b] != 0) and scale[b] > 0 and w > 0)
    assert refused, "a host form that could be accepted"
    ones = [np.ones(128, np.float32) for _ in range(8)]
    p = lambda x: None if x is None else x.ctypes.data
    args = [C.c_void_p(FAKE_HANDLE if a["ctx"] else None), pointer_table(a["dq"], 8), p(scale), p(weight), p(valid), nb, a["layout"], a["bits"], None, None]
    if HOST[fn] >= 1:
        args.append(pointer_table(a["bands"], 8, ones))
    if HOST[fn] >= 2:
        args.append(pointer_table(a["syms"], 8, ones))
    st = getattr(L, fn)(*args)
    return [st, L.dabgpu_last_error().decode() if st else ""]


def run_lib(L, fn, kw):
    return run_device(L, fn, kw) if fn in DEVICE else run_host(L, fn, kw)


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
        assert len(cases) == len(CASES.get(name) or LIB_CASES[name]), (name, "two cases with one key")
    with open(OUT, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    n = sum(len(c) for c in table.values())
    refused = sum(1 for cases in table.values() for v in cases.values() if (v["status"] if isinstance(v, dict) else v[0]))
    print("%s: %d cases, %d of them refusals" % (OUT, n, refused))


if __name__ == "__main__":
    main()
