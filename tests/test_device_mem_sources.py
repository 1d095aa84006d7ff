"""CPU, no build: what the runtime hands out is released in one place.  In dab-radio_amd/csrc the four release calls occur in
device_mem.h only -- and in dabgpu_abi.hip, whose context parks outgrown scratch buffers for captured graphs and keeps its own lists --
and no struct keeps a blanket list of allocations beside its members."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
RELEASES = ("hipFree(", "hipHostFree(", "hipEventDestroy(", "hipStreamDestroy(")
ALLOWED = {"device_mem.h", "dabgpu_abi.hip"}


def sources():
    names = sorted(n for n in os.listdir(CSRC) if n.endswith((".h", ".hip", ".cpp")))
    assert "device_mem.h" in names and "ofdm_stream.hip" in names and len(names) > 40
    return [(n, open(os.path.join(CSRC, n), encoding="utf-8").read()) for n in names]


def test_release_calls_live_in_the_owner_header_only():
    found = {(name, word) for name, text in sources() for word in RELEASES if word in text}
    assert {n for n, _ in found} <= ALLOWED, sorted(f for f in found if f[0] not in ALLOWED)
    # the header does release each kind: the check above is not vacuous
    assert {w for n, w in found if n == "device_mem.h"} == set(RELEASES)


def test_no_struct_keeps_a_list_of_allocations():
    pattern = re.compile(r"std::vector\s*<\s*void\s*\*\s*>\s*allocs")
    assert [name for name, text in sources() if pattern.search(text)] == []
