"""-m gpu: tools/waterfall.py --blank with --interferer-gate bursts, the tool run as a program on its smallest useful shape (two receivers,
six frames, one SNR, 15 dB): with white bursts on 205 of every 20480 samples, 17 dB above the signal, the unblanked receiver loses FIBs on
both channels and the blanked one delivers every FIB; between 1 and 2 % of the blocks are zeroed.  What is held per protection level
follows what the closed loop of tests/test_blanker_closed_loop.py establishes on the CPU models, not what this run happens to give: the
FIC and EEP 3-A are delivered whole behind the blanker from SNR 9 dB on, so they, and the stronger codes EEP 1-A and 2-A, must show no byte
error; for EEP 4-A (rate 3/4, the weakest, with errors of its own at 12 and 13 dB on two paths in profiles/tx/waterfall.md) and the UEP
row nothing is claimed but that blanking does not make them worse: a symbol that loses 10 of its 80 blocks keeps 12 % less energy and
gains inter-carrier interference, which a code without margin shows (first run: EEP 4-A 3.35e-01 -> 3.86e-04 on two paths, 2.71e-01 -> 0
on white noise).  The tool's exit status is its sensitivity verdict (1: not error-free at the top SNR), so 0 and 1 both count as a run.
The options are refused outside the plain receiver path."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "waterfall.py")


def test_bursts_cost_fibs_unblanked_and_nothing_blanked(tmp_path):
    out = tmp_path / "waterfall_blank.md"
    res = subprocess.run([sys.executable, TOOL, "--blank", "--interferer-gate", "20480:205:17", "--streams", "2", "--frames", "6", "--snr", "15:15:1",
                          "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert res.returncode in (0, 1), res.stdout[-2000:] + res.stderr[-2000:]
    text = out.read_text()
    rows = re.findall(r"^\| 15 \| ([0-9.]+) -> ([0-9.]+) \|(.*)\|$", text, re.M)
    assert len(rows) == 2, text                                              # white noise, and two paths
    for unblanked, blanked, cells in rows:
        print(f"FIB CRC pass {unblanked} -> {blanked}; byte errors {cells}")
        assert float(blanked) == 1.0 and float(unblanked) < 0.95
        levels = [[float(v) for v in c.split("->")] for c in cells.split("|")]       # EEP 1-A, 2-A, 3-A, 4-A, UEP row 20
        assert len(levels) == 5
        assert all(after == 0.0 for _, after in levels[:3])                  # no byte error behind the blanker
        assert all(after <= before for before, after in levels)              # and no level made worse
    shares = [float(v) for v in re.findall(r"15 dB ([0-9.]+) %", text)]
    assert len(shares) == 2 and all(1.0 < v < 2.0 for v in shares), shares


def test_option_rules():
    for extra, want in ((["--blank", "1"], "threshold above 1"), (["--blank", "--ber"], "plain receiver path"),
                        (["--interferer-gate", "100:5:17", "--branches", "2"], "plain receiver path"),
                        (["--interferer-gate", "100:200:17"], "ON <= PERIOD"), (["--interferer-gate", "100:5"], "PERIOD:ON:IS_DB")):
        res = subprocess.run([sys.executable, TOOL] + extra, capture_output=True, text=True, timeout=60)
        assert res.returncode != 0 and want in res.stderr, (extra, res.stderr[-300:])
