"""A short run of the randomised parity sweeps (tools/fuzz_parity.py) with fixed seeds: shapes nobody wrote down by hand, at the suite's
usual values and in the saturated-gate regime (tests/hot_cases.py).
The long runs are recorded in profiles/r03_fuzz_parity.txt."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode,cases,seed", [("seq", 60, 11), ("stack", 40, 12), ("wide", 40, 13)])
def test_random_shapes_against_the_oracle(mode, cases, seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), str(cases), str(seed), mode],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
    assert " 0 FAILED" in r.stdout
    if mode in ("seq", "wide"):   # these draws stay inside the library's envelope: nothing may be refused
        assert f" {cases} ok, 0 refused by the library" in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize("mode,cases,seed", [("seq", 40, 21), ("rb", 25, 22), ("stack", 25, 23)])
def test_random_shapes_in_the_saturated_regime_against_the_oracle(mode, cases, seed):
    """The same draws with biases at sigma 5 (one case in four: 40), x at sigma 3 and c0 at sigma 4; a case plain fp32 cannot be held to
    is drawn again before it reaches the GPU, and the run counts those (tests/test_hot_regime_cpu.py replays the count without a GPU)."""
    import re
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), str(cases), str(seed), mode, "hot"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
    assert " 0 FAILED" in r.stdout
    if mode == "seq":   # these draws stay inside the library's envelope: nothing may be refused
        assert f" {cases} ok, 0 refused by the library" in r.stdout, r.stdout[-3000:]
    m = re.search(r", (\d+) redrawn \(fp32 oracle\)", r.stdout)
    assert m is not None, r.stdout[-1000:]
    assert int(m.group(1)) <= 0.10 * cases, r.stdout[-1000:]
    print("\n" + r.stdout.strip().splitlines()[-1])
