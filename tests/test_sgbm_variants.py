"""The SGBM instantiations behind process-static A/B switches, bit-exact against the oracle.

SV_SGBM_COST=0 (k_sgbm_hsum_tiled<0..4> + the window-row sums at win 1, 3, 5, 7, 9),
SV_SGBM_H32=0 (16-lane k_sgbm_hpath<N, .., WPE = 1> for every N: 1, 2, 4, 8, 12, 16, 20, 24, 32
at D = 16, 32, 48, 128, 130, 256, 320, 384, 500) and SV_SGBM_VWTA=0 (k_sgbm_vpath<32, N> and
k_sgbm_wta<32, N> unfused for every N of D > 128: 6, 8, 10, 12, 16 at D = 130, 256, 320, 384,
500) are compiled and shipped, but read once per process, so monkeypatch cannot reach them.
Each switch gets one fresh child process (tests/sgbm_variant_child.py), one after another;
this process does not open the GPU itself.
"""
import json
import os
import subprocess
import sys

import pytest

import sgbm_frames as F
from sgbm_variant_child import GROUPS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHILD = os.path.join(HERE, "sgbm_variant_child.py")
SWITCHES = ["SV_SGBM_COST", "SV_SGBM_H32", "SV_SGBM_VWTA"]


@pytest.mark.gpu
def test_gpu_sgbm_ab_variants_match_oracle():
    bad = {}
    for switch in SWITCHES:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env[switch] = "0"
        try:
            p = subprocess.run([sys.executable, CHILD, switch], env=env, cwd=ROOT, capture_output=True,
                               text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{switch}=0: the child did not finish in 120 s; no further child started")
        # a signal, an abort or any other abnormal end: stop here, start no further child
        assert p.returncode == 0, f"{switch}=0: child ended with {p.returncode}\n{p.stderr[-2000:]}"
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert lines, f"{switch}=0: no result line\n{p.stdout[-1000:]}\n{p.stderr[-1000:]}"
        res = json.loads(lines[-1])
        want = sum(c.group == GROUPS[switch] for c in F.CASES)      # 10 windows' cases, 18 of num_disp
        assert want >= 10 and res["switch"] == switch and res["ran"] == want, res
        if res["mismatch"]:
            bad[switch] = res["mismatch"]
    assert not bad, bad
