"""One A/B variant of the SGBM kernels against the oracle, in a process of its own.

SV_SGBM_COST, SV_SGBM_H32 and SV_SGBM_VWTA are read once per process, so the instantiations
they select can only be reached by a process started with the switch in its environment:
tests/test_sgbm_variants.py starts this script once per switch.  It runs the cases of
the switch's group from tests/sgbm_frames.py through engine.sgbm, compares each map bit for
bit with the oracle's, prints one JSON line and exits 0 (a mismatch is reported, not raised).

    SV_SGBM_COST=0 python tests/sgbm_variant_child.py SV_SGBM_COST
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)

# switch -> the group whose cases make the instantiations it selects launch:
#   SV_SGBM_COST=0: k_sgbm_hsum_tiled<0..4> + the window-row sums for win 1, 3, 5, 7, 9
#   SV_SGBM_H32=0:  16-lane k_sgbm_hpath<N, .., WPE = 1>, unfused, N = 1, 2, 4, 8, 12, 16, 20, 24,
#                   32 at D = 16, 32, 48, 128, 130, 256, 320, 384, 500 (sgbm_frames.CVD_NUM_DISP)
#   SV_SGBM_VWTA=0: k_sgbm_vpath<32, N> + k_sgbm_wta<32, N> unfused, N = 6, 8, 10, 12, 16 at
#                   D = 130, 256, 320, 384, 500
GROUPS = {"SV_SGBM_COST": "cvwin", "SV_SGBM_H32": "cvd", "SV_SGBM_VWTA": "cvd"}


def main(switch):
    import sgbm_frames as F
    from stereovision_amd.engine import get_engine
    assert os.environ.get(switch) == "0", f"{switch}=0 expected in the environment"
    engine = get_engine(0)
    ran, bad = [], []
    for c in F.CASES:
        if c.group != GROUPS[switch]:
            continue
        L, R = c.frames()
        got = engine.sgbm(L, R, c.min_disp, c.D, c.win, **c.engine_kw())
        ran.append(c.id)
        if not np.array_equal(got, F.expected(c)):
            bad.append(c.id)
    print(json.dumps({"switch": switch, "ran": len(ran), "mismatch": bad}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
