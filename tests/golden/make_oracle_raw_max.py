"""Writes tests/golden/oracle_raw_max.json: for every reference golden that ran
without error, the max of the ORACLE's unnormalised products over the
fixture's batch (oracle/ref_infer.py OracleBN.infer_raw), as a float hex
string.  tests/parity.py scales its absolute floor by it, so the GPU tests
need no oracle pass per fixture; tests/test_oracle_golden.py pins every entry
to the oracle's own run.  The reference is not needed.

    python tests/golden/make_oracle_raw_max.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

from golden_io import golden_names, load_golden, param_golden_names  # noqa: E402
from parity import golden_raw  # noqa: E402


def main():
    out = {}
    for name in golden_names():
        if not load_golden(name)["meta"]["error"]:
            out[name] = float(np.float32(golden_raw(name).max())).hex()
    for name in param_golden_names():
        out[name] = float(np.float32(golden_raw(name, True).max())).hex()
    with open(os.path.join(HERE, "oracle_raw_max.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
