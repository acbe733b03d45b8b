"""Child process of tests/test_conv_ref_cpu.py and tests/test_conv_routes_gpu.py (a helper, not a test): one group of tests/conv_ref.py's CACHED cases.
The parent sets the group's CLHIP_<NAME> switches in this process's environment: they are cached at their first use, so no in-process test can flip them.
usage: python conv_route_worker.py GROUP_INDEX [run]      prints the routes; with `run`, launches every case on the GPU and prints its worst err / bound"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import conv_ref as R                      # noqa: E402
from libcontinual_amd import _lib         # noqa: E402


def main():
    group = R.CACHED[int(sys.argv[1])]
    L = _lib.lib()
    out = {}
    for case in group["cases"]:
        out[case["name"]] = {f"{dt}/{key}": fam for (dt, key), fam in R.routes_of(L, case).items()}
    print("ROUTES " + json.dumps(out))
    if len(sys.argv) > 2 and sys.argv[2] == "run":
        import conv_run
        worst = {}
        for case in group["cases"]:
            res = conv_run.run_case(L, case)
            worst[case["name"]] = {f"{dt}/{key}/{what}": r for (dt, key, what), r in res.items()}
        print("RATIOS " + json.dumps(worst))


if __name__ == "__main__":
    main()
