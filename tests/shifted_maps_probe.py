"""Child process of tests/test_gpu_shifted_maps.py: runs the map and field checks of every case on whatever library
TPIV_LIB names (there: tools/diag/libtorchpiv_hip_mutant_tw.so, whose codelets scale w_N^1 by 1 + 1e-4) and prints what
they said.  Not a test module itself."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import test_gpu_shifted_maps as T
    from torchpiv_amd import _lib, engine
    out = {"lib": _lib.LIB_PATH, "cases": {}}
    only = set(sys.argv[1:])            # (optional: case ids to run, e.g. CWS-32-fast)
    for case in T.CASES:
        if only and T.case_id(case) not in only:
            continue
        rep = T.run_case(engine, *case)
        out["cases"][T.case_id(case)] = {"name": rep["name"], "kind": rep["kind"], "map_worst": rep["map_worst"],
                                         "field_worst": rep["field_worst"], "n_mismatch": len(rep["mismatch"]),
                                         "excused": rep["excused"], "per_family_map": rep["per_family_map"]}
    print("PROBE " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
