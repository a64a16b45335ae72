"""Child process of tests/test_gpu_f64_pass1.py: runs the gates of the named cases on whatever library TPIV_LIB names and
under whatever TPIV_EXACT_BAND_SCALE the parent set (the library reads it once per process), and prints the reports.
Stops at the first case the device does not survive: a non-zero exit status ends the parent's test.  Not a test module."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    os.environ.setdefault("MKL_CBWR", "COMPATIBLE")         # (as tests/conftest.py pins it for the oracle)
    import test_gpu_f64_pass1 as T
    from torchpiv_amd import _lib, engine
    out = {"lib": _lib.LIB_PATH, "band_scale": os.environ.get("TPIV_EXACT_BAND_SCALE"), "cases": {}}
    for cid in sys.argv[1:]:
        out["cases"][cid] = T.run_case(engine, T.BY_ID[cid])
        print(T.report_line(out["cases"][cid]), file=sys.stderr, flush=True)
    print("PROBE " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
