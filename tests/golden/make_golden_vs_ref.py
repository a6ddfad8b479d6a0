"""Record tests/golden/oracle_vs_ref.npz (and the files the test module's SPLIT names): every call that tests/test_oracle_vs_ref.py makes of the reference's own functions
(oracle/_ref/libref_orp.so, built by oracle/build_ref.py from the reference's sources), on the test's own seeded inputs.
Run where the reference tree is (python tests/golden/make_golden_vs_ref.py); the fixture is committed."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import build_ref, orp_oracle  # noqa: E402


def main():
    if not build_ref.build() or orp_oracle.ref() is None:
        raise SystemExit("oracle/_ref could not be built: the reference tree is needed to record this fixture")
    spec = importlib.util.spec_from_file_location("test_oracle_vs_ref", os.path.join(ROOT, "tests", "test_oracle_vs_ref.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    orp_oracle.build()
    record = {}
    for name in sorted(n for n in dir(t) if n.startswith("test_")):
        fn = getattr(t, name)
        params = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        if params:
            argname, values = params[0].args
            cases = [("%s[%s]" % (name, v), {argname: v}) for v in values]
        else:
            cases = [(name, {})]
        for test_id, kw in cases:
            rec = t.Recorded(orp_oracle, test_id, record=record)
            fn(ref=rec, **kw)
            rec.finish()
    files = {}
    for key, v in record.items():
        files.setdefault(t.golden_file_of(key), {})[key] = v
    for name, arrays in sorted(files.items()):
        path = os.path.join(HERE, name)
        if os.path.exists(path):                      # leave a file alone whose records did not change
            with np.load(path) as old:
                if sorted(old.files) == sorted(arrays) and all(
                        old[k].dtype == np.asarray(arrays[k]).dtype and np.array_equal(old[k], arrays[k], equal_nan=True) for k in arrays):
                    print("%s: unchanged (%d arrays)" % (name, len(arrays)))
                    continue
        np.savez_compressed(path, **arrays)
        print("%s: %d arrays" % (name, len(arrays)))


if __name__ == "__main__":
    main()
