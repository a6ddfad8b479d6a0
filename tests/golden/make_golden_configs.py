"""Record tests/golden/dota_configs.json: the settings of the reference's three configs/dota/*.py files, loaded UNCHANGED
through the package's mmcv-free Config.fromfile (tuples kept as {"__tuple__": [...]}, key order kept).  Run where the
reference tree is (python tests/golden/make_golden_configs.py <reference root>); the fixture is committed."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from orientedreppoints_amd.mmdet_models import Config  # noqa: E402


def encode(v):
    if isinstance(v, dict):
        return {k: encode(x) for k, x in v.items()}
    if isinstance(v, tuple):
        return {"__tuple__": [encode(x) for x in v]}
    if isinstance(v, list):
        return [encode(x) for x in v]
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ORP_REFERENCE_ROOT")
    if not ref:
        raise SystemExit("usage: make_golden_configs.py <reference root> (or ORP_REFERENCE_ROOT)")
    cfg_dir = os.path.join(ref, "configs", "dota")
    out = {f: encode(dict(Config.fromfile(os.path.join(cfg_dir, f))._cfg_dict)) for f in sorted(os.listdir(cfg_dir))}
    with open(os.path.join(HERE, "dota_configs.json"), "w") as g:
        json.dump(out, g, indent=1)
        g.write("\n")


if __name__ == "__main__":
    main()
