"""The sections of the reference's config files that the shipped configs under configs/ must equal, as the reference's
own Config loader sees them (``Config(path).dump()``), stored as data so that the comparison runs without the reference
(tests/test_configs_cpu.py, tests/test_config_registry_cpu.py, tests/test_orcnn_cpu.py).  Tuples are stored as
``{"__tuple__": [...]}``: a config's tuple and list are different values to the comparison.
Run in the build container:  python tests/golden/make_config_golden.py  ->  tests/golden/ref_configs.json
(``--check``: fail if the stored file differs from what the reference says today)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "ref_configs.json")
BASE_KEYS = ["model", "optimizer", "scheduler", "max_epoch", "log_interval", "checkpoint_interval"]
# shipped file name -> (the reference's file, the sections compared)
FILES = {
    "s2anet_r50_fpn_1x_dota.py": ("configs/s2anet/s2anet_r50_fpn_1x_dota.py", BASE_KEYS),
    "s2anet_r101_fpn_1x_dota_rotate_balance_ms.py": ("projects/s2anet/configs/s2anet_r101_fpn_1x_dota_rotate_balance_ms.py",
                                                     BASE_KEYS + ["dataset", "eval_interval", "dataset_root"]),
    "orcnn_van3_7_anchor.py": ("configs/orcnn_van3_7_anchor_swa_1.py",
                               BASE_KEYS + ["optimizer_swa", "scheduler_swa", "swa_start_epoch", "eval_interval",
                                            "merge_nms_threshold_type"]),
}


def encode(x):
    if isinstance(x, tuple):
        return {"__tuple__": [encode(v) for v in x]}
    if isinstance(x, list):
        return [encode(v) for v in x]
    if isinstance(x, dict):
        return {k: encode(v) for k, v in x.items()}
    return x


def decode(x):
    if isinstance(x, dict):
        if set(x) == {"__tuple__"}:
            return tuple(decode(v) for v in x["__tuple__"])
        return {k: decode(v) for k, v in x.items()}
    if isinstance(x, list):
        return [decode(v) for v in x]
    return x


def load():
    """{shipped file name: {section: value}} of the stored fixture, tuples restored."""
    with open(OUT) as f:
        return decode(json.load(f))


def from_reference():
    sys.path.insert(0, ROOT)
    from rs_detection_amd.config import Config
    out = {}
    for name, (rel, keys) in FILES.items():
        d = Config(os.path.join(REF, rel)).dump()
        out[name] = {k: d.get(k) for k in keys}
    return out


def main():
    out = from_reference()
    if "--check" in sys.argv:
        assert load() == out, "tests/golden/ref_configs.json is stale: re-run this script"
        return
    with open(OUT, "w") as f:
        json.dump(encode(out), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, {k: sorted(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
