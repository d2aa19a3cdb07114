"""tests/golden/ref_fresh.npz: the outputs of oracle/_ref/libjdet_ref.so (the reference's own CPU sources, built by
oracle/build_ref.py) on the fresh inputs of tests/test_oracle_golden_cpu.py (``fresh_iou_case`` / ``fresh_nms_cases``),
so that the oracle is compared with the reference build where that build is absent.
Run in the build container after build():  python tests/golden/make_ref_fresh.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
from test_oracle_golden_cpu import reference_build_outputs  # noqa: E402


def main():
    r = oracle.ref()
    assert r.available, "oracle/_ref not built"
    out = reference_build_outputs(r)
    path = os.path.join(HERE, "ref_fresh.npz")
    np.savez_compressed(path, provenance=np.array("oracle/_ref/libjdet_ref.so (g++ -O2 -std=c++14) on the seeded "
                                                  "cases of tests/test_oracle_golden_cpu.py"), **out)
    print("wrote", path, {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
