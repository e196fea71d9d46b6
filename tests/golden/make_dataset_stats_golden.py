"""Writes tests/golden/dataset_stats_metadata.json: what the REFERENCE's simulation/generate_metadata.py computes for recordings of
tests/dataset_stats_cases.py.  Needs a checkout of the reference (its path is the argument) and pandas; run by hand when the
cases change:

    python tests/golden/make_dataset_stats_golden.py <reference checkout>

Nothing of the reference is copied: the fixture holds the metadata.json its script wrote for our inputs.  Per fixture case the
recordings (FIXTURE_SIZES of dataset_stats_cases.FIXTURE_KINDS: one T, as the script reads every file with one --timesteps) go
out as particles_%06d.csv, rows time-major, every float32 printed with 17 significant digits (the decimal form of the float32 as
a double), and the script's main() runs over that directory.
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dataset_stats_cases as dc  # noqa: E402


def main():
    ref = sys.argv[1]
    spec = importlib.util.spec_from_file_location("generate_metadata", os.path.join(ref, "simulation", "generate_metadata.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = {}
    for kind in dc.FIXTURE_KINDS:
        k = dc.KINDS[kind]
        with tempfile.TemporaryDirectory() as d:
            for i, (t, n) in enumerate(dc.FIXTURE_SIZES):
                rec = dc.recording(kind, t, n)
                np.savetxt(os.path.join(d, "particles_%06d.csv" % i), rec.reshape(-1, dc.D).astype(np.float64), fmt="%.17g", delimiter=",")
            cols = list(range(k.cart0, k.cart0 + k.dim))
            gen.main(argparse.Namespace(data_dir=d, target_dir=None, timesteps=dc.FIXTURE_SIZES[0][0], upper_bounds=[0.9] * k.dim,
                                        lower_bounds=[0.1] * k.dim, cartesian_idx=cols, control_idx=[5, 6, 7], material_id=dc.MAT_COL))
            with open(os.path.join(d, "metadata.json")) as fp:
                out[kind] = json.load(fp)
    with open(os.path.join(HERE, "dataset_stats_metadata.json"), "w") as fp:
        json.dump(out, fp, indent=1)
    print("wrote", sorted(out))


if __name__ == "__main__":
    main()
