"""Records tests/golden/mae_reference.npz: the outputs of the reference's utils/mae_utils.py (angular_error_map and compute_mae, which
import only torch and run on the CPU) on the seeded inputs of metrics_ref.golden_cases().  The inputs are stored beside the outputs, so
tests/test_metrics_ref.py reads the fixture alone.

    python tests/make_mae_golden.py REFERENCE_DIR        # the directory that holds the reference's utils/mae_utils.py

Without a reference checkout there is nothing to record: the script says so and leaves the fixture as it is.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as MR  # noqa: E402


def main():
    path = os.path.join(sys.argv[1], "utils", "mae_utils.py") if len(sys.argv) > 1 else ""
    if not os.path.isfile(path):
        raise SystemExit("usage: make_mae_golden.py REFERENCE_DIR (utils/mae_utils.py of the reference not found): nothing recorded")
    spec = importlib.util.spec_from_file_location("reference_mae_utils", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    maps, scaled = MR.golden_cases()
    out = {}
    for name, (p, g) in maps.items():
        out[f"map_{name}_pred"], out[f"map_{name}_gt"] = p, g
        out[f"map_{name}_out"] = ref.angular_error_map(torch.from_numpy(p), torch.from_numpy(g)).numpy()
    for name, (p, g) in scaled.items():
        out[f"mae_{name}_pred"], out[f"mae_{name}_gt"] = p, g
        out[f"mae_{name}_out"] = np.float32(ref.compute_mae(torch.from_numpy(p), torch.from_numpy(g)).item())
    os.makedirs(os.path.dirname(MR.GOLDEN), exist_ok=True)
    np.savez_compressed(MR.GOLDEN, **out)
    print("wrote %s (%d bytes, %d arrays)" % (MR.GOLDEN, os.path.getsize(MR.GOLDEN), len(out)))


if __name__ == "__main__":
    main()
