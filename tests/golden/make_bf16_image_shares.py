"""Writes golden/bf16_image_cpu_shares.json: per NT case of tests/bf16_image_cases.py (at 256 CUs)
the number of elements the CPU float32 evaluation rounds to another bf16 value than the float64
reference does.  Run from the repository root: python tests/golden/make_bf16_image_shares.py"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parents[1]), str(HERE.parent)]

import bf16_image_cases as bc  # noqa: E402

if __name__ == "__main__":
    bc.SHARES_FILE.write_text(json.dumps(bc.compute_shares(), indent=1) + "\n")
    print(bc.SHARES_FILE.read_text())
