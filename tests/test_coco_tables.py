"""The host half of scoring (engine/coco_tables.py: accumulate, summarize, joining tables) is NumPy only: importing it loads
neither the binding nor the HIP library."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = "cvpr22_cross_modal_pseudo_labeling_amd"


def test_importing_coco_tables_loads_no_device_code():
    code = (f"import sys; import {PACKAGE}.engine.coco_tables as t; "
            f"assert callable(t.accumulate) and callable(t.merge_shard_tables); "
            f"print(sorted(m for m in sys.modules if m in ('{PACKAGE}._C', '{PACKAGE}._lib', 'torch')))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "[]", out.stdout
