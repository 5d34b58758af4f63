"""The reference's unchanged BatchedDiffPoolLayer under install(diffpool=True) on the GPU: tests/_diffpool_layer_run.py (which
states the rule) in a fresh interpreter against the reference package build() stages under oracle/_ref/pkg, or $COGDL_REFERENCE."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
def test_reference_layer_on_the_segment_gemms():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_diffpool_layer_run.py"), ROOT, REF, "cuda:0"],
                          capture_output=True, text=True, timeout=600)
    print(proc.stdout)
    assert proc.returncode == 0 and "DIFFPOOL-LAYER-OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
