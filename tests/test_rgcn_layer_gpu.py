"""The reference's unchanged RGCNLayer under install(rgcn=True) on the GPU, both regularisers (tests/_rgcn_layer_run.py, in a
fresh interpreter against the reference package build() stages under oracle/_ref/pkg, or $COGDL_REFERENCE): output and every
gradient within 4 x the float32 error of the layer's law composed in float64, as tests/test_relational_layer_gpu.py; the two
methods are the reference's own objects again after uninstall()."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
def test_reference_layer_on_the_rgcn_operators():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_rgcn_layer_run.py"), ROOT, REF, "cuda:0"],
                          capture_output=True, text=True, timeout=600)
    print(proc.stdout)
    assert proc.returncode == 0 and "RGCN-LAYER-OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
