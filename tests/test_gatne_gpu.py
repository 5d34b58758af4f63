"""embedding.gatne on the GPU: the run on the two-layer block network of tests/_gatne_cases.py through the HIP kernels (walks,
multiplex_embed, sampled_scores) -- purity of at least 0.9 in every layer, unit-norm rows, a falling loss, equal bytes for one
seed -- without a TorchRouteWarning."""
import warnings

import pytest

import _gatne_cases as G

pytestmark = pytest.mark.gpu


def test_the_run_on_the_block_network():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        G.check_run("cuda")
