"""The host twin of the three walk operators still returns exactly the arrays recorded in tests/golden/walk_pins.npz (written
by tests/golden/make_walk_pins.py before the walks were split into rules and one scaffold).  The other walk tests compare the
GPU with the host and laws by chi-square: they would pass if both sides changed together.  This one would not."""
import importlib.util
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_host_walks_equal_the_recorded_arrays():
    spec = importlib.util.spec_from_file_location("make_walk_pins", os.path.join(GOLDEN, "make_walk_pins.py"))
    pins = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pins)
    want = np.load(os.path.join(GOLDEN, "walk_pins.npz"))
    got = pins.compute()
    assert sorted(got) == sorted(want.files) and len(got) == 57
    for name in sorted(got):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), name
    # what the record is made of: 64 walkers x 20 positions, walks that end early, steps decided by the fallback
    assert want["random.random_walk.0.3"].shape == (pins.WALKERS, pins.LENGTH) == (64, 20)
    assert sum(int(want["%s.node2vec.one_trial.fallback" % g].sum()) for g in ("dup", "n2v", "random", "star")) > 100
    held = np.concatenate([want["%s.metapath.lengths" % g] for g in pins.TYPED])
    assert int((held < 20).sum()) > 100 and int((held == 20).sum()) > 60
