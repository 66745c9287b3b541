"""CPU: the C oracle in the dispersion-floor regime against the LAPACK restatement (see tests/floor_regime.py for what
is compared and why)."""
import hashlib

import numpy as np
import pytest

from tests import wide_cases
from tests.floor_regime import SEEDS, assert_visible_parity, floor_case, rates, visible_chain

# sha256 over the counts (as int64) and the design of floor_case(seed) as it stood before it took a design argument
DIGESTS = {5: "c52d0e24944311fe", 6: "d55d0ca93eacb9fd", 7: "ce77e032d735520f"}


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_floor_regime_vs_lapack(oracle, seed):
    from oracle import lapack_oracle
    d = floor_case(seed)
    ref = visible_chain(lapack_oracle, d)
    got = visible_chain(oracle, d)
    s = assert_visible_parity(got, ref, "oracle seed %d" % seed)
    # the premise of the module: on the floor genes the step COUNT is rounding noise of the special functions underneath
    # (two correct implementations agree on few of them) while everything R's callers see agrees
    assert s["iter_equal_floor"] < 0.5, rates(got, ref)


@pytest.mark.parametrize("seed", SEEDS)
def test_default_floor_case_inputs_are_unchanged(seed):
    """floor_case() without a design is ~ batch + condition on the inputs it always had"""
    d = floor_case(seed)
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(d["counts"], dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(d["x"], dtype=np.float64).tobytes())
    assert d["counts"].shape == (500, 60) and d["x"].shape == (60, 4)
    assert h.hexdigest()[:16] == DIGESTS[seed]


@pytest.mark.parametrize("name", sorted(wide_cases.FLOOR))
def test_oracle_floor_regime_vs_lapack_wide(oracle, name):
    """the floor regime on a paired design (p = 21, the rolled kernels' widths) and on a 16-level factor: the same budgets"""
    from oracle import lapack_oracle
    d = wide_cases.floor_wide_case(name)
    assert d["x"].shape[1] >= 11
    assert_visible_parity(visible_chain(oracle, d), visible_chain(lapack_oracle, d), "oracle " + name)
