"""Flow-seeded initial state, host formula (initial_state(..., flow=f)): the
host copy of gqmap_init_state_flow.  No device."""
import numpy as np
import pytest

from tests._initflow import make_flow

OPTS = dict(L=3, minu=-2.0, maxu=3.0, minv=-1.0, maxv=0.5, temperature=0.2)


@pytest.mark.parametrize("L", [1, 3])
def test_flow_overlay_touches_component_zero_of_the_mean_only(L):
    from gqmap_opticalflow_amd import initial_state
    o = dict(OPTS, L=L)
    M, N = 7, 9
    f = make_flow(M, N)
    base = initial_state(o, M, N, seed=3)
    st = initial_state(o, M, N, seed=3, flow=f)
    for k in ("sigu", "sigv", "pn", "rou", "w", "alpha"):
        assert np.array_equal(getattr(st, k), getattr(base, k)), k
    assert st.it == base.it and st.T == base.T
    assert np.array_equal(st.muu[:, :, 1:], base.muu[:, :, 1:])
    assert np.array_equal(st.muv[:, :, 1:], base.muv[:, :, 1:])
    known = ~(np.isnan(f) | (np.abs(f) > 1e9))
    assert known.sum() == f.size - 5
    for plane, bplane, q, lo, hi in ((st.muu, base.muu, 0, o["minu"], o["maxu"]),
                                     (st.muv, base.muv, 1, o["minv"], o["maxv"])):
        x, k = f[:, :, q], known[:, :, q]
        assert np.array_equal(plane[:, :, 0][k], np.clip(x[k], lo, hi))
        assert np.array_equal(plane[:, :, 0][~k], bplane[:, :, 0][~k])  # NaN / 1e10 keep the draw
        assert (x[k] < lo).any() and (x[k] > hi).any()                  # clamping happens on both sides
        assert plane[:, :, 0].min() >= lo and plane[:, :, 0].max() <= hi


def test_flow_shape_is_checked_and_no_flow_is_the_old_state():
    from gqmap_opticalflow_amd import initial_state
    with pytest.raises(ValueError):
        initial_state(OPTS, 5, 6, flow=np.zeros((6, 5, 2)))
    a, b = initial_state(OPTS, 5, 6, seed=1), initial_state(OPTS, 5, 6, seed=1, flow=None)
    assert np.array_equal(a.muu, b.muu) and np.array_equal(a.muv, b.muv)
