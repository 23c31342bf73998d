"""gqmap_structure_texture (HIP kernels) against gqmap_structure_texture_host:
the two compile one header (csrc/gqmap_rof.h), so texture and structure agree
BIT FOR BIT, whatever T (iterations per launch: 1 = the plain kernel, 2, 4, 8 =
the fused LDS-tile kernel).  The host model itself is checked against the numpy
restatement and the reference's frames in tests/test_structure_texture.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _structure_texture_np as R

pytestmark = pytest.mark.gpu

ALL_T = (1, 2, 4, 8)


def _debug(name, *args):
    from gqmap_opticalflow_amd import _lib
    f = getattr(_lib.load(), name)
    f.restype, f.argtypes = C.c_int, [C.c_int] * len(args)
    return f(*args)


def force_T(T):
    assert _debug("gqmap_debug_rof_T", T) == 0


def tile():
    return _debug("gqmap_debug_rof_tile")


def default_T():
    return _debug("gqmap_debug_rof_default_T")


@functools.lru_cache(maxsize=None)
def host(shape, Cn, theta, n_iter, alp):
    """(texture, structure) of the host model, computed once per case."""
    from gqmap_opticalflow_amd import structure_texture
    out = structure_texture(R.random_frames(shape, Cn), theta, n_iter, alp, host=True, structure=True)
    for a in out:
        a.setflags(write=False)
    return out


def assert_kernel_equals_host(shape, Cn, n_iter, theta=0.125, alp=0.95):
    from gqmap_opticalflow_amd import structure_texture
    tex, s = structure_texture(R.random_frames(shape, Cn), theta, n_iter, alp, structure=True)
    htex, hs = host(tuple(shape), Cn, theta, n_iter, alp)
    assert R.bits_equal(tex, htex), ("texture", shape, Cn, n_iter)
    assert R.bits_equal(s, hs), ("structure", shape, Cn, n_iter)


@pytest.mark.parametrize("shape", [(5, 7), (1, 64)], ids=str)
def test_frames_smaller_than_the_halo(shape):
    """Every cell of the halo lies outside the frame or is a frame border cell:
    the border rules, not staleness, decide them.  n_iter is above every T."""
    assert_kernel_equals_host(shape, 2, 2 * max(ALL_T) + 3)


@pytest.mark.parametrize("Cn", [1, 3])
def test_several_tiles_with_partial_tiles_on_both_axes(Cn):
    S = tile()
    for shape in ((S + 5, 3 * S + 7), (3 * S + 9, S + 3)):
        assert_kernel_equals_host(shape, Cn, 2 * default_T() + 3)


def test_whole_chunks_a_leftover_and_nothing():
    T = default_T()
    for n_iter in sorted({0, 1, T - 1, T, T + 1, 2 * T + 3}):
        assert_kernel_equals_host((70, 45), 2, n_iter)


@pytest.mark.parametrize("T", ALL_T)
def test_every_forced_T_gives_the_same_bits(T):
    """70 x 45 x 2: 3 x 2 tiles, partial on both axes; n_iter in
    (T - 1, T, T + 1, 2T + 3) for the forced T."""
    try:
        force_T(T)
        for n_iter in sorted({T - 1, T, T + 1, 2 * T + 3, 19}):
            assert_kernel_equals_host((70, 45), 2, n_iter)
    finally:
        force_T(0)


def test_illegal_T_is_refused():
    for T in (-1, 3, 16):
        assert _debug("gqmap_debug_rof_T", T) == -1
    assert default_T() in ALL_T


@pytest.mark.parametrize("T", ALL_T)
def test_inexact_products(T):
    """theta = 0.1, alp = 0.7: a contracted multiply-add would change bits."""
    try:
        force_T(T)
        assert_kernel_equals_host((70, 45), 2, 11, theta=0.1, alp=0.7)
    finally:
        force_T(0)


def test_full_rubberwhale_equals_the_reference_frames():
    """The kernel at its defaults against the frames the reference itself holds."""
    from gqmap_opticalflow_amd import load_pair, load_preprocessed
    T1, T2, _ = load_pair("rubberwhale", preprocessed=True)
    R1, R2, _ = load_preprocessed("RubberWhale")
    assert R.bits_equal(T1, R1) and R.bits_equal(T2, R2)


def test_elapsed_ms():
    from gqmap_opticalflow_amd import structure_texture
    tex, ms = structure_texture(R.random_frames((70, 45), 2), n_iter=5, timed=True)
    assert np.isfinite(ms) and ms > 0
    assert R.bits_equal(tex, host((70, 45), 2, 0.125, 5, 0.95)[0])


@pytest.mark.parametrize("case", ["constant", "nan", "theta0", "C9", "M0"])
def test_argument_errors_launch_nothing_further(case):
    """theta0, C9, M0 are refused before any launch; the constant and the NaN
    frame after the range reduction, the only kernel that runs."""
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    im, kw = R.bad_cases()[case]
    M, N, Cn = im.shape
    a = dict(M=M, theta=0.125)
    a.update(kw)
    tex = np.full(im.shape, 77.0, order="F")
    s = np.full(im.shape, 77.0, order="F")
    ms = C.c_double(-1.0)
    st = lib.gqmap_structure_texture(_lib.dptr(im), a["M"], N, Cn, a["theta"], 3, 0.95, _lib.dptr(tex), _lib.dptr(s),
                                     C.cast(C.byref(ms), _lib._D), 0)
    assert st == 1  # GQMAP_ERR_INVALID_ARG
    assert b"gqmap_structure_texture" in lib.gqmap_last_error()
    assert np.all(tex == 77.0) and np.all(s == 77.0) and ms.value == -1.0
